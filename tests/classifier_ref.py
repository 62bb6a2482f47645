"""Torch restatement of the classifier's step, from the text of include/ocrl_hip_classifier.h, in the dtype it is given (fp64 as the
reference, fp32 as torch's own evaluation): the head (tests/dqn_ref.q_forward: the chain is the Q head's), the soft-max cross-entropy
with the rule for labels outside [0, A), the accuracy on the lowest index of the maximum, the gradients by autograd, and the cases the
GPU tests run (tests/test_classifier_cpu.py checks the restatement on the same ones).

Hand-worked example of the out-of-range rule (test_classifier_cpu.py checks it through `ce_rule`): A = 2, B = 3,
    z = [[0, ln 3], [5, 5], [1, 0]], labels = [1, 0, 7]
    row 0: lse = ln(1 + 3) = ln 4, l = ln 4 - ln 3, p = (1/4, 3/4), dz = (1/4, -1/4) / 3, the maximum is index 1 = y: a hit
    row 1: lse = 5 + ln 2, l = ln 2, p = (1/2, 1/2), dz = (-1/2, 1/2) / 3, the tie's lowest index 0 = y: a hit
    row 2: label 7 is outside [0, 2): no loss, no hit, dz = 0
    scalars = ((ln 4 - ln 3 + ln 2) / 3, 2 / 3, 2): the denominators stay B = 3."""
import functools

import torch

from .dqn_ref import q_forward

SHAPES = [(1, 4, 2), (5, 8, 3), (16, 8, 4), (17, 12, 4), (9, 10, 4), (37, 128, 15), (64, 12, 64), (5, 1152, 4), (1040, 8, 4)]
LAYOUTS = {"none": ((), ()), "clf": ((64,), (1,)), "mlp": ((64, 64), (1, 1))}


def make_params(F, A, dims, seed=0, dtype=torch.float32):
    """[W_0, b_0, ..., W_out, b_out] in state_dict order, every entry uniform in +-1 / sqrt(fan_in) (nn.Linear's own range)"""
    g = torch.Generator().manual_seed(seed)
    ps, k = [], F
    for n in list(dims) + [A]:
        ps += [((torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5).to(dtype), ((torch.rand(n, generator=g) * 2 - 1) / k ** 0.5).to(dtype)]
        k = n
    return ps


@functools.lru_cache(maxsize=None)
def case(B, F, A, lname):
    """(features, parameters, labels) of a case on the CPU, built once: standard normal features, labels uniform over [0, A)"""
    gen = torch.Generator().manual_seed(131 + B)
    ps = make_params(F, A, LAYOUTS[lname][0], 61 + F)
    x = torch.randn(B, F, generator=gen)
    labels = torch.randint(0, A, (B,), generator=gen)
    return x, ps, labels


def lowest_argmax(z):
    """the lowest index of the maximum of every row, spelled out (no reliance on a library's tie rule)"""
    A = z.shape[1]
    at_max = z == z.max(dim=1, keepdim=True).values
    return torch.where(at_max, torch.arange(A, device=z.device).expand_as(z), torch.full_like(at_max, A, dtype=torch.int64)).min(dim=1).values


def ce_rule(z, labels):
    """scalars [3] of logits z [B, A] and labels [B] in z's dtype: (sum l_b / B, sum hit_b / B, the count of rows with a label in range)"""
    B, A = z.shape
    labels = labels.reshape(-1).to(z.device)
    valid = (labels >= 0) & (labels < A)
    y = labels.clamp(0, A - 1).reshape(-1, 1)
    m = z.max(dim=1, keepdim=True).values
    lse = (m + torch.log(torch.exp(z - m).sum(dim=1, keepdim=True))).squeeze(1)
    l = torch.where(valid, lse - z.gather(1, y).squeeze(1), torch.zeros_like(lse))
    hit = valid & (lowest_argmax(z.detach()) == y.squeeze(1))
    return torch.stack([l.sum() / B, hit.to(z.dtype).sum() / B, valid.to(z.dtype).sum()])


def ce_step(x, params, acts, labels, dtype=torch.float64):
    """(scalars [3], logits, dfeatures, [dw]) of the step in `dtype`, by autograd"""
    x = x.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    z = q_forward(x, ps, acts)
    scal = ce_rule(z, labels)
    grads = torch.autograd.grad(scal[0], [x] + ps)
    return scal.detach(), z.detach(), grads[0], list(grads[1:])


def train(params, acts, batches, lr, dtype):
    """the parameters after one torch.optim.Adam step (eps 1e-8) per batch (features, labels) on the restated loss, in `dtype`"""
    ps = [p.detach().to(dtype).clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ps, lr=lr)
    for x, labels in batches:
        opt.zero_grad()
        ce_rule(q_forward(x.to(dtype), ps, acts), labels)[0].backward()
        opt.step()
    return [p.detach() for p in ps]


class StubPooling:
    """what Classifier needs of a pooling head, with nothing behind it: the observations are the features themselves"""
    _learn_aux_loss = _learn_downstream_loss = False

    def __init__(self, rep_dim):
        self.rep_dim = int(rep_dim)

    def __call__(self, obs, with_loss=False):
        return (obs, {}) if with_loss else obs

    def set_zero_grad(self):
        pass

    def do_step(self):
        pass

    def train(self):
        pass

    def eval(self):
        pass

    def to(self, device):
        pass

    def save(self):
        return {}

    def load(self, checkpoint):
        pass
