"""Generate the golden vectors of the slot property probe from the reference's own ``PropertyPredictor``.

Runs ONLY in the build container (needs /root/reference and scipy): imports ``utils.property_predictor`` with ``wandb`` and
``utils.tools`` stubbed, gives it a stand-in encoder that returns seeded rows (``rows``), closed-form head weights (``closed_form``,
the last layer scaled by a gain) and seeded targets (``targets``), and runs ``get_loss`` and ``loss.backward()`` in fp64.  It writes
tests/golden/probe.npz: per case the state_dict names and shapes, the head outputs, the cost matrices, ``col``, the loss, every
metric, and every parameter gradient (whole when it has at most FULL_MAX entries, else moments and a strided sample); for the wide
case (head outputs fed to the matching directly) outputs, costs, ``col``, loss and metrics.

Uniqueness of the matching is a condition on the fixture: per image the gap between the best and the second-best assignment (fp64)
must exceed 1000 times the largest difference between the fp32 and fp64 cost entries, or the case is not written; the gain of the
last layer is doubled until it holds and is recorded in the inventory.

The helpers below need neither the reference nor a GPU: the tests import them to rebuild the same inputs, ``ref_probe`` is the
vectorised fp64 torch restatement of the reference's loss that the fixture pins, and ``dp_assign`` is the bit-mask assignment of the
kernel written in numpy.

    python tests/golden/make_golden_probe.py
"""
import contextlib
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

PROPERTY_ORDER = ["color", "shape", "scale", "xy"]
NUM_CANDIDATES = dict(color=7, shape=4, scale=2)
# tag: encoder name, batch, slots K, objects N, rep_dim D, model_type
CASES = {
    "slate_mlp3": ("SLATE", 4, 6, 5, 192, "mlp3"),
    "slate_linear": ("SLATE", 4, 6, 5, 192, "linear"),
    "iodine_mlp3": ("Iodine", 3, 7, 5, 64, "mlp3"),
    "vae_mlp3": ("VAE", 3, 6, 5, 256, "mlp3"),
    "nk_linear": ("SlotAttn", 3, 6, 6, 192, "linear"),
}
WIDE = ("wide", 4, 12, 9)            # tag, batch, K = the built limit, N: head outputs go to ocrl_probe_match directly
NSAMPLE = 257
FULL_MAX = 4096
MARGIN = 1000.0


def fixture_path():
    return os.path.join(HERE, "probe.npz")


def dataset_config():
    ns = types.SimpleNamespace
    props = {k: ns(num_candidates=v) for k, v in NUM_CANDIDATES.items()}
    props["xy"] = ns(dims=2)
    return ns(property_order_in_state=list(PROPERTY_ORDER), properties=props)


def probe_config(tag):
    return types.SimpleNamespace(matching_mode="loss", model_type=CASES[tag][5], num_slots_for_dist_rep=CASES[tag][2],
                                 learning=types.SimpleNamespace(lr=1e-4))


def schema():
    """(target ranges, output ranges, kinds) of the default property order: kind 1 is xy"""
    tgt, out, kind = [], [], []
    t = o = 0
    for name in PROPERTY_ORDER:
        w = 2 if name == "xy" else NUM_CANDIDATES[name]
        tw = 2 if name == "xy" else 1
        tgt.append([t, t + tw]); out.append([o, o + w]); kind.append(int(name == "xy"))
        t, o = t + tw, o + w
    return tgt, out, kind


class StandInEncoder:
    """what PropertyPredictor touches of an encoder wrapper; returns the recorded rows whatever the observation"""

    def __init__(self, name, x):
        self.name, self._x = name, x
        self.rep_dim = x.shape[-1]
        self.num_slots = x.shape[1] if x.dim() == 3 else 1

    def __call__(self, obs):
        return self._x

    def set_zero_grad(self): pass
    def do_step(self): pass
    def train(self): pass
    def eval(self): pass
    def to(self, device): self._x = self._x.to(device)
    def save(self): return {}
    def load(self, checkpoint): pass


def rows(tag, dtype=torch.float64):
    """the encoder output of a case: [B, K, D] slots, [B, D] for the VAE"""
    name, B, K, N, D, _ = CASES[tag]
    g = torch.Generator().manual_seed(100 + list(CASES).index(tag))
    shape = (B, D) if name == "VAE" else (B, K, D)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def targets(B, N, seed, dtype=torch.float64):
    """[B, N, 5]: colour, shape and scale indices, x, y"""
    g = torch.Generator().manual_seed(200 + seed)
    cols = [torch.randint(0, NUM_CANDIDATES[k], (B, N, 1), generator=g).double() for k in ("color", "shape", "scale")]
    cols.append(0.1 + 0.8 * torch.rand(B, N, 2, generator=g, dtype=torch.float64))
    return torch.cat(cols, -1).to(dtype)


def case_targets(tag, dtype=torch.float64):
    return targets(CASES[tag][1], CASES[tag][3], list(CASES).index(tag), dtype)


def wide_inputs(gain, dtype=torch.float64):
    """head outputs [B, K, 15] and targets of the wide case"""
    _, B, K, N = WIDE
    g = torch.Generator().manual_seed(300)
    out = torch.randn(B, K, 15, generator=g, dtype=torch.float64) * gain
    return out.to(dtype), targets(B, N, 99, dtype)


def closed_form(shape, t, gain=1.0):
    """tensor t of the head: a pseudo-random pattern in closed form (phases from exact integer arithmetic: the quadratic term keeps a
    weight matrix from being a sum of a few outer products), weights scaled by gain / sqrt(fan_in)"""
    n = int(np.prod(shape))
    k = torch.arange(n, dtype=torch.int64)
    p1 = ((k * k * 7 + 13 * (t + 1) * k + 101 * t) % 1009).double() / 1009.0
    p2 = ((k * k * 3 + 29 * k + 17 * t) % 2003).double() / 2003.0
    v = torch.sin(2 * math.pi * p1 + 0.3) + 0.35 * torch.cos(2 * math.pi * p2)
    if len(shape) >= 2:
        v = v * (1.6 * gain / math.sqrt(shape[1]))
    else:
        v = v * 0.05
    return v.reshape(shape)


def load_closed_form(module, gain):
    """closed-form weights into an nn.Sequential head; the gain applies to the last Linear's weight"""
    named = list(module.named_parameters())
    with torch.no_grad():
        for t, (n, p) in enumerate(named):
            last_w = t == len(named) - 2
            p.copy_(closed_form(tuple(p.shape), t, gain if last_w else 1.0).to(p.dtype))


def dp_assign(C):
    """exact minimum-cost assignment of the N rows of C [N, K] to distinct columns, as the kernel does it: best[mask] = min over s in
    mask of best[mask \\ s] + C[popcount(mask) - 1, s], ties to the lowest s (strict <), the end state to the lowest mask -> col [N]"""
    C = np.asarray(C)
    N, K = C.shape
    best = np.full(1 << K, np.inf, dtype=C.dtype)
    choice = np.zeros(1 << K, dtype=np.int64)
    best[0] = 0
    pop = np.array([bin(m).count("1") for m in range(1 << K)])
    for c in range(1, N + 1):
        for mask in np.nonzero(pop == c)[0]:
            v, bs = np.inf, -1
            for s in range(K):
                if (mask >> s) & 1:
                    cand = best[mask ^ (1 << s)] + C[c - 1, s]
                    if cand < v:
                        v, bs = cand, s
            best[mask], choice[mask] = v, bs
    end = np.nonzero(pop == N)[0]
    mask = int(end[np.argmin(best[end])])          # argmin returns the first (lowest mask) of equal values
    col = np.zeros(N, dtype=np.int64)
    for o in range(N - 1, -1, -1):
        col[o] = choice[mask]
        mask ^= 1 << int(col[o])
    return col


def head_forward(x, params, slope=0.01):
    """the nn.Sequential head over a list of parameters in state_dict order"""
    n = len(params) // 2
    for l in range(n):
        x = F.linear(x, params[2 * l], params[2 * l + 1])
        if l < n - 1:
            x = F.leaky_relu(x, slope)
    return x


def match_loss(out, y, col=None):
    """the reference's costs, matching, loss and metrics on head outputs out [B, K, O] and targets y [B, N, T] (default schema)"""
    tgt, outr, kind = schema()
    B, K, _ = out.shape
    N = y.shape[1]
    cost = out.new_zeros(B, N, K)
    for (t, _), (a, b), k in zip(tgt, outr, kind):
        if k:
            cost = cost + ((out[:, None, :, a:b] - y[:, :, None, t:t + 2]) ** 2).mean(-1)
        else:
            lp = F.log_softmax(F.softmax(out[..., a:b], -1), -1)                  # the soft-max taken twice, as the reference does
            idx = y[..., t].long()[:, :, None].expand(B, N, K)
            cost = cost - lp.transpose(1, 2).gather(1, idx)
    if col is None:
        col = np.stack([dp_assign(c) for c in cost.detach().cpu().numpy()])
    colt = torch.as_tensor(col, dtype=torch.long, device=out.device)
    loss = cost.gather(2, colt[:, :, None]).sum()
    om = out.gather(1, colt[:, :, None].expand(B, N, out.shape[2]))               # matched outputs [B, N, O]
    metrics = {"loss": loss}
    for name, (t, _), (a, b), k in zip(PROPERTY_ORDER, tgt, outr, kind):
        if k:
            yt = y[..., t:t + 2]
            mean = yt.mean(1, keepdim=True)
            metrics[f"R^2_{name}"] = (((om[..., a:b] - mean) ** 2).sum(1) / ((yt - mean) ** 2).sum(1)).mean()
            metrics[f"mse_{name}"] = ((om[..., a:b] - yt) ** 2).sum(-1).sqrt().mean()
        else:
            metrics[f"acc_{name}"] = (om[..., a:b].argmax(-1) == y[..., t]).to(out.dtype).mean()
    return dict(out=out, cost=cost, col=np.asarray(col), loss=loss, metrics=metrics)


def ref_probe(x, params, y, K, slope=0.01):
    """fp64 (or the dtype of its inputs) restatement of PropertyPredictor.get_loss: x [B, K, D] slots or [B, D] (VAE, K pseudo-slots)"""
    B = x.shape[0]
    out = head_forward(x.reshape(B * K, -1) if x.dim() == 3 else x, params, slope).reshape(B, K, -1)
    return match_loss(out, y)


METRIC_NAMES = ["loss", "acc_color", "acc_shape", "acc_scale", "R^2_xy", "mse_xy"]


def metric_vector(metrics):
    return np.array([float(metrics[k].detach()) for k in METRIC_NAMES])


def moments(a):
    a = np.asarray(a, dtype=np.float64).ravel()
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), a.max(), a.min()])


def sample_idx(n):
    return np.linspace(0, n - 1, min(n, NSAMPLE)).round().astype(np.int64)


def second_best_gap(C, col):
    """cost of the best assignment that differs from col, minus col's: every other assignment avoids at least one edge of col"""
    from scipy.optimize import linear_sum_assignment
    base = C[np.arange(len(col)), col].sum()
    alt = np.inf
    for o in range(len(col)):
        D = C.copy()
        D[o, col[o]] = 1e30
        r, c = linear_sum_assignment(D)
        alt = min(alt, D[r, c].sum())
    return alt - base


def unique_enough(cost64, cost32, col):
    """per image: gap to the second-best assignment > MARGIN x the largest fp32-vs-fp64 cost difference -> (ok, min gap, max diff)"""
    gaps = [second_best_gap(c, k) for c, k in zip(cost64, col)]
    diff = np.abs(cost64 - cost32.astype(np.float64)).reshape(len(cost64), -1).max(1)
    return all(g > MARGIN * d for g, d in zip(gaps, diff)), float(min(gaps)), float(diff.max())


@contextlib.contextmanager
def _reference_imports():
    """import utils.property_predictor with wandb and utils.tools stubbed (they pull wandb, omegaconf, sb3)"""
    import typing
    names = ("wandb", "utils", "utils.tools", "utils.property_predictor")
    saved = {k: sys.modules.get(k) for k in names}
    tools = types.ModuleType("utils.tools")
    for k in typing.__all__:
        setattr(tools, k, getattr(typing, k))
    tools.Tensor, tools.torch, tools.np = torch.Tensor, torch, np
    tools.__all__ = [k for k in vars(tools) if not k.startswith("_")]
    utils = types.ModuleType("utils")
    utils.__path__ = [os.path.join(REF, "utils")]
    utils.tools = tools
    sys.modules.update({"wandb": types.ModuleType("wandb"), "utils": utils, "utils.tools": tools})
    sys.path.insert(0, REF)
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # the reference builds its loss matrix with torch.zeros(...): fp64 throughout
    try:
        import importlib
        yield importlib.import_module("utils.property_predictor")
    finally:
        torch.set_default_dtype(default)
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def main():
    from scipy.optimize import linear_sum_assignment
    out, inventory = {}, {}
    with _reference_imports() as pm:
        for tag, (name, B, K, N, D, model_type) in CASES.items():
            x, y = rows(tag), case_targets(tag)
            gain = 1.0
            while True:
                pp = pm.PropertyPredictor(StandInEncoder(name, x), probe_config(tag), dataset_config())
                pp._module.double()
                load_closed_form(pp._module, gain)
                params = list(pp._module.parameters())
                r64 = ref_probe(x, params, y, K)
                r32 = ref_probe(x.float(), [p.detach().float() for p in params], y.float(), K)
                ok, gap, diff = unique_enough(r64["cost"].detach().numpy(), r32["cost"].numpy(), r64["col"])
                if ok:
                    break
                gain *= 2.0
                assert gain <= 64.0, f"{tag}: no unique matching up to gain 64 (gap {gap:.3e}, fp32 difference {diff:.3e})"
            metrics = pp.get_loss({"obss": None, "objs": y})
            metrics["loss"].backward()
            # the reference's own matching, recomputed as it computes it, must be the restatement's
            ref_col = np.stack([linear_sum_assignment(c)[1] for c in r64["cost"].detach().numpy()])
            assert np.array_equal(ref_col, r64["col"]), tag
            assert np.allclose(metric_vector(metrics), metric_vector(r64["metrics"]), rtol=1e-12, atol=0), tag
            inventory[tag] = dict(params=[[k, list(v.shape)] for k, v in pp._module.state_dict().items()], gain=gain, gap=gap, fp32_diff=diff)
            p = tag + "/"
            out[p + "out"] = r64["out"].detach().numpy()
            out[p + "cost"] = r64["cost"].detach().numpy()
            out[p + "col"] = ref_col.astype(np.int32)
            out[p + "metrics"] = metric_vector(metrics)
            for k, prm in pp._module.named_parameters():
                g = prm.grad.numpy().ravel()
                if g.size <= FULL_MAX:
                    out[p + "grad/" + k] = g.astype(np.float64)
                else:
                    out[p + "gradm/" + k], out[p + "grads/" + k] = moments(g), g[sample_idx(g.size)]
            print(f"{tag}: gain {gain}, loss {metrics['loss'].item():.6f}, smallest gap {gap:.3e}, fp32 cost difference {diff:.3e}")
    # the wide case: scipy on the restatement's costs (the reference's head is not involved; its matching call is)
    tag, B, K, N = WIDE
    gain = 1.0
    while True:
        o64, y = wide_inputs(gain)
        r64 = match_loss(o64, y)
        r32 = match_loss(o64.float(), y.float())
        ok, gap, diff = unique_enough(r64["cost"].numpy(), r32["cost"].numpy(), r64["col"])
        if ok:
            break
        gain *= 2.0
        assert gain <= 64.0, f"wide: no unique matching (gap {gap:.3e}, fp32 difference {diff:.3e})"
    ref_col = np.stack([linear_sum_assignment(c)[1] for c in r64["cost"].numpy()])
    assert np.array_equal(ref_col, r64["col"])
    inventory[tag] = dict(gain=gain, gap=gap, fp32_diff=diff)
    out["wide/out"], out["wide/cost"], out["wide/col"] = o64.numpy(), r64["cost"].numpy(), ref_col.astype(np.int32)
    out["wide/metrics"] = metric_vector(r64["metrics"])
    print(f"wide: gain {gain}, loss {r64['loss'].item():.6f}, smallest gap {gap:.3e}, fp32 cost difference {diff:.3e}")
    out["inventory"] = np.array(json.dumps(inventory))
    np.savez_compressed(fixture_path(), **out)
    print(f"wrote {fixture_path()} ({os.path.getsize(fixture_path())} bytes)")


if __name__ == "__main__":
    main()
