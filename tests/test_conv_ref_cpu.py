"""CPU-only: tests/conv_ref.py, the float64 reference the convolution kernels are graded against, agrees with torch's autograd -- the
mask rules are the ELU / ReLU derivatives, the transposed form is the input gradient of F.conv2d, and the two together are the
backward of a conv -> activation -> conv chain.  No device is touched."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_elu_mask_rule_is_the_elu_derivative_including_exact_zeros():
    g = _g(1)
    x = torch.randn(4, 64, 7, 9, generator=g, dtype=torch.double) * 2
    x.view(-1)[::37] = 0.0                                      # pre-activations that are exactly 0: ELU'(0) = 1, m = 0 is "not > 0"
    assert int((x == 0).sum()) > 100
    x.requires_grad_(True)
    dy = torch.randn(4, 64, 7, 9, generator=g, dtype=torch.double)
    m = F.elu(x)
    m.backward(dy)
    neg = m.detach()[x.detach() < 0]
    assert neg.min() > -1 and neg.max() < 0
    got = R.apply_mask(dy, m.detach(), mask_elu=True)
    assert (got - x.grad).abs().max().item() < 1e-15
    assert torch.equal(got[x.detach() == 0], dy[x.detach() == 0])


def test_relu_mask_rule_is_the_relu_derivative_away_from_zero():
    g = _g(2)
    x = torch.randn(4, 64, 7, 9, generator=g, dtype=torch.double)
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 0.5), x).requires_grad_(True)
    dy = torch.randn(4, 64, 7, 9, generator=g, dtype=torch.double)
    m = F.relu(x)
    m.backward(dy)
    assert torch.equal(R.apply_mask(dy, m.detach(), mask_elu=False), x.grad)
    # an independent mask tensor decides by its sign alone
    act = torch.randn(4, 64, 7, 9, generator=g, dtype=torch.double)
    assert torch.equal(R.apply_mask(dy, act), dy * (act > 0))


@pytest.mark.parametrize("ks,B,H,W", [(5, 2, 1, 1), (5, 1, 3, 5), (3, 2, 7, 33), (5, 1, 9, 6), (3, 1, 1, 4)])
def test_transposed_form_is_the_input_gradient(ks, B, H, W):
    g = _g(ks * 100 + H * W)
    x = torch.randn(B, 64, H, W, generator=g)
    w = torch.randn(64, 64, ks, ks, generator=g) / (64 * ks * ks) ** 0.5
    dy = torch.randn(B, 64, H, W, generator=g)
    dx, dw, db = R.conv_grads(x, w, dy)
    got = R.conv_backward_data(dy, w)
    assert got.dtype == torch.double and got.shape == dx.shape
    assert (got - dx).abs().max().item() < 1e-12 * max(1.0, dx.abs().max().item())
    assert (db - dy.double().sum((0, 2, 3))).abs().max().item() < 1e-12 * max(1.0, db.abs().max().item())
    assert dw.shape == w.shape


def test_transposed_weight_swaps_channels_and_flips_taps():
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.double).reshape(2, 3, 3, 3)
    t = R.transposed_weight(w)
    assert t.shape == (3, 2, 3, 3)
    for co in range(2):
        for ci in range(3):
            for ky in range(3):
                for kx in range(3):
                    assert t[ci, co, 2 - ky, 2 - kx] == w[co, ci, ky, kx]


@pytest.mark.parametrize("act", [1, 2])
def test_forward_order_and_chain_backward(act):
    """y = act(conv(x) + b) + posmap (activation BEFORE the position map); the gradient that reaches conv's output through a second
    convolution is the transposed form of that second convolution masked with the activation's output"""
    g = _g(7 + act)
    ks, B, H, W = 3, 2, 5, 6
    x = torch.randn(B, 64, H, W, generator=g)
    w1 = torch.randn(64, 64, ks, ks, generator=g) / 24.0
    w2 = torch.randn(64, 64, ks, ks, generator=g) / 24.0
    b1 = torch.randn(64, generator=g)
    pm = torch.randn(64, H, W, generator=g)
    dz = torch.randn(B, 64, H, W, generator=g)
    pre = F.conv2d(x.double(), w1.double(), b1.double(), padding=1).requires_grad_(True)
    a = F.relu(pre) if act == 1 else F.elu(pre)
    y = a + pm.double()
    assert torch.equal(R.conv_forward(x, w1, b1, relu=act, posmap=pm), y.detach())
    F.conv2d(y, w2.double(), None, padding=1).backward(dz.double())
    got = R.conv_backward_data(dz, w2, mask=a.detach(), mask_elu=(act == 2))
    assert (got - pre.grad).abs().max().item() < 1e-12 * pre.grad.abs().max().item()
    # the full epilogue, step by step
    m = torch.randn(B, 64, H, W, generator=g)
    full = R.conv_forward(x, w1, b1, relu=act, posmap=pm, mask=m, mask_elu=True)
    assert torch.equal(full, torch.where(m.double() > 0, y.detach(), y.detach() * (m.double() + 1)))
    assert torch.equal(R.conv_forward(x, w1, b1, relu=act, posmap=pm, mask=m), y.detach() * (m > 0))
