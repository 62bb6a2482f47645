"""Reference, cases and grader of the slot-attention input chain x = W2 relu(W0 LN(e4) + b0) + b2 over [R, 64] rows (csrc/sa_input.hip
through ocrl_sa_input_fwd / _bwd, include/ocrl_hip.h), shared by the CPU suite (tests/test_sa_input_ref_cpu.py) and the GPU suite
(tests/test_gpu_sa_input.py).

Reference: the chain in float64 under autograd, loss = sum(x * dx); mean and rstd are LayerNorm's row statistics (eps = 1e-5).

ReLU guard (the rule of tests/slot_attn_ref.py): the reference is fp64 and the kernel fp32, so a hidden unit whose pre-activation lies
within rounding of zero can take the other branch in the kernel and move a gradient by far more than rounding.  The inputs of a case
come from the first seed base, base + 1, ... (at most MAX_SEEDS) whose fp64 mlp.0 pre-activations all stay at |.| >= RELU_GUARD = 1e-5.

Error measure of every quantity: max|a - b| / max|ref|; a non-finite difference counts as infinite.  The grader takes the bar of each
quantity from its caller: the GPU suite measures the unfused chain's error on the same inputs and allows the fused form twice that (only
the order of the row sums changes); the CPU suite grades the fp32 restatement at TOL, the fp32 unit-kernel tolerance of
tests/test_gpu_kernels.py."""
import ctypes
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

C = 64
EPS = 1e-5
TOL = 2e-5
RELU_GUARD = 1e-5
MAX_SEEDS = 8
OUTPUTS = ("mean", "rstd", "h1", "x", "de4")
GRADS = ("dW0", "db0", "dW2", "db2", "dgamma", "dbeta")
QUANTITIES = OUTPUTS + GRADS

Case = namedtuple("Case", "name R max_wgs")


def plan(R):
    """ocrl_sa_input_plan: dict(tile, wgs, slab) -- rows per tile, workgroups at max_wgs = 0, floats per workgroup slab (host only)"""
    from ocrl_amd import _lib
    out = (ctypes.c_int * 3)()
    _lib.check(_lib.lib().ocrl_sa_input_plan(R, ctypes.byref(out)))
    return dict(zip(("tile", "wgs", "slab"), out))


@functools.lru_cache(maxsize=None)
def cases():
    """row counts around the tile size the plan reports, 1000, and 5 tiles walked by 2 workgroups"""
    t = plan(1000)["tile"]
    return [Case("1", 1, 0), Case("tile-1", t - 1, 0), Case("tile", t, 0), Case("tile+1", t + 1, 0), Case("2tile+5", 2 * t + 5, 0),
            Case("1000", 1000, 0), Case("5tiles-2wgs", 5 * t, 2)]


CASE_NAMES = ["1", "tile-1", "tile", "tile+1", "2tile+5", "1000", "5tiles-2wgs"]


def case(name):
    return next(c for c in cases() if c.name == name)


def make_inputs(R, seed):
    """dict of fp32 tensors: gamma 1 + 0.1 N(0,1), beta and the biases 0.1 N(0,1) (nonzero), W0 / W2 N(0,1) / 8 (not symmetric), e4 rows with
    their own offset and scale, dx N(0,1)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(gamma=1.0 + 0.1 * rn(C), beta=0.1 * rn(C), W0=rn(C, C) / 8, b0=0.1 * rn(C), W2=rn(C, C) / 8, b2=0.1 * rn(C),
                e4=rn(R, C) * (0.5 + torch.rand(R, 1, generator=g)) + 0.3 * rn(R, 1), dx=rn(R, C))


def reference(inp, dtype=torch.float64):
    """every quantity of QUANTITIES in `dtype`, and min_pre = the smallest |mlp.0 pre-activation|"""
    p = {k: v.to(dtype).clone().requires_grad_(k != "dx") for k, v in inp.items()}
    e4 = p["e4"]
    mean = e4.mean(-1)
    rstd = (e4.var(-1, unbiased=False) + EPS).rsqrt()
    ln = F.layer_norm(e4, (C,), p["gamma"], p["beta"], EPS)
    pre = ln @ p["W0"].T + p["b0"]
    h1 = torch.relu(pre)
    x = h1 @ p["W2"].T + p["b2"]
    (x * p["dx"]).sum().backward()
    return dict(mean=mean.detach(), rstd=rstd.detach(), h1=h1.detach(), x=x.detach(), de4=e4.grad, dW0=p["W0"].grad, db0=p["b0"].grad,
                dW2=p["W2"].grad, db2=p["b2"].grad, dgamma=p["gamma"].grad, dbeta=p["beta"].grad, min_pre=float(pre.detach().abs().min()))


Prepared = namedtuple("Prepared", "case seed tried inputs ref")


@functools.lru_cache(maxsize=None)
def prepare(c):
    """the inputs of a case (first guarded seed) and their fp64 reference; computed once per process, shared, never modified"""
    base = 7000 + 10 * c.R + c.max_wgs
    for j in range(MAX_SEEDS):
        inp = make_inputs(c.R, base + j)
        ref = reference(inp)
        if ref["min_pre"] >= RELU_GUARD:
            return Prepared(c, base + j, j + 1, inp, ref)
    raise AssertionError(f"R = {c.R}: no seed in {base}..{base + MAX_SEEDS - 1} keeps every mlp.0 pre-activation at >= {RELU_GUARD:g}")


@functools.lru_cache(maxsize=None)
def cpu32(c):
    """the fp32 CPU restatement on the prepared inputs"""
    return reference(prepare(c).inputs, torch.float32)


# ---- grader
def _worst(a, b):
    d = (a.detach().double().cpu() - b.detach().double().cpu()).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    i = int(d.argmax())
    return float(d.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), d.shape))


def errors(ref, got):
    """{quantity: (max|got - ref| / max|ref|, index of the worst element)}"""
    out = {}
    for k in QUANTITIES:
        assert tuple(got[k].shape) == tuple(ref[k].shape), (k, tuple(got[k].shape), tuple(ref[k].shape))
        d, idx = _worst(got[k], ref[k])
        out[k] = (d / max(float(ref[k].abs().max()), 1e-30), idx)
    return out


def grade(ref, got, bars, tag=""):
    """asserts error <= bar for every quantity (bars: {quantity: bar} or one number); the failure message names every quantity over its
    bar, the worst first, and the element the error sits at; returns {quantity: error}"""
    e = errors(ref, got)
    bar = (lambda k: bars[k]) if isinstance(bars, dict) else (lambda k: bars)
    bad = sorted((k for k in QUANTITIES if not e[k][0] <= bar(k)), key=lambda k: -e[k][0] / max(bar(k), 1e-300))
    assert not bad, tag + "; ".join(f"{k} error {e[k][0]:.3e} > {bar(k):.3e} at {k}{list(e[k][1])}" for k in bad)
    return {k: v[0] for k, v in e.items()}
