"""Reference, cases and grader of the slot-attention kernel tests (csrc/slot_attn.hip through ocrl_slot_attention_fwd / _bwd and the
_mh_ pair, include/ocrl_hip.h), shared by the CPU suite (tests/test_slot_attn_ref_cpu.py: every case finds its inputs, the fp32
restatement passes the grader, the grader has teeth) and the GPU suite (tests/test_gpu_slot_attention.py, tests/sa_variant_worker.py).

Reference: oracle.slate_oracle.slot_attention in float64 under autograd, loss = sum(slots * dslots).

ReLU guard: the reference is fp64 and the kernel fp32, so a hidden unit of mlp.0 whose pre-activation lies within rounding of zero can
take the other branch in the kernel and move a weight-gradient row by far more than rounding.  The inputs of a case come from the first
seed base, base + 1, ... (at most MAX_SEEDS) whose fp64 reference keeps every mlp.0 pre-activation at |.| >= RELU_GUARD = 1e-5, ten
times the fp32 error scale of the operator (<= 1.5e-6 of the tensor's maximum).

Grader: slots, attn, dx, dslots0 by max|a - b| / max|ref|; a weight gradient by max|a - b| / max(max|ref|, 1e-4 gmax), gmax the largest
reference gradient of the case; all below TOL = 2e-5, the fp32 unit-kernel tolerance of tests/test_gpu_kernels.py.  A weight gradient
whose reference is identically zero (max|ref| <= 1e-9 gmax: norm_slots.bias at one head -- a common shift of all queries cancels in the
soft-max over the slots -- and norm_slots.weight, project_q.weight, project_k.weight too where the soft-max or the normalisation over
the positions has a single term, K = 1 or N = 1) holds only the rounding residue of sums whose terms cancel; it passes with
max|g| <= max(1e-7 gmax, 4 x the residue of the fp32 CPU restatement of the same case)."""
import ctypes
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import slate_oracle as O

PRE = "_slotattn.slot_attention."
NAMES = ["norm_inputs.weight", "norm_inputs.bias", "norm_slots.weight", "norm_slots.bias", "norm_mlp.weight", "norm_mlp.bias",
         "project_q.weight", "project_k.weight", "project_v.weight", "gru.weight_ih", "gru.weight_hh", "gru.bias_ih", "gru.bias_hh",
         "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"]
TENSORS = ("slots", "attn", "dx", "dslots0")
AXES = dict(slots=("image", "slot", "column"), attn=("image", "position", "slot"), dx=("image", "position", "channel"),
            dslots0=("image", "slot", "column"))
C = 64
TOL = 2e-5                  # tests/test_gpu_kernels.py TOL
ATTN_SUM_TOL = 2e-6         # |sum over the slots of attn - 1|
RELU_GUARD = 1e-5
MAX_SEEDS = 8
ZERO_REF = 1e-9             # a reference gradient below this share of gmax is identically zero
ZERO_FLOOR = 1e-7           # what the weight-gradient floor (1e-4 gmax) and the former tolerance (1e-3) implied for such a tensor
GRAD_FLOOR = 1e-4

Case = namedtuple("Case", "B N K D H I heads")


def shapes(D, H):
    return [(C,), (C,), (D,), (D,), (D,), (D,), (D, D), (D, C), (D, C), (3 * D, D), (3 * D, D), (3 * D,), (3 * D,), (H, D), (H,), (D, H), (D,)]


# ---- the cases
# the 14 shapes this kernel was tested at before; the last four single-head ones take several streaming workgroups per image
EXISTING = [Case(*c) for c in [(3, 200, 5, 128, 192, 3, 1), (2, 1024, 6, 192, 192, 3, 1), (2, 77, 16, 64, 64, 2, 1), (1, 16, 1, 256, 256, 1, 1),
                               (2, 300, 11, 192, 128, 2, 1), (3, 2100, 6, 192, 192, 3, 1), (2, 4099, 16, 64, 64, 2, 1), (2, 8200, 11, 192, 128, 2, 1),
                               (1, 4096, 1, 128, 64, 3, 1),
                               # several heads: 12, 12, 16, 16 and 15 soft-max columns; head widths 96, 32, 16, 96, 64
                               (2, 1024, 6, 192, 192, 3, 2), (3, 200, 3, 128, 192, 3, 4), (2, 4099, 4, 64, 64, 2, 4), (1, 2100, 8, 192, 128, 2, 2),
                               (2, 300, 5, 192, 192, 3, 3)]]
N_A = 261       # 17 position tiles, the last one of 5 positions: two streaming workgroups per image
# A: every slot count, three iterations (first / middle / final backward variants); K <= 8: one full group of 16 / K images + a group of one
SET_A = [Case(16 // K + 1 if K <= 8 else 2, N_A, K, 64, 64, 3, 1) for K in range(1, 17)]
# B: one iteration (first and final at once) and two; 3 position tiles, fewer than the 4 waves of a streaming workgroup
SET_B = [Case(3, 37, K, 64, 64, I, 1) for I in (1, 2) for K in (2, 8, 9, 16)]
# C: tiny N
SET_C = [Case(2, N, K, 64, 64, 2, 1) for N in (1, 15, 16, 17) for K in (3, 10)]
# D: slot / MLP widths on both sides of the LDS limit of the grouped form
WIDTHS_D = [(192, 192), (192, 256), (256, 256), (256, 64)]
KS_D = (1, 2, 3, 4, 5, 8)
SET_D = [Case(16 // K + 1, 130, K, D, H, 2, 1) for K in KS_D for D, H in WIDTHS_D]
# E: every head split, every soft-max column count 2..16
SET_E = ([Case(3, N_A, K, 64, 64, 3, 2) for K in range(1, 9)] + [Case(3, N_A, K, 192, 64, 3, 3) for K in range(1, 6)] +
         [Case(3, N_A, K, 64, 64, 3, 4) for K in range(1, 5)] + [Case(3, N_A, K, 128, 64, 3, 8) for K in (1, 2)] + [Case(3, N_A, 1, 256, 64, 3, 16)])
NEW = SET_A + SET_B + SET_C + SET_D + SET_E
ALL = EXISTING + NEW
PROPERTY_KS = (2, 7, 9, 13, 16)       # the property tests run set A's shape at these slot counts


def case_id(c):
    return f"B{c.B}-N{c.N}-K{c.K}-D{c.D}-H{c.H}-I{c.I}-h{c.heads}"


def base_seed(c):
    return c.B * 1000 + c.N + c.K


# ---- inputs and reference
def make_inputs(c, seed):
    """(P, x, slots0, dslots) fp32: LayerNorm weights 1 + 0.1 N(0,1), biases 0.1 N(0,1), matrices N(0,1) / sqrt(fan-in), the rest N(0,1)"""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for n, shp in zip(NAMES, shapes(c.D, c.H)):
        if n.endswith("weight") and len(shp) == 1:
            P[PRE + n] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif len(shp) == 1:
            P[PRE + n] = 0.1 * torch.randn(shp, generator=g)
        else:
            P[PRE + n] = torch.randn(shp, generator=g) / shp[1] ** 0.5
    x = torch.randn(c.B, c.N, C, generator=g)
    s0 = torch.randn(c.B, c.K, c.D, generator=g)
    dsl = torch.randn(c.B, c.K, c.D, generator=g)
    return P, x, s0, dsl


class _MinRelu:
    """records the smallest |pre-activation| of the F.relu calls made inside the block (slot_attention: mlp.0, once per iteration)"""

    def __enter__(self):
        self.min, self.calls, self._orig = float("inf"), 0, F.relu

        def relu(x, inplace=False):
            self.calls += 1
            self.min = min(self.min, float(x.detach().abs().min()))
            return self._orig(x)
        F.relu = relu
        return self

    def __exit__(self, *a):
        F.relu = self._orig


def reference(c, inputs, dtype=torch.float64):
    """slots, attn [B,N,K], dx, dslots0, grads {name: tensor}, min_pre (smallest |mlp.0 pre-activation|) of the oracle evaluated in `dtype`"""
    P, x, s0, dsl = inputs
    Pr = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    xr, sr = x.to(dtype).clone().requires_grad_(True), s0.to(dtype).clone().requires_grad_(True)
    with _MinRelu() as mr:
        slots, attn = O.slot_attention(Pr, xr, sr, c.I, heads=c.heads)
    assert mr.calls == c.I
    (slots * dsl.to(dtype)).sum().backward()
    return dict(slots=slots.detach(), attn=attn.detach().reshape(c.B, c.N, c.K), dx=xr.grad, dslots0=sr.grad,
                grads={n: Pr[PRE + n].grad for n in NAMES}, min_pre=mr.min)


Prepared = namedtuple("Prepared", "case seed tried inputs ref")


@functools.lru_cache(maxsize=None)
def prepare(c):
    """the inputs of a case (first guarded seed) and their fp64 reference; computed once per process, shared, never modified"""
    base = base_seed(c)
    for j in range(MAX_SEEDS):
        inputs = make_inputs(c, base + j)
        ref = reference(c, inputs)
        if ref["min_pre"] >= RELU_GUARD:
            return Prepared(c, base + j, j + 1, inputs, ref)
    raise AssertionError(f"{case_id(c)}: no seed in {base}..{base + MAX_SEEDS - 1} keeps every mlp.0 pre-activation at >= {RELU_GUARD:g}")


@functools.lru_cache(maxsize=None)
def cpu32(c):
    """the fp32 CPU restatement on the prepared inputs (the grader takes its zero-gradient residues; the CPU suite grades it)"""
    return reference(c, prepare(c).inputs, torch.float32)


def expected_zero(c):
    """names of the weight gradients that are identically zero for this case"""
    if c.N == 1 or (c.heads == 1 and c.K == 1):
        return {"norm_slots.weight", "norm_slots.bias", "project_q.weight", "project_k.weight"}
    return {"norm_slots.bias"} if c.heads == 1 else set()


# ---- grader
def _worst(a, b):
    """(max |a - b|, its index tuple); a non-finite difference counts as infinite"""
    d = (a.detach().double().cpu() - b.detach().double().cpu()).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    i = int(d.argmax())
    return float(d.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), d.shape))


def _where(name, idx):
    ax = AXES.get(name, ("row", "column"))
    return name + "[" + ", ".join(f"{a} {v}" for a, v in zip(ax, idx)) + "]"


def gmax_of(ref):
    return max(float(g.abs().max()) for g in ref["grads"].values())


def zero_class(ref):
    gm = gmax_of(ref)
    return {n for n, g in ref["grads"].items() if float(g.abs().max()) <= ZERO_REF * gm}


def errors(c, ref, got, res32):
    """{quantity: (error, bound, where)} of `got` (slots, attn, dx, dslots0, grads) against the fp64 reference `ref`; res32 = the fp32 CPU
    restatement of the same case"""
    out = {}
    for k in TENSORS:
        assert tuple(got[k].shape) == tuple(ref[k].shape), (k, got[k].shape, ref[k].shape)
        d, idx = _worst(got[k], ref[k])
        out[k] = (d / max(float(ref[k].abs().max()), 1e-30), TOL, _where(k, idx))
    gm = gmax_of(ref)
    zero = zero_class(ref)
    for n in NAMES:
        g, r = got["grads"][n], ref["grads"][n]
        assert tuple(g.shape) == tuple(r.shape), (n, g.shape, r.shape)
        d, idx = _worst(g, r)
        if n in zero:
            out[n] = (d / gm, max(ZERO_FLOOR, 4.0 * float(res32["grads"][n].abs().max()) / gm), _where(n, idx))
        else:
            out[n] = (d / max(float(r.abs().max()), GRAD_FLOOR * gm), TOL, _where(n, idx))
    return out


def check(c, e, tag="", log=None, seed=None):
    """asserts the errors `e` of errors(); the failure message names every quantity over its bound, the worst first, and the element the
    error sits at; returns {quantity: error}"""
    if log is not None:
        reg, zero = [n for n in NAMES if e[n][1] == TOL], [n for n in NAMES if e[n][1] != TOL]
        wg = max(reg, key=lambda n: e[n][0])
        msg = f" worst dW {wg}={e[wg][0]:.2e}"
        if zero:          # the identically zero gradients: residue / gmax and its bound
            wz = max(zero, key=lambda n: e[n][0] / e[n][1])
            msg += f" zero dW {wz}={e[wz][0]:.2e} (bound {e[wz][1]:.1e})"
        log(f"[slot_attention {tag}{case_id(c)}" + (f" seed {seed}] " if seed is not None else "] ") + " ".join(f"{k}={e[k][0]:.2e}" for k in TENSORS) + msg)
    bad = sorted((k for k in e if not e[k][0] < e[k][1]), key=lambda k: -e[k][0] / e[k][1])
    assert not bad, f"{tag}{case_id(c)}: " + "; ".join(f"{k} error {e[k][0]:.3e} >= {e[k][1]:.1e} at {e[k][2]}" for k in bad)
    return {k: v[0] for k, v in e.items()}


def grade(c, got, tag="", log=None):
    """asserts `got` against the prepared fp64 reference of case c (errors() + check())"""
    return check(c, errors(c, prepare(c).ref, got, cpu32(c)), tag, log, prepare(c).seed)


def attn_sum_error(attn):
    """(max |sum over the slots - 1|, (image, position))"""
    d = (attn.detach().double().cpu().sum(-1) - 1.0).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    i = int(d.argmax())
    return float(d.flatten()[i]), (i // d.shape[1], i % d.shape[1])


# ---- the kernel
def plan(K, D, H, heads):
    """ocrl_slot_attention_plan: dict(G, NB, KB, lds_fwd, lds_bwd, KS), or raises RuntimeError with the library's message"""
    from ocrl_amd import _lib
    out = (ctypes.c_int * 6)()
    _lib.check(_lib.lib().ocrl_slot_attention_plan(K, D, H, heads, ctypes.byref(out)))
    return dict(zip(("G", "NB", "KB", "lds_fwd", "lds_bwd", "KS"), out))


def run_kernel(c, inputs, want_attn=True, backward=True):
    """the HIP kernels on `inputs`: every output buffer and the workspace hold NaN before the forward call, and everything returned must
    be finite.  Returns CPU tensors: slots, attn (None without want_attn), and with backward dx, dslots0, grads."""
    from ocrl_amd import _lib
    L = _lib.lib()
    P, x, s0, dsl = inputs
    B, N, K, D, H, I, NH = c
    dev = lambda t: t.contiguous().cuda()
    nan = lambda *shp: torch.full(shp, float("nan"), device="cuda")
    wd = [dev(P[PRE + n]) for n in NAMES]
    gd = [nan(*t.shape) for t in wd]
    xd, s0d, dsd = dev(x), dev(s0), dev(dsl)
    slots, attn = nan(B, K, D), nan(B, N, K) if want_attn else None
    dx, ds0 = nan(B, N, C), nan(B, K, D)
    nws = L.ocrl_slot_attention_mh_ws_floats(B, N, K, D, H, I, NH)
    if NH == 1:
        assert nws == L.ocrl_slot_attention_ws_floats(B, K, D, H, I)
    ws = nan(nws)
    p = _lib.ptr
    if NH == 1:         # the single-head entry points
        _lib.check(L.ocrl_slot_attention_fwd(p(xd), p(s0d), _lib.ptrs(wd), p(slots), p(attn), B, N, K, D, H, I, p(ws), nws, None))
        if backward:
            _lib.check(L.ocrl_slot_attention_bwd(p(xd), p(dsd), p(dx), p(ds0), _lib.ptrs(gd), B, N, K, D, H, I, p(ws), nws, None))
    else:
        _lib.check(L.ocrl_slot_attention_mh_fwd(p(xd), p(s0d), _lib.ptrs(wd), p(slots), p(attn), B, N, K, D, H, I, NH, p(ws), nws, None))
        if backward:
            _lib.check(L.ocrl_slot_attention_mh_bwd(p(xd), p(dsd), p(dx), p(ds0), _lib.ptrs(gd), B, N, K, D, H, I, NH, p(ws), nws, None))
    torch.cuda.synchronize()
    out = dict(slots=slots.cpu(), attn=attn.cpu() if want_attn else None)
    if backward:
        out.update(dx=dx.cpu(), dslots0=ds0.cpu(), grads={n: t.cpu() for n, t in zip(NAMES, gd)})
    for k, v in list(out.items()) + list(out.get("grads", {}).items()):
        if torch.is_tensor(v):
            assert bool(torch.isfinite(v).all()), f"{case_id(c)}: {k} holds {int((~torch.isfinite(v)).sum())} non-finite elements (never written, or read before written)"
    return out
