"""The fused slot-attention input chain (csrc/sa_input.hip: LayerNorm + Linear/ReLU + Linear, one kernel per direction) through the C ABI
only, at row counts around the tile size ocrl_sa_input_plan reports, at 1000 rows, and at 5 tiles walked by 2 workgroups.

Per case, once: the fused pair and the unfused chain (ocrl_layernorm_fwd, ocrl_gemm_ex with bias / ReLU / mask, ocrl_layernorm_bwd; the
weight gradients split over the rows as lin_bwd_w splits them, one split per 256 rows) run on the same inputs.  Every output, gradient
and workspace buffer holds NaN before the calls and everything returned must be finite.

  1. mean, rstd, h1, x and d e4 of the fused form are bitwise the unfused chain's.
  2. Every output and the six parameter gradients meet a bar against the fp64 reference (tests/sa_input_ref.py), error measure
     max|a - b| / max|ref|: at most twice the unfused chain's error against the same reference on the same inputs -- only the order of
     the row sums changes.  Both values are logged per quantity (DESIGN.md section 3 records them).
  3. Two runs give bitwise equal gradients, and the rows of the batch are bitwise the same rows run as a batch of their own."""
import ctypes
import functools

import pytest
import torch

from tests import sa_input_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu
C = R.C


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _finite(d, tag):
    for k, v in d.items():
        assert bool(torch.isfinite(v).all()), f"{tag}: {k} holds a non-finite value"
    return d


def run_fused(inp, max_wgs=0):
    """ocrl_sa_input_fwd + _bwd on the device tensors `inp`; returns device tensors of every quantity"""
    from ocrl_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    Rn = inp["e4"].shape[0]
    pl = R.plan(Rn)
    wgs = min(pl["wgs"], max_wgs) if max_wgs else pl["wgs"]
    o = dict(mean=_nan(Rn), rstd=_nan(Rn), h1=_nan(Rn, C), x=_nan(Rn, C), de4=_nan(Rn, C), dW0=_nan(C, C), db0=_nan(C), dW2=_nan(C, C),
             db2=_nan(C), dgamma=_nan(C), dbeta=_nan(C))
    ws = _nan(wgs * pl["slab"])
    _lib.check(L.ocrl_sa_input_fwd(P(inp["e4"]), P(inp["gamma"]), P(inp["beta"]), P(inp["W0"]), P(inp["b0"]), P(inp["W2"]), P(inp["b2"]),
                                   P(o["mean"]), P(o["rstd"]), P(o["h1"]), P(o["x"]), Rn, max_wgs, None))
    _lib.check(L.ocrl_sa_input_bwd(P(inp["dx"]), P(o["h1"]), P(inp["e4"]), P(o["mean"]), P(o["rstd"]), P(inp["gamma"]), P(inp["beta"]),
                                   P(inp["W0"]), P(inp["W2"]), P(o["de4"]), P(o["dW0"]), P(o["db0"]), P(o["dW2"]), P(o["db2"]), P(o["dgamma"]),
                                   P(o["dbeta"]), Rn, max_wgs, P(ws), ws.numel(), None))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), "a slab entry of the workspace was left unwritten"
    return _finite(o, "fused")


def run_unfused(inp):
    """the chain the fused kernels replace, through the existing entry points"""
    from ocrl_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    Rn = inp["e4"].shape[0]

    def gemm(**kw):
        ws = kw.pop("ws", None)
        _lib.check(L.ocrl_gemm_ex(ctypes.byref(_lib.gemm_desc(**{k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in kw.items()})),
                                  P(ws), ws.numel() if ws is not None else 0, None))

    def lin_fwd(x, W, b, y, relu):
        gemm(A=x, B=W, C=y, M=Rn, N=C, K=C, lda=C, ldb=C, ldc=C, akc=1, bkc=1, bias=b, relu=relu)

    def lin_bwd_x(dy, W, dx, mask):
        kw = dict(mask=mask, ldmask=C) if mask is not None else {}
        gemm(A=dy, B=W, C=dx, M=Rn, N=C, K=C, lda=C, ldb=C, ldc=C, akc=1, bkc=0, **kw)

    def lin_bwd_w(dy, x, dW, db):
        splits = max(1, min(1024, Rn // 256))
        kw = dict(splitk=splits, sBias=C, ws=_nan(splits * (C * C + C))) if splits > 1 else {}
        gemm(A=dy, B=x, C=dW, M=C, N=C, K=Rn, lda=C, ldb=C, ldc=C, akc=0, bkc=0, bias_out=db, **kw)

    o = dict(mean=_nan(Rn), rstd=_nan(Rn), h1=_nan(Rn, C), x=_nan(Rn, C), de4=_nan(Rn, C), dW0=_nan(C, C), db0=_nan(C), dW2=_nan(C, C),
             db2=_nan(C), dgamma=_nan(C), dbeta=_nan(C))
    ln0, dh1, dln0, dgb = _nan(Rn, C), _nan(Rn, C), _nan(Rn, C), _nan(2 * C)
    _lib.check(L.ocrl_layernorm_fwd(P(inp["e4"]), P(inp["gamma"]), P(inp["beta"]), P(ln0), P(o["mean"]), P(o["rstd"]), Rn, C, None))
    lin_fwd(ln0, inp["W0"], inp["b0"], o["h1"], 1)
    lin_fwd(o["h1"], inp["W2"], inp["b2"], o["x"], 0)
    lin_bwd_w(inp["dx"], o["h1"], o["dW2"], o["db2"])
    lin_bwd_x(inp["dx"], inp["W2"], dh1, o["h1"])
    lin_bwd_w(dh1, ln0, o["dW0"], o["db0"])
    lin_bwd_x(dh1, inp["W0"], dln0, None)
    ws = _nan(1 << 20)
    _lib.check(L.ocrl_layernorm_bwd(P(dln0), P(inp["e4"]), P(o["mean"]), P(o["rstd"]), P(inp["gamma"]), P(o["de4"]), P(dgb), Rn, C, P(ws),
                                    ws.numel(), None))
    torch.cuda.synchronize()
    o["dgamma"], o["dbeta"] = dgb[:C].clone(), dgb[C:].clone()
    return _finite(o, "unfused")


@functools.lru_cache(maxsize=None)
def runs(name):
    """(case, device inputs, fused, unfused) of a case: computed once, shared by the tests below, never modified"""
    c = R.case(name)
    inp = {k: v.contiguous().cuda() for k, v in R.prepare(c).inputs.items()}
    return c, inp, run_fused(inp, c.max_wgs), run_unfused(inp)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_outputs_are_bitwise_the_unfused_chains(name):
    c, inp, fused, unfused = runs(name)
    for k in R.OUTPUTS:
        same = _bits(fused[k]) == _bits(unfused[k])
        n = int((~same).sum())
        assert n == 0, f"R = {c.R}: {k} differs from the unfused chain in {n} of {same.numel()} elements, first at flat index {int((~same).view(-1).nonzero()[0])}"


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_errors_against_fp64_within_twice_the_unfused_chains(name):
    c, inp, fused, unfused = runs(name)
    ref = R.prepare(c).ref
    base = {k: v[0] for k, v in R.errors(ref, unfused).items()}
    mine = {k: v[0] for k, v in R.errors(ref, fused).items()}
    log(f"[sa_input R={c.R} wgs={c.max_wgs or 'default'} seed {R.prepare(c).seed}] fused / unfused error vs fp64: " +
        " ".join(f"{k}={mine[k]:.2e}/{base[k]:.2e}" for k in R.QUANTITIES))
    assert max(base.values()) < R.TOL, base          # the yardstick itself is an fp32 result
    R.grade(ref, fused, {k: 2.0 * base[k] for k in R.QUANTITIES}, tag=f"R = {c.R}: ")


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_runs_repeat_bitwise_and_rows_do_not_depend_on_the_batch(name):
    c, inp, fused, _ = runs(name)
    again = run_fused(inp, c.max_wgs)
    for k in R.QUANTITIES:
        assert torch.equal(_bits(fused[k]), _bits(again[k])), f"R = {c.R}: {k} differs between two runs"
    # a slice of the rows as a batch of its own: other tile positions, other workgroups
    lo = c.R // 3
    hi = min(c.R, lo + 37)
    sub = dict(inp, e4=inp["e4"][lo:hi].clone(), dx=inp["dx"][lo:hi].clone())
    part = run_fused(sub, 0)
    for k in R.OUTPUTS:
        assert torch.equal(_bits(fused[k][lo:hi]), _bits(part[k])), f"R = {c.R}: rows {lo}..{hi - 1} of {k} depend on the batch they run in"
