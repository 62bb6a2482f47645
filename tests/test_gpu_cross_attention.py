"""Kernel-level tests of the decoder's cross attention to the slots in both forms, against the fp64 reference of tests/cross_attn_ref.py
(proved on the CPU by tests/test_cross_attn_ref_cpu.py): the folded form (csrc/xattn.hip) through ocrl_xattn_fwd / ocrl_xattn_bwd -- the
fold, the MFMA kernels and SlateModel's own backward of the fold, xattn_fold_bwd_launch -- at every instantiation a legal model
configuration reaches, and the plain kernels (csrc/elementwise.hip) through ocrl_cross_attn_fwd / _bwd at every (MAXK, d/h).

Every call goes through run_folded / run_plain, which are hostile on purpose (the harness of tests/test_gpu_attention_edges.py): outputs
are pre-filled with NaN (the contract is "writes", not "adds to") between sentinel guard words that must come back bit-unchanged, the
four folded operands are zeroed once by the caller as the contract says and their padding columns must still be bit-zero, and every
input is followed by NaN rows, so a read past its end that reaches a result shows up as NaN.

Tolerance: relerr (tests/gpu_util.py: max |a - b| / max |b|) < 2e-5 for every output, the kernel-level standard of
tests/test_gpu_attention_edges.TOL.  The wide-range runs compute their bar as that suite does: the same arithmetic in fp32 PyTorch on the
CPU (the folded restatement for the folded form) is measured against fp64, and the kernel may be max(2e-5, 4 x that) off (4: another
summation order, the fast exponential and the hardware reciprocal).  No output needed more than the standard: measured on the MI355X, the
worst error of any output is 1.4e-6 (dWq) over the ordinary cases and 4.7e-6 (dx; fp32 on the CPU: 3.9e-6) over the wide-range ones."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cross_attn_ref as R
from tests.gpu_util import log, relerr
from tests.test_gpu_attention_edges import GUARD, SENTINEL, TOL, Guarded, _bits

pytestmark = pytest.mark.gpu
TAIL = 72                 # NaN rows after every input (more than one 64-row tile)
_fid = lambda c: "B{}-T{}-K{}-d{}-h{}-p{}-seed{}".format(*c)
FWD_OUT = ("ck", "cv", "Ab", "AbT", "Vo", "VoT", "y", "P")
BWD_OUT = ("Pd", "dS", "dx", "dAb", "dVo", "dck", "dcv", "dWq", "dWo", "pq", "po")


def _lib():
    from ocrl_amd import _lib as M
    return M, M.lib()


def _input(t, rowlen):
    """the tensor on the device, followed by TAIL rows of NaN"""
    buf = torch.full((t.numel() + TAIL * rowlen,), float("nan"), device="cuda")
    buf[:t.numel()].copy_(t.reshape(-1))
    return buf


def _ptr(t):
    return t.data_ptr()


def _dsc32(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)


def _unpad(t, B, T, h, K):
    """[B*T, NC] in the padded column layout -> ([B,h,T,K] real slots, [B,T,h,KP-K] padding)"""
    KP = R.kp_of(K, h)
    t = t.view(B, T, h, KP)
    return t[..., :K].permute(0, 2, 1, 3).contiguous(), t[..., K:].contiguous()


def _pad_cols(t, h, K):
    """[B,h,T,K] -> [B,T,NC] in the padded column layout (zeros in the padding)"""
    B, _, T, _ = t.shape
    KP = R.kp_of(K, h)
    return torch.cat([t.permute(0, 2, 1, 3), torch.zeros(B, T, h, KP - K, dtype=t.dtype)], -1).reshape(B, T, h * KP)


def _bitzero(t):
    return bool((_bits(t) == 0).all())


# ------------------------------------------------------------------------------------------------ the folded form
def run_folded(inp, h, p=0.0, seed=0, backward=True):
    """ocrl_xattn_fwd, then ocrl_xattn_bwd, on the inputs of cross_attn_ref.make_inputs; returns every output as a CPU tensor.  Asserts the
    memory-safety side of the contract on the way."""
    M, L = _lib()
    x = inp["x"]
    B, T, d = x.shape
    K = inp["mem"].shape[1]
    KP = R.kp_of(K, h)
    NC = h * KP
    dev = {n: _input(inp[n], d) for n in ("x", "resid", "mem", "Wq", "Wk", "Wv", "Wo", "gd")}
    size = dict(ck=B * K * d, cv=B * K * d, Ab=B * NC * d, AbT=B * NC * d, Vo=B * NC * d, VoT=B * NC * d, y=B * T * d, P=B * h * T * K,
                Pd=B * T * NC, dS=B * T * NC, dx=B * T * d, dAb=B * NC * d, dVo=B * NC * d, dck=B * K * d, dcv=B * K * d, dWq=d * d, dWo=d * d,
                pq=B * d * d, po=B * d * d, cs_ws=d * d)
    g = {n: Guarded(s) for n, s in size.items()}
    for n in ("Ab", "AbT", "Vo", "VoT"):                      # the caller zeroes the folded operands once
        g[n].data.zero_()
    desc = M.XattnDesc(cs_ws_floats=d * d, B=B, T=T, K=K, d=d, h=h, p=p, seed=seed, site_p=R.SITE_P, site_o=R.SITE_O)
    for n, t in dev.items():
        setattr(desc, n, _ptr(t))
    for n, t in g.items():
        setattr(desc, n, _ptr(t.data))
    M.check(L.ocrl_xattn_fwd(ctypes.byref(desc), None))
    torch.cuda.synchronize()
    for n, t in g.items():
        assert t.guards_intact(), f"forward wrote outside {n}"
    for n in BWD_OUT + ("cs_ws",):
        assert bool(torch.isnan(g[n].data).all()), f"forward wrote {n}"
    shape = dict(ck=(B, K, d), cv=(B, K, d), Ab=(B, NC, d), AbT=(B, d, NC), Vo=(B, NC, d), VoT=(B, d, NC), y=(B, T, d), P=(B, h, T, K),
                 Pd=(B * T, NC), dS=(B * T, NC), dx=(B, T, d), dAb=(B, NC, d), dVo=(B, NC, d), dck=(B, K, d), dcv=(B, K, d), dWq=(d, d), dWo=(d, d),
                 pq=(B, d, d), po=(B, d, d))
    out = {n: g[n].data.view(shape[n]).cpu() for n in FWD_OUT}
    for n, t in out.items():
        assert torch.isfinite(t).all(), f"forward left or produced a non-finite value in {n}"
    if not backward:
        return out
    M.check(L.ocrl_xattn_bwd(ctypes.byref(desc), None))
    torch.cuda.synchronize()
    for n, t in g.items():
        assert t.guards_intact(), f"backward wrote outside {n}"
    for n in FWD_OUT:
        assert torch.equal(_bits(out[n]), _bits(g[n].data.view(shape[n]).cpu())), f"the backward changed {n}"
    for n in BWD_OUT:
        out[n] = g[n].data.view(shape[n]).cpu()
        assert torch.isfinite(out[n]).all(), f"{n} holds a non-finite value (not overwritten, or read from a tail row)"
    return out


def folded_reference(inp, h, p, seed, dtype=torch.float64, folded=False):
    """block_ref + fold_ref at the case's masks, with the operands and per-image sums of the folded form added in the padded layout"""
    B, T, d = inp["x"].shape
    K = inp["mem"].shape[1]
    kp, ko = R.keep_masks(seed, R.SITE_P, R.SITE_O, p, B, h, T, K, d) if p > 0 else (None, None)
    ref = R.block_ref(*R.weights_of(inp), h, kp, ko, p, inp["gd"], dtype=dtype, folded=folded)
    ref["Ab"], ref["Vo"] = R.fold_ref(ref["ck"], ref["cv"], inp["Wq"].to(dtype), inp["Wo"].to(dtype), h)
    ref["dVo"] = _pad_cols(ref["Pd"], h, K).transpose(1, 2) @ inp["gd"].to(dtype)
    ref["dAb"] = _pad_cols(ref["dS"], h, K).transpose(1, 2) @ inp["x"].to(dtype)
    ref["keep_p"] = kp
    return ref


def folded_errors(out, ref, inp, h, p):
    """{output: relerr} against the reference, after the exact checks: transposes, padding columns, Pd = P * keep / (1 - p) bit for bit"""
    B, T, d = inp["x"].shape
    K = inp["mem"].shape[1]
    KP = R.kp_of(K, h)
    pad = torch.ones(h, KP, dtype=torch.bool)
    pad[:, :K] = False
    pad = pad.reshape(-1)
    assert torch.equal(_bits(out["AbT"]), _bits(out["Ab"].transpose(1, 2))), "AbT is not the transpose of Ab"
    assert torch.equal(_bits(out["VoT"]), _bits(out["Vo"].transpose(1, 2))), "VoT is not the transpose of Vo"
    for n in ("Ab", "Vo"):
        assert _bitzero(out[n][:, pad]), f"a padding column of {n} was written"
    e = {n: relerr(out[n], ref[n]) for n in ("ck", "cv", "Ab", "Vo", "y", "P")}
    if "Pd" in out:
        Pd, Pd_pad = _unpad(out["Pd"], B, T, h, K)
        dS, dS_pad = _unpad(out["dS"], B, T, h, K)
        assert _bitzero(Pd_pad) and _bitzero(dS_pad), "a padding column of Pd / dS is not +0"
        want = out["P"] * torch.tensor(_dsc32(p)) if p > 0 else out["P"]
        if p > 0:
            want = torch.where(ref["keep_p"], want, torch.zeros_like(want))
        assert torch.equal(_bits(Pd), _bits(want)), "Pd is not P * keep * fp32(1 / (1 - p)) bit for bit"
        e["dS"] = relerr(dS, ref["dS"])
        for n in ("dx", "dAb", "dVo", "dck", "dcv", "dWq", "dWo"):
            e[n] = relerr(out[n], ref[n])
        e["pq"] = relerr(out["pq"].double().sum(0), ref["dWq"])
        e["po"] = relerr(out["po"].double().sum(0), ref["dWo"])
    return e


def check(tag, e, tol=TOL):
    log(f"[cross attention] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()) + f" worst={max(e.values()):.2e}")
    bad = {k: v for k, v in e.items() if not v < tol}
    assert not bad, (tag, bad)


def _folded_case(case, group):
    B, T, K, d, h, p, seed = case
    inp = R.make_inputs(B, T, K, d, h)
    out = run_folded(inp, h, p, seed)
    ref = folded_reference(inp, h, p, seed)
    if p > 0:
        assert relerr(R.block_ref(*R.weights_of(inp), h)["y"], ref["y"]) > 1e-2           # the masks move the result far beyond the tolerance
    check(f"folded {group} {_fid(case)} KP{R.kp_of(K, h)} NC{h * R.kp_of(K, h)}", folded_errors(out, ref, inp, h, p))


@pytest.mark.parametrize("case", R.FOLDED_GRID, ids=_fid)
def test_folded_every_instantiation(case):
    """d_model 64 .. 256 x every (KP, NC) a legal head count reaches, every slot class, with dropout wherever K % 4 != 0"""
    _folded_case(case, "grid")


@pytest.mark.parametrize("case", R.FOLDED_SWEEP, ids=_fid)
def test_folded_token_counts(case):
    """T = 1, one short of a tile, a tile, one more, three tiles with a ragged last, and 13 tiles in three uneven splits"""
    _folded_case(case, "tokens")


# ------------------------------------------------------------------------------------------------ the plain kernels
def run_plain(Q, Km, Vm, dO, h, p=0.0, seed=0, site=R.SITE_P, backward=True):
    M, L = _lib()
    B, T, d = Q.shape
    K = Km.shape[1]
    dev = [_input(t, d) for t in (Q, Km, Vm, dO)]
    O, P = Guarded(B * T * d), Guarded(B * h * T * K)
    M.check(L.ocrl_cross_attn_fwd(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(O.data), _ptr(P.data), B, T, K, d, h, p, seed, site, None))
    torch.cuda.synchronize()
    assert O.guards_intact() and P.guards_intact(), "forward wrote outside O / P"
    out = dict(O=O.data.view(B, T, d).cpu(), P=P.data.view(B, h, T, K).cpu())
    assert torch.isfinite(out["O"]).all() and torch.isfinite(out["P"]).all(), "forward left or produced a non-finite value"
    if not backward:
        return out
    nws = L.ocrl_cross_attn_bwd_ws_floats(B, T, K, d, h)
    assert nws == B * h * ((T + 255) // 256) * 2 * K * (d // h)
    g = dict(dQ=Guarded(B * T * d), dKm=Guarded(B * K * d), dVm=Guarded(B * K * d), ws=Guarded(nws))
    M.check(L.ocrl_cross_attn_bwd(_ptr(dev[3]), _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(P.data), _ptr(g["dQ"].data), _ptr(g["dKm"].data),
                                  _ptr(g["dVm"].data), B, T, K, d, h, p, seed, site, _ptr(g["ws"].data), nws, None))
    torch.cuda.synchronize()
    for n, t in g.items():
        assert t.guards_intact(), f"backward wrote outside {n}"
    assert O.guards_intact() and P.guards_intact()
    assert torch.equal(_bits(out["P"]), _bits(P.data.view(B, h, T, K).cpu())), "the backward changed P"
    for n, s in (("dQ", (B, T, d)), ("dKm", (B, K, d)), ("dVm", (B, K, d))):
        out[n] = g[n].data.view(s).cpu()
        assert torch.isfinite(out[n]).all(), f"{n} holds a non-finite value (not overwritten, or read from a tail row)"
    return out


def plain_inputs(inp, h):
    """the reference's q, ck, cv (rounded to fp32) as the plain kernels' Q, Km, Vm, and gd as their dO"""
    full = R.block_ref(*R.weights_of(inp), h)
    return full["q"].float(), full["ck"].float(), full["cv"].float(), inp["gd"]


def _plain_case(case, group):
    B, T, K, d, h, p, seed = case
    Q, Km, Vm, dO = plain_inputs(R.make_inputs(B, T, K, d, h), h)
    kp = R.keep_masks(seed, R.SITE_P, R.SITE_O, p, B, h, T, K, d)[0] if p > 0 else None
    out = run_plain(Q, Km, Vm, dO, h, p, seed)
    ref = R.core_ref(Q, Km, Vm, h, kp, p, dO)
    if p > 0:
        assert relerr(R.core_ref(Q, Km, Vm, h)["O"], ref["O"]) > 1e-2
    check(f"plain {group} {_fid(case)} MAXK{8 if K <= 8 else 16} dh{d // h}", {n: relerr(out[n], ref[n]) for n in ("O", "P", "dQ", "dKm", "dVm")})


@pytest.mark.parametrize("case", R.PLAIN_GRID, ids=_fid)
def test_plain_every_head_width(case):
    """cross_attn_*_kernel<8 | 16> at d/h = 4 .. 64: every load_tile stride and the partial 16-channel MFMA tile at d/h = 8 and 24"""
    _plain_case(case, "grid")


@pytest.mark.parametrize("case", R.PLAIN_LONG, ids=_fid)
def test_plain_two_query_blocks(case):
    """T = 300: two blocks of 256 queries, the second ragged; the slot-side partials of both are summed by the reduction kernel"""
    _plain_case(case, "two blocks")


@pytest.mark.parametrize("case", R.PLAIN_SWEEP, ids=_fid)
def test_plain_token_counts(case):
    _plain_case(case, "tokens")


# ------------------------------------------------------------------------------------------------ both forms, one reference
@pytest.mark.parametrize("case", R.SHARED, ids=_fid)
def test_both_forms_against_one_reference(case):
    """the plain kernels are fed the reference's q, ck, cv and d ao, so that both forms are graded against the same block_ref"""
    B, T, K, d, h, p, seed = case
    inp = R.make_inputs(B, T, K, d, h)
    ref = folded_reference(inp, h, p, seed)
    check(f"shared folded {_fid(case)}", folded_errors(run_folded(inp, h, p, seed), ref, inp, h, p))
    out = run_plain(ref["q"].float(), ref["ck"].float(), ref["cv"].float(), ref["dao"].float(), h, p, seed)
    check(f"shared plain {_fid(case)}", {a: relerr(out[a], ref[b]) for a, b in (("O", "ao"), ("P", "P"), ("dQ", "dq"), ("dKm", "dck"), ("dVm", "dcv"))})


# ------------------------------------------------------------------------------------------------ a wide soft-max range
@pytest.mark.parametrize("case", R.WIDE, ids=lambda c: "B{}-T{}-K{}-d{}-h{}".format(*c))
def test_softmax_range(case):
    """scores spanning about +-50: both forms must stay finite and as accurate as fp32 allows.  The bar is computed here (module
    docstring): max(2e-5, 4 x the error of the same arithmetic in fp32 on the CPU)."""
    B, T, K, d, h = case
    inp = R.make_wide_range_inputs(B, T, K, d, h)
    ref = folded_reference(inp, h, 0.0, 0)
    f32 = folded_reference(inp, h, 0.0, 0, dtype=torch.float32, folded=True)
    e = folded_errors(run_folded(inp, h), ref, inp, h, 0.0)
    bad = {}
    for n, err in e.items():
        src = {"pq": "dWq", "po": "dWo"}.get(n, n)
        e32 = relerr(f32[src], ref[src])
        bar = max(TOL, 4 * e32)
        log(f"[cross attention] softmax range folded B{B} T{T} K{K} d{d} h{h} {n}: kernel {err:.2e} fp32-cpu {e32:.2e} bar {bar:.2e}")
        if not err <= bar:
            bad[n] = (err, e32, bar)
    Q, Km, Vm, dO = plain_inputs(inp, h)
    pref, p32 = R.core_ref(Q, Km, Vm, h, dO=dO), R.core_ref(Q, Km, Vm, h, dO=dO, dtype=torch.float32)
    out = run_plain(Q, Km, Vm, dO, h)
    for n in ("O", "P", "dQ", "dKm", "dVm"):
        err, e32 = relerr(out[n], pref[n]), relerr(p32[n], pref[n])
        bar = max(TOL, 4 * e32)
        log(f"[cross attention] softmax range plain B{B} T{T} K{K} d{d} h{h} {n}: kernel {err:.2e} fp32-cpu {e32:.2e} bar {bar:.2e}")
        if not err <= bar:
            bad["plain." + n] = (err, e32, bar)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ contracts
def _same(a, b, names, sl=slice(None)):
    return [n for n in names if not torch.equal(_bits(a[n][sl]), _bits(b[n]))]


@pytest.mark.parametrize("case", R.REPRO, ids=_fid)
def test_bitwise_reproducible(case):
    B, T, K, d, h, p, seed = case
    inp = R.make_inputs(B, T, K, d, h)
    a, b = (run_folded(inp, h, p, seed) for _ in range(2))
    assert not _same(a, b, FWD_OUT + BWD_OUT)
    Q, Km, Vm, dO = plain_inputs(inp, h)
    a, b = (run_plain(Q, Km, Vm, dO, h, p, seed) for _ in range(2))
    assert not _same(a, b, ("O", "P", "dQ", "dKm", "dVm"))


@pytest.mark.parametrize("case", R.BATCH_INDEPENDENCE, ids=_fid)
def test_an_image_does_not_depend_on_the_batch(case):
    """image 0 of a B = 3 call equals the call on that image alone, bit for bit (the token split and the block-to-work mapping change
    with B, the arithmetic must not; element indices of image 0's dropout decisions do not depend on B).  d Wq / d Wo sum over the
    images and are left out."""
    B, T, K, d, h, p, seed = case
    inp = R.make_inputs(B, T, K, d, h)
    one = {n: (t[:1] if n in ("x", "resid", "mem", "gd") else t) for n, t in inp.items()}
    a, b = run_folded(inp, h, p, seed), run_folded(one, h, p, seed)
    per_image = tuple(n for n in FWD_OUT + BWD_OUT if n not in ("dWq", "dWo", "Pd", "dS"))
    diff = _same(a, b, per_image, slice(0, 1)) + _same(a, b, ("Pd", "dS"), slice(0, T))
    assert not diff, diff
    assert torch.equal(_bits(b["pq"][0]), _bits(b["dWq"])) and torch.equal(_bits(b["po"][0]), _bits(b["dWo"]))       # one image: the sum is the partial
    Q, Km, Vm, dO = plain_inputs(inp, h)
    a, b = run_plain(Q, Km, Vm, dO, h, p, seed), run_plain(Q[:1], Km[:1], Vm[:1], dO[:1], h, p, seed)
    diff = _same(a, b, ("O", "P", "dQ", "dKm", "dVm"), slice(0, 1))
    assert not diff, diff


@pytest.mark.parametrize("K,d,h", [c for c in R.UNSUPPORTED if c[1] <= 256 and c[0] >= 1])
def test_unsupported_shape_is_an_error_and_runs_nothing(K, d, h):
    """a shape without a folded form is refused with the reason by both entry points; no kernel runs in its place: every output keeps its
    NaN fill"""
    M, L = _lib()
    B, T = 2, 16
    inp = R.make_inputs(B, T, min(K, 16), d, h)
    NC = 16 * 16
    dev = {n: _input(inp[n], d) for n in ("x", "resid", "mem", "Wq", "Wk", "Wv", "Wo", "gd")}
    names = FWD_OUT + BWD_OUT + ("cs_ws",)
    g = {n: Guarded(max(B * T * NC, B * NC * d, B * d * d)) for n in names}
    desc = M.XattnDesc(cs_ws_floats=d * d, B=B, T=T, K=K, d=d, h=h, p=0.1, seed=R.SEED_LO, site_p=R.SITE_P, site_o=R.SITE_O)
    for n, t in dev.items():
        setattr(desc, n, _ptr(t))
    for n, t in g.items():
        setattr(desc, n, _ptr(t.data))
    for fn in (L.ocrl_xattn_fwd, L.ocrl_xattn_bwd):
        assert fn(ctypes.byref(desc), None) != 0
        msg = L.ocrl_last_error().decode()
        assert "no folded form" in msg and f"K {K}" in msg and f"heads {h}" in msg, msg
    torch.cuda.synchronize()
    for n, t in g.items():
        assert t.guards_intact() and bool(torch.isnan(t.data).all()), n


def test_plain_refuses_what_it_does_not_build():
    M, L = _lib()
    B, T, K, d, h = 1, 8, 3, 136, 2                            # d/h = 68 > 64
    t = lambda *s: _input(torch.randn(*s), d)
    Q, Km, Vm = t(B, T, d), t(B, K, d), t(B, K, d)
    O, P = Guarded(B * T * d), Guarded(B * h * T * K)
    for args in ((B, T, K, d, h), (B, T, 17, 64, 2), (B, T, 3, 60, 10)):          # d/h too wide; too many slots; d/h = 6 is no multiple of 4
        assert L.ocrl_cross_attn_fwd(_ptr(Q), _ptr(Km), _ptr(Vm), _ptr(O.data), _ptr(P.data), *args, 0.0, 0, 0, None) != 0
        assert "unsupported" in L.ocrl_last_error().decode()
    torch.cuda.synchronize()
    assert O.guards_intact() and P.guards_intact() and bool(torch.isnan(O.data).all()) and bool(torch.isnan(P.data).all())
    assert GUARD % 4 == 0 and SENTINEL < 0
