"""The SLATE token-path and helper kernels (elementwise.hip) one by one through include/ocrl_hip_slate_kernels.h against the fp64 references
of tests/token_path_ref.py, at the shapes tests/test_gpu_slate.py does not reach: several histogram chunks and summation units of the
dictionary gradient with segments on, across and inside unit boundaries, every instantiation of the Gumbel soft-max, wholly empty
vocabulary segments, more than 256 cached keys, both column-sum kernels with idle lanes, padding, accumulate, scale and a shrunk workspace,
the second trip of the reconstruction loss's grid-stride loop, and row counts that leave blocks partly empty.

Bar: TOL = 2e-5 of the reference tensor's maximum per output tensor; a reference that is exactly zero requires exact zeros.  Pure data
movement, dropout against its mask and the run-to-run check of the dictionary gradient are bit-exact.  The soft-max family has
max(TOL, 4 x floor), floor = what the reference's own formulas lose when torch evaluates them in fp32 on the CPU (FLOORS below, held to its
measurement by tests/test_token_path_ref_cpu.py).  Tokens allow no mismatch: the inputs' top-two gaps are at least 100 x the fp32 error of
the compared score (asserted on the CPU), and in the tie cases the lower index wins by definition.  Outputs a kernel must write in full are
pre-filled with NaN and must come back finite; memory it must not touch or read holds a sentinel.

Worst measured error per entry on an MI355X, relative to the reference's maximum (every token, layout and dropout comparison: 0 mismatches):
gumbel_softmax z 1.8e-6 (well, R 5, V 2048, tau 0.1), row sums 1.6e-7, zst 1.4e-8; softmax_bwd_rows 5.0e-8; softmax_stat_combine lse
5.3e-8, cross-entropy 1.5e-7; exp_rows 3.3e-8; rowdot_bias64 1.3e-7; embed_fwd 1.2e-7; embed_bwd ddict 2.7e-7, g 9.5e-8; embed_step
4.7e-8; colsum 2.3e-7 (R 1031, F 192); mse loss 5.2e-8, drecon 6.0e-8; posmap 8.0e-8; slot_init 9.3e-8, dmu 1.7e-7, dlogsig 2.1e-7;
decode_attn 5.8e-7 (T 300, t 256).  Dropout keep rate at n = 2^20: +0.62 sigma; drawn slot noise at n = 2^16: mean +1.2e-3, var - 1 +7.8e-3
(bounds 1.95e-2 and 2.76e-2)."""
import ctypes
import math

import pytest
import torch

from tests import token_path_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu
TOL = 2e-5
NAN = float("nan")
SENTINEL = -777.0

# (key of token_path_ref.floor_cases(), output) -> what torch's fp32 evaluation of the reference's formula loses against fp64, relative to the
# output's maximum; only the entries above TOL / 4 are listed, every other output of the family holds plain TOL.  Measured with torch 2.x on
# an x86-64 CPU; tests/test_token_path_ref_cpu.py holds each entry within a factor 1.5 of its measurement.  The table is empty: on the input
# sets used here the largest floor is the Gumbel soft sample's at tau = 0.1 (about 2e-6), below TOL / 4, so every bar of the family is TOL.
FLOORS = {
}


def bar_of(key, output):
    return max(TOL, 4 * FLOORS.get((key, output), 0.0))


# ------------------------------------------------------------------------------------------------------------------- helpers
def lib():
    from ocrl_amd import _lib
    return _lib.lib()


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def P(t):
    """device pointer of a tensor (None: null); the tensor is held until the test ends, so that a temporary's memory is not handed to the
    next allocation while a launch that reads it is still queued"""
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def stream():
    from ocrl_amd import _lib
    return _lib.stream()


def ok(rc):
    from ocrl_amd import _lib
    _lib.check(rc)


def refused(rc, *words):
    msg = lib().ocrl_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def dev(t):
    return t.detach().float().contiguous().cuda()


def idev(t):
    return t.detach().int().contiguous().cuda()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def sentinels(*shape):
    return torch.full(shape, SENTINEL, device="cuda")


def padded(t, ld, fill=SENTINEL):
    """[R, F] -> a device [R, ld] tensor whose columns beyond F hold the sentinel"""
    out = torch.full((t.shape[0], ld), fill, device="cuda")
    out[:, :t.shape[1]] = t.float().cuda()
    return out


def err(got, ref):
    """max |got - ref| / max |ref| against fp64; an exactly zero reference requires exact zeros (inf otherwise)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = ref.abs().max().item() if ref.numel() else 0.0
    d = (got - ref).abs().max().item() if ref.numel() else 0.0
    if den == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / den


def grade(tag, rows):
    """rows: (name, got, ref, bar); logs every error, then asserts finiteness and the bars"""
    out = []
    for name, got, ref, bar in rows:
        assert bool(torch.isfinite(got).all()), f"{tag}: {name} is not finite"
        out.append((name, err(got, ref), bar))
    log(f"[tpk {tag}] " + " ".join(f"{n}={e:.1e}" + (f"(bar {b:.1e})" if b != TOL else "") for n, e, b in out))
    bad = [(n, e, b) for n, e, b in out if not e <= b]
    assert not bad, (tag, bad)


def exact(tag, got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu().to(got.dtype)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    n = int((got != ref).sum())
    log(f"[tpk {tag}] mismatches={n}")
    assert n == 0 and bool(torch.isfinite(got.double()).all()), (tag, n)


def sync():
    torch.cuda.synchronize()


def keep_mask(site, n, p, seed):
    m = nans(n)
    ok(lib().ocrl_tp_dropout_mask(P(m), site, n, p, seed, stream()))
    sync()
    assert bool(((m == 0) | (m == 1)).all())
    return m


# ------------------------------------------------------------------------------------------------------------------- Gumbel soft-max
def run_gumbel(raw, e1, e2, tau, with_zst):
    Rr, V = raw.shape
    z, zst, tok = nans(Rr, V), (nans(Rr, V) if with_zst else None), torch.full((Rr,), -1, dtype=torch.int32, device="cuda")
    ok(lib().ocrl_tp_gumbel_softmax(P(dev(raw)), P(dev(e1)), P(dev(e2)), P(z), P(tok), P(zst), Rr, V, tau, 0, stream()))
    sync()
    return z, zst, tok


@pytest.mark.parametrize("with_zst", [True, False], ids=["zst", "soft"])
@pytest.mark.parametrize("kind,Rr,V,tau", R.GUMBEL_CASES, ids=[f"{k}-R{r}-V{v}-tau{t}" for k, r, v, t in R.GUMBEL_CASES])
def test_gumbel_softmax(kind, Rr, V, tau, with_zst):
    raw, e1, e2 = R.gumbel_inputs(kind, Rr, V)
    ref = R.gumbel_softmax(raw, e1, e2, tau)
    z, zst, tok = run_gumbel(raw, e1, e2, tau, with_zst)
    key = ("gumbel", kind, Rr, V, tau)
    rows = [("z", z, ref["z"], bar_of(key, "z")), ("rowsum", z.double().sum(-1), torch.ones(Rr, dtype=torch.float64), TOL)]
    if with_zst:
        rows.append(("zst", zst, ref["zst"], bar_of(key, "zst")))
    grade(f"gumbel {kind} R{Rr} V{V} tau{tau}", rows)
    exact(f"gumbel tokens {kind} R{Rr} V{V} tau{tau}", tok.long(), ref["tokens"])
    if with_zst:
        exact(f"gumbel zst one-hot {kind} R{Rr} V{V} tau{tau}", zst.round(), R.onehot(z.argmax(-1).cpu(), V))
        exact(f"gumbel zst argmax {kind} R{Rr} V{V} tau{tau}", zst.argmax(-1), ref["s1"].argmax(-1))


@pytest.mark.parametrize("V", [768, 4096])
@pytest.mark.parametrize("where", list(R.TIE_PAIRS))
def test_gumbel_softmax_ties_go_to_the_lower_index(where, V):
    raw, e1, e2 = R.gumbel_tie_inputs(where, V)
    ref = R.gumbel_softmax(raw, e1, e2, 1.0)
    z, zst, tok = run_gumbel(raw, e1, e2, 1.0, True)
    low = torch.full((3,), R.TIE_PAIRS[where][0], dtype=torch.int64)
    assert torch.equal(ref["tokens"], low) and torch.equal(ref["s1"].argmax(-1), low)
    grade(f"gumbel tie {where} V{V}", [("z", z, ref["z"], TOL)])
    exact(f"gumbel tie tokens {where} V{V}", tok.long(), low)
    exact(f"gumbel tie zst {where} V{V}", zst.round(), R.onehot(low, V))


@pytest.mark.parametrize("Rr,V", R.SOFTMAX_BWD_CASES)
def test_softmax_bwd_rows(Rr, V):
    z, d = R.softmax_bwd_inputs(Rr, V)
    dd = dev(d)
    ok(lib().ocrl_tp_softmax_bwd_rows(P(dev(z)), P(dd), Rr, V, R.BWD_SCALE, stream()))
    sync()
    grade(f"softmax_bwd R{Rr} V{V}", [("d", dd, R.softmax_bwd_rows(z, d, R.BWD_SCALE), bar_of(("softmax_bwd", Rr, V), "d"))])


# ------------------------------------------------------------------------------------------------------------------- fused-head statistics
@pytest.mark.parametrize("nseg,Rr", R.STAT_CASES)
def test_softmax_stat_combine(nseg, Rr):
    i = R.stat_inputs(nseg, Rr)
    V, ldp = i["V"], i["V"] + 8
    lse_ref, ce_ref = R.stat_combine(i["scores"], i["pred"], i["tok"], R.CE_SCALE)
    stat, hstat, hidx = dev(i["stat"]), dev(i["hstat"]), idev(i["hidx"])
    if nseg == 6:
        assert bool((i["stat"][:, 5, 0] == -math.inf).all()) and bool((i["stat"][:, 5, 1] == 0).all())       # the wholly empty segment
    nws = (Rr + 15) // 16
    key = ("stat", nseg, Rr)
    # lse alone: nothing else is touched
    lse, tok_out, out, ws = nans(Rr), torch.full((Rr,), -5, dtype=torch.int32, device="cuda"), sentinels(1), sentinels(nws)
    ok(lib().ocrl_tp_softmax_stat_combine(P(stat), nseg, Rr, P(lse), None, None, P(tok_out), None, 0, 0, None, P(out), 1.0, P(ws), nws, stream()))
    sync()
    grade(f"stat lse nseg{nseg} R{Rr}", [("lse", lse, lse_ref, bar_of(key, "lse"))])
    assert bool((tok_out == -5).all()) and float(out) == SENTINEL and bool((ws == SENTINEL).all())
    # everything
    lse, out, ws = nans(Rr), nans(1), nans(nws)
    pred = padded(i["pred"], ldp)
    ok(lib().ocrl_tp_softmax_stat_combine(P(stat), nseg, Rr, P(lse), P(hstat), P(hidx), P(tok_out), P(pred), ldp, V, P(idev(i["tok"])), P(out),
                                          R.CE_SCALE, P(ws), nws, stream()))
    sync()
    grade(f"stat all nseg{nseg} R{Rr}", [("lse", lse, lse_ref, bar_of(key, "lse")), ("ce", out, ce_ref, bar_of(key, "ce"))])
    exact(f"stat tokens nseg{nseg} R{Rr}", tok_out.long(), i["hard"].argmax(-1))


@pytest.mark.parametrize("nseg,Rr", [(4, 17), (6, 16), (64, 33)])
def test_softmax_stat_combine_ties_go_to_the_lower_column(nseg, Rr):
    hm, hidx, want = R.stat_tie(nseg, Rr)
    stat = dev(R.stat_inputs(nseg, Rr)["stat"])
    lse, tok = nans(Rr), torch.full((Rr,), -5, dtype=torch.int32, device="cuda")
    ok(lib().ocrl_tp_softmax_stat_combine(P(stat), nseg, Rr, P(lse), P(dev(hm)), P(idev(hidx)), P(tok), None, 0, 0, None, None, 1.0, None, 0, stream()))
    sync()
    exact(f"stat tie nseg{nseg} R{Rr}", tok.long(), want)


@pytest.mark.parametrize("Rr,V", R.EXP_ROWS_CASES)
def test_exp_rows(Rr, V):
    y, lse = R.exp_rows_inputs(Rr, V)
    z = nans(Rr, V)
    ok(lib().ocrl_tp_exp_rows(P(dev(y)), P(dev(lse)), P(z), Rr, V, stream()))
    sync()
    grade(f"exp_rows R{Rr} V{V}", [("z", z, R.exp_rows(y, lse), bar_of(("exp_rows", Rr, V), "z"))])


@pytest.mark.parametrize("Rr", [1, 15, 16, 17])
def test_rowdot_bias64(Rr):
    g = R._gen(21, Rr)
    gg, act, bias = torch.randn(Rr, 64, generator=g), torch.randn(Rr, 64, generator=g), torch.randn(64, generator=g)
    out = torch.cat((nans(Rr), sentinels(3)))
    ok(lib().ocrl_tp_rowdot_bias64(P(dev(gg)), P(dev(act)), P(dev(bias)), Rr, P(out), stream()))
    sync()
    grade(f"rowdot R{Rr}", [("out", out[:Rr], R.rowdot_bias64(gg, act, bias), TOL)])
    assert bool((out[Rr:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------- embedding
def run_embed_fwd(tok, dic, bos, pe, p, seed):
    B, T = tok.shape
    d = dic.shape[1]
    out = nans(B, T, d)
    ok(lib().ocrl_tp_embed_fwd(P(idev(tok)), P(dev(dic)), P(dev(bos)), P(dev(pe)), P(out), B, T, d, p, seed, stream()))
    sync()
    return out


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("V", [8, 4096])
@pytest.mark.parametrize("B,T,d", [(1, 1, 4), (2, 16, 64), (3, 37, 192)])
def test_embed_fwd(B, T, d, V, p):
    tok, dic, bos, pe, _ = R.embed_inputs(B, T, V, d)
    ref = R.embed_fwd(tok, dic, bos, pe)
    out = run_embed_fwd(tok, dic, bos, pe, p, 77)
    tag = f"embed_fwd B{B} T{T} d{d} V{V} p{p}"
    assert torch.equal(ref[:, 0], (bos.double() + pe.double()[0]).expand(B, d))                # row 0 is BOS
    if p > 0:
        m = keep_mask(1, B * (T + 1) * d, p, 77).view(B, T + 1, d)[:, :T].cpu().double()
        assert bool((out.cpu()[m == 0] == 0).all()), tag                                         # dropped elements are exact zeros
        ref = ref * m / (1.0 - R.f32(p))
        assert B * T * d < 100 or 0 < int((m == 0).sum()) < m.numel() // 4
    grade(tag, [("out", out, ref, TOL)])
    other = tok.clone()
    other[:, T - 1] = (other[:, T - 1] + 1) % V                                                # token (b, T - 1) is never used
    assert torch.equal(out, run_embed_fwd(other, dic, bos, pe, p, 77))


EMBED_BWD_CASES = [(2, 16, 8, 64, "random"), (5, 128, 8, 64, "const3"), (4, 129, 8, 64, "image"), (3, 100, 3, 64, "random"),
                   (3, 100, 4096, 192, "random"), (2, 16, 8, 4, "random"), (2, 16, 8, 1024, "random")]


def run_embed_bwd(g, tok, V, p, seed):
    B, T, d = g.shape
    n = lib().ocrl_tp_embed_bwd_ws_floats(B * T, V, d)
    assert n > 0
    gd, ddict, ws = dev(g), nans(V, d), nans(n)
    ok(lib().ocrl_tp_embed_bwd(P(gd), P(idev(tok)), P(ddict), B, T, V, d, p, seed, P(ws), n, stream()))
    sync()
    return gd, ddict


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,V,d,tokens", EMBED_BWD_CASES)
def test_embed_bwd(B, T, V, d, tokens, p):
    tok, _, _, _, g = R.embed_inputs(B, T, V, d, tokens)
    tag = f"embed_bwd B{B} T{T} V{V} d{d} {tokens} p{p}"
    gd, ddict = run_embed_bwd(g, tok, V, p, 5)
    gref = g.double()
    if p > 0:
        m = keep_mask(1, B * (T + 1) * d, p, 5).view(B, T + 1, d)[:, :T].cpu().double()
        gref = gref * m / (1.0 - R.f32(p))
        grade(tag + " g", [("g", gd, gref, TOL)])
        assert bool((gd.cpu()[m == 0] == 0).all())
        ref = R.embed_bwd(gd.cpu(), tok, V)                       # ddict is computed from the g the kernel left
    else:
        exact(tag + " g", gd, g)
        ref = R.embed_bwd(g, tok, V)
    grade(tag, [("ddict", ddict, ref, TOL)])
    absent = torch.ones(V, dtype=torch.bool)
    absent[tok[:, :T - 1].reshape(-1).long()] = False
    assert bool((ddict.cpu()[absent] == 0).all()) and (V < 4096 or int(absent.sum()) > V // 2)
    again = run_embed_bwd(g, tok, V, p, 5)[1]
    assert torch.equal(ddict, again), tag + ": two runs differ"


@pytest.mark.parametrize("t", [0, 36])
def test_embed_step(t):
    B, T, V, d = 3, 37, 4096, 192
    tok, dic, bos, pe, _ = R.embed_inputs(B, T, V, d)
    out = torch.cat((nans(B * d), sentinels(8)))
    ok(lib().ocrl_tp_embed_step(P(idev(tok)), P(dev(dic)), P(dev(bos)), P(dev(pe)), P(out), B, T, d, t, stream()))
    sync()
    grade(f"embed_step t{t}", [("out", out[:B * d].view(B, d), R.embed_step(tok, dic, bos, pe, t), TOL)])
    assert bool((out[B * d:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("n", [4, 4100])
def test_dropout_apply_is_the_mask(n):
    p, seed, site = 0.1, 1234, 24
    x = torch.randn(n, generator=R._gen(22, n))
    y = torch.cat((nans(n), sentinels(4)))
    ok(lib().ocrl_tp_dropout_apply(P(dev(x)), P(y), n, p, seed, site, stream()))
    sync()
    m = keep_mask(site, n, p, seed)
    sc = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    exact(f"dropout n{n}", y[:n], torch.where(m.cpu() > 0, x * sc, torch.zeros(n)))
    assert bool((y[n:] == SENTINEL).all())
    if n > 4:
        assert not torch.equal(m, keep_mask(site + 1, n, p, seed)) and not torch.equal(m, keep_mask(site, n, p, seed + 1))
        assert 0 < int((m == 0).sum()) < n // 4


def test_dropout_mask_rate():
    n, p = 1 << 20, 0.1
    m = keep_mask(24, n, p, 99)
    mean, sigma = float(m.double().mean()), math.sqrt(p * (1 - p) / n)
    log(f"[tpk dropout rate] mean={mean:.6f} ({(mean - (1 - p)) / sigma:+.2f} sigma)")
    assert abs(mean - (1 - p)) < 5 * sigma


# ------------------------------------------------------------------------------------------------------------------- column sums
COLSUM_GENERIC = [(1, 1, 1, 0), (5, 3, 3, 0), (63, 100, 104, 0), (1000, 64, 64, 0), (70, 1100, 1100, 0), (2048, 64, 64, 1)]
COLSUM_FAST = [(1024, 4, 4, 0), (1031, 192, 200, 0), (1500, 576, 576, 0), (2050, 1024, 1024, 0), (40000, 64, 64, 0)]
COLSUM_WS = 2048 * 1024


def run_colsum(Rr, F_, ld, offset, accumulate, scale, ws_floats):
    g = R._gen(23, Rr, F_, ld)
    X, out0 = torch.randn(Rr, F_, generator=g), torch.randn(F_, generator=g)
    buf = torch.full((Rr * ld + 4,), SENTINEL, device="cuda")
    Xd = buf[offset:offset + Rr * ld].view(Rr, ld)
    Xd[:, :F_] = X.cuda()
    out = torch.cat((dev(out0) if accumulate else nans(F_), sentinels(4)))
    ws = nans(ws_floats)
    rc = lib().ocrl_tp_colsum(ctypes.c_void_p(Xd.data_ptr()), ld, P(out), Rr, F_, accumulate, scale, P(ws), ws_floats, stream())
    sync()
    _KEEP.append(buf)
    return rc, out, R.colsum(X, F_, out0, accumulate, scale)


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("Rr,F_,ld,offset", COLSUM_GENERIC + COLSUM_FAST + [(2048, 64, 64, 0)],
                         ids=[f"R{r}-F{f}-ld{l}-off{o}" for r, f, l, o in COLSUM_GENERIC + COLSUM_FAST] + ["small-ws"])
def test_colsum(Rr, F_, ld, offset, accumulate, scale, request):
    small = "small-ws" in request.node.name
    rc, out, ref = run_colsum(Rr, F_, ld, offset, accumulate, scale, 20 * 64 if small else COLSUM_WS)
    ok(rc)
    grade(f"colsum R{Rr} F{F_} ld{ld} off{offset} acc{accumulate} scale{scale}{' small-ws' if small else ''}", [("out", out[:F_], ref, TOL)])
    assert bool((out[F_:] == SENTINEL).all())


def test_colsum_refuses_a_workspace_below_its_smallest_chunking():
    rc, out, _ = run_colsum(2048, 64, 64, 0, 1, 1.0, 15 * 64)
    refused(rc, "workspace too small")
    g = R._gen(23, 2048, 64, 64)
    torch.randn(2048, 64, generator=g)
    assert torch.equal(out[:64].cpu(), torch.randn(64, generator=g)) and bool((out[64:] == SENTINEL).all())         # untouched


# ------------------------------------------------------------------------------------------------------------------- reconstruction loss
@pytest.mark.parametrize("with_d", [True, False], ids=["drecon", "loss"])
@pytest.mark.parametrize("B,C,H,W", [(1, 3, 4, 4), (2, 1, 8, 8), (3, 3, 24, 24), (2, 4, 16, 16), (17, 3, 128, 128)])
def test_mse(B, C, H, W, with_d):
    g = R._gen(24, B, C, H, W)
    obs, recon = torch.rand(B, C, H, W, generator=g), torch.rand(B, H, W, 4, generator=g)
    recon[..., C:] = SENTINEL                                     # padding channels must not be read into the loss
    loss_ref, d_ref = R.mse(obs, recon)
    out, ws, drecon = nans(1), nans(1024), (nans(B, H, W, 4) if with_d else None)
    ok(lib().ocrl_tp_mse(P(dev(obs)), P(dev(recon)), P(drecon), P(out), B, C, H, W, P(ws), 1024, stream()))
    sync()
    rows = [("loss", out, loss_ref, TOL)]
    if with_d:
        rows.append(("drecon", drecon, d_ref, TOL))
        assert bool((drecon[..., C:] == 0).all())
    grade(f"mse B{B} C{C} H{H} W{W}", rows)


# ------------------------------------------------------------------------------------------------------------------- layout kernels
@pytest.mark.parametrize("B,h,w,Cout", [(1, 1, 1, 1), (2, 3, 5, 3), (2, 8, 8, 64)])
def test_pixel_shuffle(B, h, w, Cout):
    g = R._gen(25, B, h, w, Cout)
    x, y = torch.randn(B, h, w, 4 * Cout, generator=g), torch.randn(B, 2 * h, 2 * w, Cout, generator=g)
    mask = torch.randn(B, h, w, 4 * Cout, generator=g)
    mask[torch.rand(B, h, w, 4 * Cout, generator=g) < 0.3] = 0.0
    tag = f"pixel_shuffle B{B} h{h} w{w} C{Cout}"
    out = nans(B, 2 * h, 2 * w, Cout)
    ok(lib().ocrl_tp_pixel_shuffle(P(dev(x)), P(out), B, h, w, Cout, 1, None, stream()))
    sync()
    exact(tag + " fwd", out, R.pixel_shuffle(x))
    for m in (None, mask):
        back = nans(B, h, w, 4 * Cout)
        ok(lib().ocrl_tp_pixel_shuffle(P(dev(y)), P(back), B, h, w, Cout, 0, P(None if m is None else dev(m)), stream()))
        sync()
        exact(tag + (" inv" if m is None else " inv mask"), back, R.pixel_unshuffle(y, m))


@pytest.mark.parametrize("C", [1, 3, 8])
def test_nchw_to_nhwc8(C):
    B, H, W = 2, 5, 7
    x = torch.randn(B, C, H, W, generator=R._gen(26, C))
    out = nans(B, H, W, 8)
    ok(lib().ocrl_tp_nchw_to_nhwc8(P(dev(x)), P(out), B, C, H, W, stream()))
    sync()
    exact(f"nchw_to_nhwc8 C{C}", out, R.nchw_to_nhwc8(x))


@pytest.mark.parametrize("B,C,S", [(2, 3, 8), (1, 1, 4)])
def test_patchify4(B, C, S):
    x = torch.randn(B, C, S, S, generator=R._gen(27, B, C, S))
    out = nans(B * (S // 4) ** 2, C * 16)
    ok(lib().ocrl_tp_patchify4(P(dev(x)), P(out), B, C, S, stream()))
    sync()
    exact(f"patchify4 B{B} C{C} S{S}", out, R.patchify4(x))


def test_pad_cols_both_ways():
    Rr, C, ld = 5, 19, 24
    x = torch.randn(Rr, C, generator=R._gen(28))
    wide = sentinels(Rr, ld + 2)                                 # pad: [R, C] -> the first ld columns of rows of stride ld + 2
    ok(lib().ocrl_tp_pad_cols(P(dev(x)), C, P(wide), ld + 2, Rr, C, ld, stream()))
    sync()
    exact("pad_cols pad", wide[:, :ld], R.pad_cols(x, C, ld))
    assert bool((wide[:, ld:] == SENTINEL).all())
    src, back = padded(x, ld), sentinels(Rr, C + 1)              # and back: the padding of the source is not read
    ok(lib().ocrl_tp_pad_cols(P(src), ld, P(back), C + 1, Rr, C, C, stream()))
    sync()
    exact("pad_cols back", back[:, :C], x)
    assert bool((back[:, C:] == SENTINEL).all())


@pytest.mark.parametrize("C,ldc", [(3, 76), (3, 80), (8, 200)])
def test_im2col5(C, ldc):
    B, H, W = 2, 6, 9
    x8 = torch.randn(B, H, W, 8, generator=R._gen(29, C, ldc))
    xd = dev(x8)
    xd[..., C:] = SENTINEL                                        # channels beyond C are not read
    col = nans(B * H * W, ldc)
    ok(lib().ocrl_tp_im2col5(P(xd), P(col), B, H, W, C, ldc, stream()))
    sync()
    ref = R.im2col5(x8, C, ldc)
    exact(f"im2col5 C{C} ldc{ldc}", col, ref)
    assert bool((ref.view(B, H, W, ldc)[:, 0, :, :5 * C] == 0).all()) and bool((ref.view(B, H, W, ldc)[:, :, W - 1, 4 * C:5 * C] == 0).all())       # edge taps


def test_unpack5():
    C, ldc = 3, 76
    dWp = torch.randn(64, 75, generator=R._gen(30))
    out = nans(64, C, 5, 5)
    ok(lib().ocrl_tp_unpack5(P(padded(dWp, ldc)), P(out), C, ldc, stream()))
    sync()
    exact("unpack5", out, R.unpack5(dWp, C))


@pytest.mark.parametrize("S", [1, 2, 16])
def test_posmap_and_posgrid(S):
    C = 64
    g = R._gen(31, S)
    grid = torch.cat((nans(S * S * 4), sentinels(4)))
    ok(lib().ocrl_tp_posgrid(P(grid), S, stream()))
    sync()
    exact(f"posgrid S{S}", grid[:S * S * 4].view(S * S, 4), R.posgrid(S))
    assert bool((grid[S * S * 4:] == SENTINEL).all())
    # signed powers of two: every product is exact, so the sum does not depend on whether the compiler contracts it
    W2 = torch.ldexp(torch.ones(C, 4), torch.randint(-3, 4, (C, 4), generator=g)) * (torch.randint(0, 2, (C, 4), generator=g) * 2 - 1)
    b2 = torch.randint(-8, 9, (C,), generator=g).float() / 4
    Wn, bn = torch.randn(C, 4, generator=g), torch.randn(C, generator=g)
    for name, Wp, bp in (("dyadic", W2, b2), ("normal", Wn, bn)):
        out = torch.cat((nans(S * S * C), sentinels(4)))
        ok(lib().ocrl_tp_posmap(P(dev(Wp)), P(dev(bp)), P(out), S, C, stream()))
        sync()
        if name == "dyadic":
            exact(f"posmap S{S} dyadic", out[:S * S * C].view(S, S, C), R.posmap(Wp, bp, S, dtype=torch.float32))
        grade(f"posmap S{S} {name}", [("out", out[:S * S * C].view(S, S, C), R.posmap(Wp, bp, S), TOL)])
        assert bool((out[S * S * C:] == SENTINEL).all())


def test_onehot():
    rows, V = 5, 256
    tok = torch.tensor([0, 255, 17, 128, 64], dtype=torch.int32)
    z = nans(rows, V)
    ok(lib().ocrl_tp_onehot(P(idev(tok)), P(z), rows, V, stream()))
    sync()
    exact("onehot", z, R.onehot(tok, V))


# ------------------------------------------------------------------------------------------------------------------- slot initialisation
SLOT_CASES = [(1, 1), (17, 64), (33, 100), (12, 192)]


def slot_inputs(BK, D):
    g = R._gen(32, BK, D)
    return torch.randn(D, generator=g), torch.randn(D, generator=g) * 0.5, torch.randn(BK, D, generator=g), torch.randn(BK, D, generator=g)


def run_slot_bwd(d, ls, noise, seed):
    BK, D = d.shape
    dmu, dls = torch.cat((nans(D), sentinels(4))), torch.cat((nans(D), sentinels(4)))
    ok(lib().ocrl_tp_slot_init_bwd(P(dev(d)), P(dev(ls)), P(None if noise is None else dev(noise)), P(dmu), P(dls), BK, D, seed, stream()))
    sync()
    assert bool((dmu[D:] == SENTINEL).all()) and bool((dls[D:] == SENTINEL).all())
    return dmu[:D], dls[:D]


@pytest.mark.parametrize("BK,D", SLOT_CASES)
def test_slot_init_with_given_noise(BK, D):
    mu, ls, eps, d = slot_inputs(BK, D)
    s0 = nans(BK, D)
    ok(lib().ocrl_tp_slot_init(P(dev(mu)), P(dev(ls)), P(dev(eps)), P(s0), BK, D, 0, stream()))
    sync()
    dmu, dls = run_slot_bwd(d, ls, eps, 0)
    rm, rl = R.slot_init_bwd(d, ls, eps)
    grade(f"slot_init BK{BK} D{D}", [("slots0", s0, R.slot_init(mu, ls, eps), TOL), ("dmu", dmu, rm, TOL), ("dlogsig", dls, rl, TOL)])


@pytest.mark.parametrize("BK,D", SLOT_CASES + [(1024, 64)])
def test_slot_init_draws_the_same_noise_both_ways(BK, D):
    mu, ls, _, d = slot_inputs(BK, D)
    s0 = nans(BK, D)
    ok(lib().ocrl_tp_slot_init(P(dev(mu)), P(dev(ls)), None, P(s0), BK, D, 4242, stream()))
    sync()
    assert bool(torch.isfinite(s0).all())
    eps = (s0.cpu().double() - mu.double()) / ls.double().exp()
    dmu, dls = run_slot_bwd(d, ls, None, 4242)
    rm, rl = R.slot_init_bwd(d, ls, eps)
    grade(f"slot_init drawn BK{BK} D{D}", [("dmu", dmu, rm, TOL), ("dlogsig", dls, rl, TOL)])
    n = BK * D
    if n >= 1 << 16:
        mean, var = float(eps.mean()), float(eps.var())
        log(f"[tpk slot_init drawn BK{BK} D{D}] mean={mean:+.2e} var-1={var - 1:+.2e} (5 sigma: {5 / math.sqrt(n):.2e}, {5 * math.sqrt(2 / n):.2e})")
        assert abs(mean) < 5 / math.sqrt(n) and abs(var - 1) < 5 * math.sqrt(2 / n)
    elif n > 1:
        other = nans(BK, D)
        ok(lib().ocrl_tp_slot_init(P(dev(mu)), P(dev(ls)), None, P(other), BK, D, 4243, stream()))
        sync()
        assert not torch.equal(other, s0)


# ------------------------------------------------------------------------------------------------------------------- greedy decode
@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("t", [0, 4])
@pytest.mark.parametrize("V", [100, 256, 4096])
def test_argmax_pos(V, t, dense):
    B, T = 3, 5
    g = R._gen(33, V, t, dense)
    pred = torch.randn(B if dense else B * T, V, generator=g)
    row = 1 if dense else 1 * T + t                              # image 1: a tie between two columns of different waves; the first wins
    pred[row, 70], pred[row, 7] = 9.0, 9.0
    if V > 256:
        pred[(2 if dense else 2 * T + t), [300, 300 + 256]] = 9.0                                # image 2: a tie inside one thread's columns
    ref = R.argmax_pos(pred, B, T, t, dense)
    assert int(ref[1]) == 7 and (V <= 256 or int(ref[2]) == 300)
    tok = torch.full((B * T + 2,), int(SENTINEL), dtype=torch.int32, device="cuda")
    ok(lib().ocrl_tp_argmax_pos(P(dev(pred)), P(tok), B, T, V, t, dense, stream()))
    sync()
    exact(f"argmax_pos V{V} t{t} dense{dense}", tok[:B * T].view(B, T)[:, t].long(), ref)
    others = torch.ones(B * T + 2, dtype=torch.bool)
    others[torch.arange(B) * T + t] = False
    assert bool((tok.cpu()[others] == int(SENTINEL)).all())


@pytest.mark.parametrize("case,t", [pytest.param(c, t, id=f"B{c[0]}-T{c[1]}-d{c[2]}-h{c[3]}-ld{c[4]}-t{t}") for c in R.DECODE_CASES for t in R.decode_ts(c)])
def test_decode_attn(case, t):
    B, T, d, h, ld = case
    qkv = R.decode_inputs(case)
    ref = R.decode_attn(qkv, t, d, h)
    x = dev(qkv)
    x[:, t + 1:] = NAN                                            # rows beyond t are not read
    x[:, :, 3 * d:] = NAN                                         # nor the padding columns
    out = torch.cat((nans(B * d), sentinels(4)))
    ok(lib().ocrl_tp_decode_attn(P(x), P(out), B, T, t, d, h, ld, stream()))
    sync()
    grade(f"decode_attn {case} t{t}", [("out", out[:B * d].view(B, d), ref, bar_of(("decode", case, t), "out"))])
    assert bool((out[B * d:] == SENTINEL).all())
