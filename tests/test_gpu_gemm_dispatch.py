"""Every instantiation of the fp32 MFMA GEMM (csrc/gemm_impl.h) against a float64 reference on the CPU, through ocrl_gemm_ex.

The dispatcher picks one gemm_kernel<BM, BN, AKC, BKC, SB, XF, EPI> per call; force_tile / force_sb select one directly, so each tile
shape, buffering mode, operand layout, operand transform and epilogue runs here at shapes that straddle its tile boundaries.  Every
output buffer starts as NaN: the valid region must come back finite and correct, and everything else (padding columns, the gaps
between heads, one batch past the last) must still hold NaN.  CASES is plain data: tests/test_gemm_plan_cpu.py checks, without a
GPU, that it reaches every instantiation the launchers can produce.

Sections: a. plain products per (layout, tile, buffering), bit-identical to the natural dispatch; b. split-k; c. batched and
head-strided products; d. epilogues on the float4 and the scalar store path; e. epilogue and A-operand dropout (keep patterns exact);
f. the fused bias gradient; g. the soft-max epilogues and operand transforms."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.gpu_util import dropout_keep, log, relerr

pytestmark = pytest.mark.gpu

TOL = 2e-5
TILES = (128128, 128064, 64128, 64064, 128192)
LAYOUTS = ((1, 1), (1, 0), (0, 0), (0, 1))          # (akc, bkc); 128x192 and the operand transforms are not built for (0, 1)
TINY = 1.17549435e-38
SEED, SITE, ASITE = 0x1234_5678_9ABC, 37, 41


def tile_built(tile, akc, bkc):
    return tile != 128192 or akc or not bkc


def _r4(x):
    return (x + 3) // 4 * 4


def _plain(**kw):
    c = dict(akc=1, bkc=1, M=1, N=1, K=4, tile=0, sb=-1, splitk=1, outer=1, inner=1, alpha=1.0, bias=False, relu=0, mask=0,
             resid=False, drop=0.0, adrop=0.0, bias_out=False, a_mode=0, b_mode=0, offset=0, epi=0)
    c.update(kw)
    return c


def _shapes(akc, bkc, bm, bn):
    """eight (M, N, K) around one tile: M, N in {1, B-1, B, B+1, 2B+3} (rounded up to 4 where that operand is m/n-contiguous), K in
    {4, 28, 32, 36, 100, 1056} (odd where no operand is k-contiguous)"""
    Ms = [1, bm - 1, bm, bm + 1, 2 * bm + 3]
    Ns = [4, bn - 4, bn, bn + 4]
    Ks = [4, 28, 32, 36, 100, 1056]
    if not akc:
        Ms = [_r4(m) for m in Ms]
    if not bkc:
        Ns = [_r4(n) for n in Ns]
    else:
        Ns[0] = 3                                            # N % 4 != 0: the scalar store path
    if not akc and not bkc:
        Ks = [5, 27, 32, 33, 101, 1057]
    pick = [(0, 1, 4), (1, 2, 1), (2, 3, 2), (3, 0, 3), (4, 1, 0), (2, 2, 5), (3, 3, 4), (4, 2, 2)]
    return [(Ms[i], Ns[j], Ks[k]) for i, j, k in pick], Ms, Ns, Ks


def _build_cases():
    cases = []
    # a. every built (layout, tile, buffering): eight plain shapes, one with A-operand dropout, and the operand transforms where built
    for akc, bkc in LAYOUTS:
        for tile in TILES:
            if not tile_built(tile, akc, bkc):
                continue
            for sb in (0, 1):
                shapes, Ms, Ns, Ks = _shapes(akc, bkc, tile // 1000, tile % 1000)
                cfg = dict(akc=akc, bkc=bkc, tile=tile, sb=sb)
                for M, N, K in shapes:
                    cases.append(_plain(sec="a", M=M, N=N, K=K, **cfg))
                cases.append(_plain(sec="a", M=Ms[3], N=Ns[3], K=Ks[4], adrop=0.3, **cfg))
                if akc or not bkc:
                    cases.append(_plain(sec="a", M=Ms[3], N=Ns[1], K=Ks[4], a_mode=3, **cfg))
                    cases.append(_plain(sec="a", M=Ms[1], N=Ns[3], K=Ks[3], b_mode=2, **cfg))
    # a. the natural dispatch at the shapes that select 64x128 and both 128x192 forms
    cases.append(_plain(sec="a", akc=1, bkc=1, M=60, N=256, K=100))
    cases.append(_plain(sec="a", akc=0, bkc=0, M=64, N=384, K=77))
    cases.append(_plain(sec="a", akc=1, bkc=1, M=4100, N=192, K=1024))
    cases.append(_plain(sec="a", akc=1, bkc=0, M=4096, N=192, K=1028))
    cases.append(_plain(sec="a", akc=0, bkc=0, M=132, N=192, K=4099))
    # b. split-k, more splits than k-tiles included
    for akc, bkc, M, N, K in ((0, 0, 132, 68, 100), (0, 0, 64, 192, 1001), (1, 1, 77, 132, 100), (1, 0, 200, 64, 996)):
        for s in (2, 3, 7, 16, 64):
            cases.append(_plain(sec="b", akc=akc, bkc=bkc, M=M, N=N, K=K, splitk=s, alpha=0.75))
    cases.append(_plain(sec="b", akc=0, bkc=1, M=128, N=70, K=300, splitk=7, tile=64064, sb=1))
    # c. batched / head-strided: 3 images x {1, 4} heads, each operand a head slice of a [B, T, heads * width] tensor
    for akc, bkc, M, N, K in ((1, 1, 50, 36, 16), (1, 0, 50, 16, 36), (0, 0, 36, 16, 50), (0, 1, 16, 64, 33 * 4)):
        for inner in (1, 4):
            cases.append(_plain(sec="c", akc=akc, bkc=bkc, M=M, N=N, K=K, outer=3, inner=inner, alpha=0.5))
    cases.append(_plain(sec="c", akc=1, bkc=1, M=130, N=68, K=64, outer=3, inner=4, bias=True, relu=2, mask=1, resid=True, tile=64064, sb=0))
    # d. epilogues, float4 store path (offset 0, N % 4 == 0) and scalar path (C / bias offset by one float, or N % 4 != 0)
    epis = (dict(bias=True), dict(bias=True, relu=1), dict(bias=True, relu=2), dict(mask=1), dict(mask=2), dict(resid=True), dict(alpha=-1.5),
            dict(alpha=0.5, bias=True, relu=2, mask=2, resid=True))
    for akc, bkc in ((1, 1), (1, 0), (0, 0)):
        for e in epis:
            for M, N, off in ((150, 136, 0), (150, 136, 1), (33, 68, 1)):
                cases.append(_plain(sec="d", akc=akc, bkc=bkc, M=_r4(M) if not akc else M, N=N, K=52, offset=off, **e))
        for e in (dict(bias=True, relu=2), dict(alpha=0.5, bias=True, relu=1, mask=1, resid=True)):
            cases.append(_plain(sec="d", akc=akc, bkc=1, M=68 if not akc else 67, N=131, K=52, **e))
    # e. epilogue dropout (both store paths, batches) and A-operand dropout (both A layouts)
    for off, N in ((0, 136), (1, 136), (0, 133)):
        cases.append(_plain(sec="e", akc=1, bkc=1, M=100, N=N, K=40, drop=0.25, bias=True, relu=1, offset=off))
    cases.append(_plain(sec="e", akc=1, bkc=1, M=50, N=36, K=16, outer=3, inner=4, drop=0.4))
    cases.append(_plain(sec="e", akc=1, bkc=1, M=50, N=38, K=16, outer=3, inner=1, drop=0.4, offset=1))
    for akc, bkc, M, N, K in ((1, 1, 150, 72, 100), (1, 0, 150, 72, 100), (0, 0, 72, 100, 150), (0, 1, 72, 100, 152)):
        cases.append(_plain(sec="e", akc=akc, bkc=bkc, M=M, N=N, K=K, adrop=0.35))
    # f. fused bias gradient (dW form): N within and beyond one column tile, with and without split-k
    for bkc in (0, 1):
        for N in (60, 300):
            for s in (1, 4):
                cases.append(_plain(sec="f", akc=0, bkc=bkc, M=132, N=N, K=1000, splitk=s, bias_out=True))
    cases.append(_plain(sec="f", akc=0, bkc=0, M=192, N=192, K=4100, splitk=3, bias_out=True, adrop=0.2))
    cases.append(_plain(sec="f", akc=0, bkc=0, M=64, N=256, K=500, splitk=64, bias_out=True))
    # g. soft-max operand transforms at the natural dispatch (ragged M, vocabulary 256 / 4096 / 196)
    for akc, bkc, M, N, K, am, bm_ in ((1, 0, 200, 192, 4096, 3, 0), (1, 0, 77, 64, 196, 2, 0), (0, 0, 196, 192, 300, 3, 0),
                                       (0, 0, 256, 64, 77, 2, 0), (1, 1, 130, 196, 64, 0, 2), (1, 0, 130, 256, 64, 0, 2),
                                       (0, 0, 64, 196, 256, 0, 2), (1, 0, 100, 196, 256, 3, 2)):
        cases.append(_plain(sec="g", akc=akc, bkc=bkc, M=M, N=N, K=K, a_mode=am, b_mode=bm_))
    # g. soft-max epilogues (N = 160 has a 64-column segment wholly past N)
    for M, N in ((200, 256), (77, 4096), (130, 196), (130, 160)):
        cases.append(_plain(sec="g", epi=1, akc=1, bkc=1, M=M, N=N, K=64, bias=True, alpha=0.9))
        cases.append(_plain(sec="g", epi=2, akc=1, bkc=1, M=M, N=N, K=64, bias=True))
        cases.append(_plain(sec="g", epi=3, akc=1, bkc=0, M=M, N=N, K=64, alpha=0.9))
    return cases


CASES = _build_cases()


def _cid(c):
    s = f"{c['sec']}-a{c['akc']}b{c['bkc']}-{c['M']}x{c['N']}x{c['K']}"
    if c["tile"]:
        s += f"-t{c['tile'] // 1000}x{c['tile'] % 1000}sb{c['sb']}"
    for k in ("splitk", "outer", "inner"):
        if c[k] > 1:
            s += f"-{k}{c[k]}"
    for k in ("bias", "relu", "mask", "resid", "drop", "adrop", "bias_out", "a_mode", "b_mode", "offset", "epi"):
        if c[k]:
            s += f"-{k}{c[k] if not isinstance(c[k], bool) else ''}"
    if c["alpha"] != 1.0:
        s += f"-alpha{c['alpha']}"
    return s


def geometry(c):
    """storage of every operand: the logical A [M,K] / B [K,N] of batch z = (o, i) are head slices of [outer, rows, inner * width + 4];
    C is [outer + 1, inner, M + 1, N + 4] (a gap row per head and a whole batch past the end); offsets in floats"""
    M, N, K, akc, bkc, inner = c["M"], c["N"], c["K"], c["akc"], c["bkc"], c["inner"]
    g = {}
    if c["epi"] or c["splitk"] > 1:
        ldc = N + 4 if c["epi"] == 1 else N
    else:
        ldc = N + 4
    arows, aw = (M, K) if akc else (K, M)
    brows, bw = (N, K) if bkc else (K, N)
    g["lda"], g["ldb"], g["ldc"] = inner * aw + 4, inner * bw + 4, ldc
    g["sA"], g["sAi"] = arows * g["lda"], aw
    g["sB"], g["sBi"] = brows * g["ldb"], bw
    g["a_shape"], g["b_shape"] = (c["outer"], arows, g["lda"]), (c["outer"], brows, g["ldb"])
    if c["outer"] * inner > 1:
        g["sCi"] = (M + 1) * ldc
        g["sC"] = inner * g["sCi"]
    else:
        g["sC"] = g["sCi"] = 0
    g["c_floats"] = (c["outer"] + 1) * inner * (M + 1) * ldc + 4
    g["ldm"] = N + 4
    return g


def desc_fields(c, ptr):
    """ocrl_gemm_desc fields of a case; ptr(name) gives the address of a buffer (or 0 where the case has none)"""
    g = geometry(c)
    Z = c["outer"] * c["inner"]
    d = dict(A=ptr("A"), B=ptr("B"), C=ptr("C"), M=c["M"], N=c["N"], K=c["K"], lda=g["lda"], ldb=g["ldb"], ldc=g["ldc"], akc=c["akc"],
             bkc=c["bkc"], batch=Z, batch_inner=c["inner"], sA=g["sA"], sB=g["sB"], sC=g["sC"], sAi=g["sAi"] if c["inner"] > 1 else 0,
             sBi=g["sBi"] if c["inner"] > 1 else 0, sCi=g["sCi"], splitk=c["splitk"], alpha=c["alpha"], bias=ptr("bias"), relu=c["relu"],
             drop_p=c["drop"], drop_seed=SEED, drop_site=SITE, mask=ptr("mask"), ldmask=g["ldm"] if c["mask"] else 0,
             sMask=c["M"] * g["ldm"] if c["mask"] else 0, mask_elu=1 if c["mask"] == 2 else 0, resid=ptr("resid"),
             ldr=g["ldm"] if c["resid"] else 0, sR=c["M"] * g["ldm"] if c["resid"] else 0, adrop_p=c["adrop"], adrop_site=ASITE,
             adrop_ld=(c["K"] if c["akc"] else c["M"]) if c["adrop"] else 0, bias_out=ptr("bias_out"), a_mode=c["a_mode"],
             b_mode=c["b_mode"], x_lse=ptr("x_lse"), x_tok=ptr("x_tok"), x_scale=0.5 if c["a_mode"] == 3 else 1.0,
             force_tile=c["tile"], force_sb=c["sb"])
    if Z == 1:
        d.update(sA=0, sB=0)
    if c["epi"]:
        d.update(epi_mode=c["epi"], stat=ptr("stat"), hstat=ptr("hstat"), hidx=ptr("hidx"), e1=ptr("e1"), e2=ptr("e2"), e_lse=ptr("e_lse"),
                 e_rowvec=ptr("e_rowvec"), e_scale=0.7 if c["epi"] != 1 else 1.0)
        if c["epi"] == 3:
            d.update(mask=ptr("C"), ldmask=g["ldc"], sMask=0)
    return d


def buffers_present(c):
    """names of the buffers a case passes (the rest are null)"""
    names = {"A", "B", "C"}
    for k in ("bias", "resid", "bias_out"):
        if c[k]:
            names.add(k)
    if c["mask"]:
        names.add("mask")
    if c["a_mode"] or c["b_mode"]:
        names.add("x_lse")
        if c["a_mode"] == 3:
            names.add("x_tok")
    if c["epi"] in (1, 2):
        names.add("stat")
    if c["epi"] == 2:
        names.update(("hstat", "hidx", "e1", "e2"))
    if c["epi"] == 3:
        names.update(("e_lse", "e_rowvec"))
    return names


# ------------------------------------------------------------------------------------------------------------------- GPU side
def _lib():
    from ocrl_amd import _lib as L
    return L


def _launch(c, bufs, ws=None):
    L = _lib()
    present = buffers_present(c)

    def ptr(name):
        if name not in present:
            return None
        t = bufs[name]
        off = c["offset"] if name in ("C", "bias") else 0
        return t.data_ptr() + 4 * off
    d = L.gemm_desc(**desc_fields(c, ptr))
    L.check(L.lib().ocrl_gemm_ex(d, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), None))


def _xform(x, mode, lse, tok, scale):
    """fp64 operand transform (GemmArgs::a_mode / b_mode) of a stored operand: in either storage the token row is the stored row and the
    vocabulary index the column (k-contiguous: [mn][k]; m/n-contiguous: [k][mn])"""
    p = torch.exp(x - lse[:x.shape[0], None])
    if mode == 3:
        p = (p - (torch.arange(x.shape[1])[None, :] == tok[:x.shape[0], None]).double()) * scale
    return p


def _run_plain(c, natural=None):
    """one product of sections a-f / the transforms of g; returns (worst rel err, C valid region as a tensor, extra log text)"""
    M, N, K, akc, bkc = c["M"], c["N"], c["K"], c["akc"], c["bkc"]
    outer, inner, Z = c["outer"], c["inner"], c["outer"] * c["inner"]
    g = geometry(c)
    gen = torch.Generator().manual_seed(hash((M, N, K, akc, bkc, Z)) & 0xFFFFFFFF)
    Ast = torch.randn(*g["a_shape"], generator=gen)
    Bst = torch.randn(*g["b_shape"], generator=gen)
    bufs = dict(A=Ast.cuda(), B=Bst.cuda())
    bufs["C"] = torch.full((g["c_floats"],), float("nan"), device="cuda")
    bias = torch.randn(N + 4, generator=gen)
    mask = torch.randn(Z, M, g["ldm"], generator=gen)
    if c["mask"] == 2:
        mask = torch.where(mask > 0, mask, torch.expm1(mask))          # ELU outputs
    resid = torch.randn(Z, M, g["ldm"], generator=gen)
    vocab_rows = max(M, N, K)
    lse = 2.0 + torch.rand(vocab_rows, generator=gen)
    tok = torch.randint(-1, max(M, N, K), (vocab_rows,), generator=gen, dtype=torch.int32)
    bufs.update(bias=bias.cuda(), mask=mask.cuda(), resid=resid.cuda(), x_lse=lse.cuda(), x_tok=tok.cuda())
    bufs["bias_out"] = torch.full((M + 8,), float("nan"), device="cuda")
    ws = None
    if c["splitk"] > 1:
        ws = torch.full((c["splitk"] * (M * N + _r4(M)),), float("nan"), device="cuda")
    _launch(c, bufs, ws)
    torch.cuda.synchronize()

    # fp64 reference, batch by batch
    Cout = bufs["C"].cpu()
    off = c["offset"]
    ref = torch.empty(Z, M, N, dtype=torch.float64)
    got = torch.empty(Z, M, N, dtype=torch.float64)
    valid = torch.zeros(g["c_floats"], dtype=torch.bool)
    bref = None
    for z in range(Z):
        o, i = divmod(z, inner)
        aw = K if akc else M
        bw = K if bkc else N
        As = Ast[o, :, i * aw:(i + 1) * aw].double()
        Bs = Bst[o, :, i * bw:(i + 1) * bw].double()
        if c["adrop"]:
            keep = torch.from_numpy(dropout_keep(SEED, ASITE, c["adrop"], np.arange(As.numel()))).reshape(As.shape)
            As = As * keep.double() * float(np.float32(1.0) / (np.float32(1.0) - np.float32(c["adrop"])))
        if c["a_mode"]:
            As = _xform(As, c["a_mode"], lse.double(), tok.long(), 0.5)
        if c["b_mode"]:
            Bs = _xform(Bs, c["b_mode"], lse.double(), tok.long(), 1.0)
        A = As if akc else As.t()
        B = Bs.t() if bkc else Bs
        if c["bias_out"]:
            bref = A.sum(1)
        v = float(np.float32(c["alpha"])) * (A @ B)
        if c["splitk"] == 1:
            if c["bias"]:
                v = v + bias[off:off + N].double()
            if c["relu"] == 1:
                v = v.clamp_min(0)
            elif c["relu"] == 2:
                v = torch.where(v > 0, v, torch.expm1(v))
            if c["drop"]:
                idx = (z * M + np.arange(M)[:, None]) * N + np.arange(N)[None, :]
                keep = torch.from_numpy(dropout_keep(SEED, SITE, c["drop"], idx))
                v = v * keep.double() * float(np.float32(1.0) / (np.float32(1.0) - np.float32(c["drop"])))
            if c["mask"]:
                mk = mask[z, :, :N].double()
                v = torch.where(mk > 0, v, v * (mk + 1) if c["mask"] == 2 else torch.zeros_like(v))
            if c["resid"]:
                v = v + resid[z, :, :N].double()
        ref[z] = v
        base = off + o * g["sC"] + i * g["sCi"]
        pos = base + torch.arange(M)[:, None] * g["ldc"] + torch.arange(N)[None, :]
        valid[pos.reshape(-1)] = True
        got[z] = Cout[pos].double()
    assert torch.isfinite(got).all(), "non-finite values in the valid region"
    assert torch.isnan(Cout[~valid]).all(), "a write outside the valid region (padding, head gap or past the last batch)"
    err = relerr(got, ref)
    extra = ""
    if c["drop"]:
        keepm = torch.stack([torch.from_numpy(dropout_keep(SEED, SITE, c["drop"], (z * M + np.arange(M)[:, None]) * N + np.arange(N)[None, :]))
                             for z in range(Z)])
        clear = ref.abs() > 1e-3 * ref.abs().max()                  # a dropped element is exactly 0; a kept one carries its value
        assert torch.equal((got != 0) & clear, keepm & clear), "epilogue dropout keep pattern differs from csrc/common.h"
        extra += f" kept {keepm.double().mean().item():.3f}"
    if c["bias_out"]:
        bo = bufs["bias_out"].cpu()
        assert torch.isnan(bo[M:]).all(), "bias_out written past M"
        eb = relerr(bo[:M], bref)
        extra += f" bias_out {eb:.2e}"
        err = max(err, eb)
    return err, got, extra


def _sel(sec, pred=lambda c: True):
    return [pytest.param(c, id=_cid(c)) for c in CASES if c["sec"] == sec and pred(c)]


_natural = {}


@pytest.mark.parametrize("akc,bkc,tile,sb", [(a, b, t, s) for a, b in LAYOUTS for t in TILES if tile_built(t, a, b) for s in (0, 1)])
def test_a_every_instantiation(akc, bkc, tile, sb):
    """each (layout, tile, buffering) at shapes straddling the tile, with A-operand dropout and the operand transforms; with one split
    every forced kernel must equal the natural dispatch bit for bit: the per-element k order (8c + 4h + j within each 32-wide k-tile,
    k-tiles in order) does not depend on the tile shape or the buffering, and the epilogue arithmetic is the same"""
    mine = [c for c in CASES if c["sec"] == "a" and (c["akc"], c["bkc"], c["tile"], c["sb"]) == (akc, bkc, tile, sb)]
    assert len(mine) >= 9
    worst, nbit = 0.0, 0
    for c in mine:
        e, got, _ = _run_plain(c)
        assert e < TOL, (_cid(c), e)
        key = tuple(sorted((k, v) for k, v in c.items() if k not in ("tile", "sb")))
        if key not in _natural:
            _natural[key] = _run_plain(dict(c, tile=0, sb=-1))[1]
        assert torch.equal(got, _natural[key]), f"{_cid(c)} differs from the natural dispatch"
        nbit += 1
        worst = max(worst, e)
    log(f"gemm sweep a{akc}b{bkc} tile {tile // 1000}x{tile % 1000} sb{sb}: {len(mine)} products, worst {worst:.2e}, "
        f"{nbit} bit-identical to the natural dispatch")


@pytest.mark.parametrize("c", _sel("a", lambda c: c["tile"] == 0))
def test_a_natural_dispatch_at_the_rule_shapes(c):
    L = _lib()
    out = (ctypes.c_int * 6)()
    L.check(L.lib().ocrl_gemm_plan(L.gemm_desc(**desc_fields(c, lambda n: 0x100000 if n in buffers_present(c) else 0)), out))
    e, _, _ = _run_plain(c)
    log(f"gemm natural {_cid(c)} -> {out[0]}x{out[1]} sb{out[2]}: {e:.2e}")
    assert e < TOL


@pytest.mark.parametrize("c", _sel("b") + _sel("c") + _sel("d") + _sel("e") + _sel("f") + _sel("g", lambda c: not c["epi"]))
def test_products(c):
    e, got, extra = _run_plain(c)
    if c["splitk"] > 1 and not c["bias_out"]:
        e1 = relerr(got, _run_plain(dict(c, splitk=1))[1])
        extra += f" vs one split {e1:.2e}"
        assert e1 < TOL
    log(f"gemm {_cid(c)}: {e:.2e}{extra}")
    assert e < TOL


# ----------------------------------------------------------------------------------------------------------- soft-max epilogues
TIE_PATTERNS = ((1, 2), (5, 40), (3, 12), (28, 33))          # within a float4 group, across patches, across lanes, across the patch edge


def _run_epi(c):
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    g = geometry(c)
    ldc = g["ldc"]
    nseg = 2 * ((N + 127) // 128)
    gen = torch.Generator().manual_seed(M * 7919 + N * 31 + epi)
    A = (0.3 * torch.randn(M, g["lda"], generator=gen))
    bias = torch.randn(N + 4, generator=gen)
    if epi in (1, 2):
        Bst = 0.3 * torch.randn(N, g["ldb"], generator=gen)
        # tie columns: identical rows of B and equal bias give bitwise-equal logits
        for s in range(nseg):
            cols = [s * 64 + t for p in TIE_PATTERNS for t in p if s * 64 + t < N]
            if cols:
                Bst[cols] = Bst[cols[0]].clone()
                bias[cols] = bias[cols[0]].clone()
    else:
        Bst = 0.3 * torch.randn(K, g["ldb"], generator=gen)
    bufs = dict(A=A.cuda(), B=Bst.cuda(), bias=bias.cuda())
    e1 = torch.empty(M, N).exponential_(generator=gen)
    e2 = torch.empty(M, N).exponential_(generator=gen)
    for r in range(M):
        for s in range(nseg):
            for t in TIE_PATTERNS[r % len(TIE_PATTERNS)]:
                if s * 64 + t < N:
                    e2[r, s * 64 + t] = 1e-30                         # g2 = -log(1e-30) = 69: the tied columns hold the segment maximum
    y = torch.randn(M, ldc, generator=gen)
    e_lse = 1.0 + torch.rand(M, generator=gen)
    e_rowvec = torch.randn(M, generator=gen)
    if epi == 3:
        bufs["C"] = y.reshape(-1).clone().cuda()
    else:
        bufs["C"] = torch.full((M * ldc + 4,), float("nan"), device="cuda")
    bufs.update(stat=torch.full((M * nseg * 2 + 8,), float("nan"), device="cuda"), hstat=torch.full((M * nseg + 8,), float("nan"), device="cuda"),
                hidx=torch.full((M * nseg + 8,), -7, dtype=torch.int32, device="cuda"), e1=e1.cuda(), e2=e2.cuda(), e_lse=e_lse.cuda(),
                e_rowvec=e_rowvec.cuda())
    _launch(c, bufs)
    torch.cuda.synchronize()
    Cout = bufs["C"].cpu().reshape(-1)
    acc = A[:, :K].double() @ (Bst[:, :K].double().t() if epi != 3 else Bst[:, :N].double())
    alpha = float(np.float32(c["alpha"]))
    pos = torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :]
    valid = torch.zeros(Cout.numel(), dtype=torch.bool)
    valid[pos.reshape(-1)] = True
    got = Cout[pos].double()
    assert torch.isfinite(got).all()
    if epi == 3:
        ref = torch.exp(y[:, :N].double() - e_lse.double()[:, None]) * (alpha * acc - e_rowvec.double()[:, None]) * float(np.float32(0.7))
        assert torch.equal(Cout[~valid], y.reshape(-1)[~valid[:M * ldc]]), "soft-max backward wrote outside [M, N]"
        return dict(C=relerr(got, ref))
    assert torch.isnan(Cout[~valid]).all(), "soft-max epilogue wrote outside [M, N]"
    lgt = alpha * acc + bias[:N].double()
    if epi == 1:
        ref = lgt
    else:
        ref = (lgt - torch.log(e1.double() + TINY)) * float(np.float32(0.7))
    errs = dict(C=relerr(got, ref))
    # per (row, 64-column segment) statistics of the written values; a segment wholly past N holds (-inf, 0)
    stat = bufs["stat"].cpu()
    assert torch.isnan(stat[M * nseg * 2:]).all()
    st = stat[:M * nseg * 2].reshape(M, nseg, 2).double()
    smax = torch.full((M, nseg), -math.inf, dtype=torch.float64)
    ssum = torch.zeros(M, nseg, dtype=torch.float64)
    for s in range(nseg):
        lo, hi = s * 64, min(N, s * 64 + 64)
        if lo < hi:
            smax[:, s] = ref[:, lo:hi].max(1).values
            ssum[:, s] = torch.exp(ref[:, lo:hi] - smax[:, s:s + 1]).sum(1)
    live = torch.isfinite(smax)
    assert torch.equal(st[..., 0][~live], smax[~live]) and torch.equal(st[..., 1][~live], ssum[~live]), "empty segment statistics"
    # the pair is graded as the segment's log-sum-exp (the max is the max of written values, so it matches C's error)
    errs["stat"] = relerr(st[..., 0][live] + torch.log(st[..., 1][live]), smax[live] + torch.log(ssum[live]))
    errs["stat_max"] = relerr(st[..., 0][live], smax[live])
    if epi == 2:
        h = lgt - torch.log(e2.double() + TINY)
        hst = bufs["hstat"].cpu()
        hix = bufs["hidx"].cpu()
        assert torch.isnan(hst[M * nseg:]).all() and (hix[M * nseg:] == -7).all()
        hst, hix = hst[:M * nseg].reshape(M, nseg).double(), hix[:M * nseg].reshape(M, nseg)
        hmax = torch.full((M, nseg), -math.inf, dtype=torch.float64)
        harg = torch.zeros(M, nseg, dtype=torch.int32)
        for s in range(nseg):
            lo, hi = s * 64, min(N, s * 64 + 64)
            if lo < hi:
                mx = h[:, lo:hi].max(1)
                hmax[:, s] = mx.values
                harg[:, s] = lo + torch.argmax((h[:, lo:hi] == mx.values[:, None]).int(), 1).int()      # the lowest column of the maximum
        assert torch.equal(hst[~live], hmax[~live]) and (hix[~live] == 0).all(), "empty segment hard-sample statistics"
        errs["hstat"] = relerr(hst[live], hmax[live])
        bad = (hix != harg) & live
        assert not bad.any(), f"hard-sample column: kernel {hix[bad][:8].tolist()} reference (lowest tied column) {harg[bad][:8].tolist()}"
    return errs


@pytest.mark.parametrize("c", _sel("g", lambda c: c["epi"] > 0))
def test_softmax_epilogue(c):
    errs = _run_epi(c)
    log(f"gemm {_cid(c)}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs
