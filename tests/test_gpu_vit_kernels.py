"""The pooling-Transformer and masked-autoencoder kernels (pool.hip, pool_long.hip, mae.hip) one by one through
include/ocrl_hip_vit_kernels.h against the fp64 references of tests/vit_kernels_ref.py, at the shapes the whole-model tests do not reach:
the short attention at its limit S = 32, with a second trip of its pair loop and exactly at the 160 KiB backward limit; the flash
attention at every head size across sub-block, key-tile and query-block boundaries, with dropout, seeds above 2^32 and scores far from zero;
the CLS-row attention at head counts that leave waves with 0, 1 or 2 heads and at 1, 2, 3 and 5 chunks; the MAE row kernels, GELU,
LayerNorm (every F / 4 tail, the 256-chunk cap) and loss (3 p p below 256 and above 512).

Harness: every output lies between sentinel bands and is pre-filled with NaN, every input is followed by NaN, scratch is NaN-filled and
sized to the float, every call runs twice and must repeat bit for bit, and image 0 of a batch must equal the same image run alone bit for
bit wherever the arithmetic is per image.  Data movement is compared to the bit.  Everything else: TOL = 2e-5 of the reference tensor's
maximum per output tensor, or max(TOL, 4 x floor) where FLOORS lists what the reference's own formula loses in fp32 on the CPU (held to its
measurement by tests/test_vit_kernels_ref_cpu.py).  An output that is exactly zero by construction (dq, dk, w at S = 1) is held to TOL of
the terms it cancels from.

Worst measured error per family on an MI355X, relative to the reference's maximum (every bit comparison: 0 mismatches): pool_attn 7.4e-7
(dv, S 32, hd 64, p 0.1); pool_flash 4.5e-6 (dk at the +-50 scores, d 48; below 1e-6 on the plain inputs); CLS row 2.8e-6 (dX at the +-50
scores); cls_drop with a residual 5.4e-8; GELU 6.9e-8; LayerNorm 1.4e-6 (dg, the row of mean 100); loss 9.4e-8; d cls 7.0e-8; d mask_token
1.9e-7."""
import ctypes
import math

import pytest
import torch

from tests import vit_kernels_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu
TOL = 2e-5
NAN = float("nan")
SENTINEL = -777.0
BAND = 64
SITE = R.SITE

# (key of vit_kernels_ref.floor_cases(), output) -> what torch's fp32 evaluation of the reference's formula loses against fp64, relative to the
# output's maximum; only the entries above TOL / 4 are listed, every other output holds plain TOL.  Measured with torch 2.x on an x86-64 CPU.
FLOORS = {
    (("flash", 40, 96, 3, "wide"), "dk"): 5.8e-6,
    (("flash", 40, 144, 3, "wide"), "dk"): 5.6e-6,
    (("cls", 2, 129, 128, 8, "wide"), "dX"): 5.3e-6,
}


# every entry point of the header and its argument count: what this file runs (tests/test_vit_kernels_ref_cpu.py holds the header to it)
ENTRIES = {"ocrl_vit_pool_embed": 8, "ocrl_vit_pool_rows": 7, "ocrl_vit_pool_attn_fwd": 11, "ocrl_vit_pool_attn_bwd": 12, "ocrl_vit_pool_short_ok": 4,
           "ocrl_vit_pool_cols": 8, "ocrl_vit_cls_drop": 11, "ocrl_vit_cls_add": 6, "ocrl_vit_flash_fwd": 11, "ocrl_vit_flash_bwd": 14,
           "ocrl_vit_cls_nchunk": 3, "ocrl_vit_cls_part_floats": 5, "ocrl_vit_cls_attn_fwd": 18, "ocrl_vit_cls_attn_bwd": 26,
           "ocrl_vit_patch_gather": 9, "ocrl_vit_tokens_fwd": 10, "ocrl_vit_tokens_bwd": 7, "ocrl_vit_unshuffle_fwd": 10, "ocrl_vit_unshuffle_bwd": 11,
           "ocrl_vit_gelu_fwd": 4, "ocrl_vit_gelu_bwd": 5, "ocrl_vit_ln_chunks": 1, "ocrl_vit_ln_fwd": 10, "ocrl_vit_ln_bwd": 14, "ocrl_vit_loss": 13}


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


def sync():
    torch.cuda.synchronize()


class Out:
    """an output (or scratch) of the given shape, NaN-filled, between two sentinel bands"""

    def __init__(self, *shape):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * BAND,), SENTINEL, device="cuda", dtype=torch.float32)
        self.t = self.buf[BAND:BAND + n].view(*shape)
        self.t.fill_(NAN)
        _KEEP.append(self)

    def done(self, tag):
        assert bool((self.buf[:BAND] == SENTINEL).all()) and bool((self.buf[-BAND:] == SENTINEL).all()), f"{tag}: wrote outside its output"
        return self.t.clone()


def inp(t, dtype=torch.float32):
    """a device copy of t followed by a band of NaN (ints: of -2^30)"""
    t = t.detach().to(dtype).contiguous()
    buf = torch.full((t.numel() + BAND,), NAN if dtype == torch.float32 else -(1 << 30), device="cuda", dtype=dtype)
    buf[:t.numel()] = t.reshape(-1).cuda()
    _KEEP.append(buf)
    return buf[:t.numel()].view(t.shape)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def twice(tag, fn):
    """run fn twice: every output must repeat bit for bit"""
    a, b = fn(), fn()
    for k in a:
        assert bits_equal(a[k], b[k]), f"{tag}: {k} differs between two identical calls"
    return a


def err(got, ref, scale=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = ref.abs().max().item() if scale is None else scale
    d = (got - ref).abs().max().item() if ref.numel() else 0.0
    if den == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / den


def grade(tag, rows):
    """rows: (name, got, ref, bar[, scale]); logs every error, then asserts finiteness and the bars"""
    out = []
    for name, got, ref, bar, *scale in rows:
        assert bool(torch.isfinite(got).all()), f"{tag}: {name} is not finite"
        out.append((name, err(got, ref.reshape(got.shape), *scale), bar))
    log(f"[vit {tag}] " + " ".join(f"{n}={e:.1e}" + (f"(bar {b:.1e})" if b != TOL else "") for n, e, b in out))
    bad = [(n, e, b) for n, e, b in out if not e <= b]
    assert not bad, (tag, bad)


def exact(tag, got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu().to(got.dtype).reshape(got.shape)
    n = int((got != ref).sum())
    log(f"[vit {tag}] mismatches={n}")
    assert n == 0 and bool(torch.isfinite(got.double()).all()), (tag, n)


def keep_mask(site, n, p, seed):
    m = torch.full((n,), NAN, device="cuda")
    ok(lib().ocrl_tp_dropout_mask(P(m), site, n, p, seed, stream()))
    sync()
    assert bool(((m == 0) | (m == 1)).all())
    return m.cpu().double()


# ------------------------------------------------------------------------------------------------------------------- short path
def run_pool_attn(qkv, dO, B, S, d, h, p, seed):
    L = lib()
    Pm, O, dqkv = Out(B, h, S, S), Out(B * S, d), Out(B * S, 3 * d)
    x = inp(qkv)
    ok(L.ocrl_vit_pool_attn_fwd(P(x), P(Pm.t), P(O.t), B, S, d, h, p, seed, SITE, stream()))
    ok(L.ocrl_vit_pool_attn_bwd(P(x), P(Pm.t), P(inp(dO)), P(dqkv.t), B, S, d, h, p, seed, SITE, stream()))
    sync()
    g = dqkv.done("dqkv")
    return dict(P=Pm.done("P"), O=O.done("O"), dq=g[:, :d], dk=g[:, d:2 * d], dv=g[:, 2 * d:])


@pytest.mark.parametrize("B,S,d,h,p,seed", R.POOL_ATTN_CASES, ids=[f"B{c[0]}-S{c[1]}-d{c[2]}-h{c[3]}-p{c[4]}" for c in R.POOL_ATTN_CASES])
def test_pool_attn(B, S, d, h, p, seed):
    tag = f"pool_attn B{B} S{S} d{d} h{h} p{p}"
    qkv, dO = R.attn_inputs(B, S, d, h)
    keep = keep_mask(SITE, B * h * S * S, p, seed) if p else None
    ref = R.attention(qkv, B, S, d, h, keep, p, dO)
    got = twice(tag, lambda: run_pool_attn(qkv, dO, B, S, d, h, p, seed))
    key = ("pool_attn", S, d, h, "randn")
    zs = [ref["zero_scale"]] if S == 1 else []
    grade(tag, [("P", got["P"], ref["P"], bar_of(key, "P")), ("O", got["O"], ref["O"], bar_of(key, "O")),
                ("dq", got["dq"], ref["dq"], bar_of(key, "dq"), *zs), ("dk", got["dk"], ref["dk"], bar_of(key, "dk"), *zs),
                ("dv", got["dv"], ref["dv"], bar_of(key, "dv"))])
    if B > 1:
        one = run_pool_attn(qkv[:S], dO[:S], 1, S, d, h, p, seed)
        for k in ("P", "O", "dq", "dk", "dv"):
            assert bits_equal(one[k], got[k][:1] if k == "P" else got[k][:S]), f"{tag}: image 0 of {k} depends on the batch"


@pytest.mark.parametrize("B,K,d", [(1, 1, 4), (3, 6, 64), (5, 31, 36)])
def test_pool_embed_and_rows(B, K, d):
    L = lib()
    g = R.gen(31, B, K, d)
    lin, cls, pos = R.randn(g, B, K, d), R.randn(g, d), R.randn(g, K + 1, d)
    for with_pos in (False, True):
        def run(lin=lin, B=B):
            x0 = Out(B, K + 1, d)
            ok(L.ocrl_vit_pool_embed(P(inp(lin)), P(inp(cls)), P(inp(pos)) if with_pos else None, P(x0.t), B, K, d, stream()))
            sync()
            return dict(x0=x0.done("x0"))
        got = twice("pool_embed", run)["x0"]
        if with_pos:
            exact(f"pool_embed pos B{B} K{K} d{d}", got, R.pool_embed(lin, cls, pos))        # one fp32 add: the same bits
        else:
            exact(f"pool_embed B{B} K{K} d{d}", got, R.pool_embed(lin, cls, None))
        assert bits_equal(run(lin[:1], 1)["x0"], got[:1])
    x, dout = R.randn(g, B, K + 1, d), R.randn(g, B, d)
    for mode, src, shape in ((0, x, (B * K, d)), (1, dout, (B, K + 1, d)), (2, x, (B, d))):
        def run():
            o = Out(*shape)
            ok(L.ocrl_vit_pool_rows(P(inp(src)), P(o.t), B, K, d, mode, stream()))
            sync()
            return dict(o=o.done("rows"))
        exact(f"pool_rows mode{mode} B{B} K{K} d{d}", twice("pool_rows", run)["o"], R.pool_rows(src, K, mode))


# ------------------------------------------------------------------------------------------------------------------- flash attention
def run_flash(qkv, dO, B, S, d, h, p, seed):
    L = lib()
    O, lse, Dd, dqkv = Out(B * S, d), Out(B * h, S), Out(B * h, S), Out(B * S, 3 * d)
    x = inp(qkv)
    ok(L.ocrl_vit_flash_fwd(P(x), P(O.t), P(lse.t), B, S, d, h, p, seed, SITE, stream()))
    ok(L.ocrl_vit_flash_bwd(P(x), P(O.t), P(lse.t), P(inp(dO)), P(Dd.t), P(dqkv.t), B, S, d, h, p, seed, SITE, stream()))
    sync()
    g = dqkv.done("dqkv")
    return dict(O=O.done("O"), lse=lse.done("lse"), Dd=Dd.done("Dd"), dq=g[:, :d], dk=g[:, d:2 * d], dv=g[:, 2 * d:])


@pytest.mark.parametrize("B,S,d,h,p,seed,kind", R.FLASH_CASES, ids=[f"{c[6]}-S{c[1]}-d{c[2]}-h{c[3]}-p{c[4]}" for c in R.FLASH_CASES])
def test_pool_flash(B, S, d, h, p, seed, kind):
    tag = f"flash {kind} B{B} S{S} d{d} h{h} p{p}"
    qkv, dO = R.attn_inputs(B, S, d, h, kind)
    keep = keep_mask(SITE, B * h * S * S, p, seed) if p else None
    ref = R.attention(qkv, B, S, d, h, keep, p, dO)
    got = twice(tag, lambda: run_flash(qkv, dO, B, S, d, h, p, seed))
    key = ("flash", S, d, h, kind)
    zs = [ref["zero_scale"]] if S == 1 else []
    grade(tag, [(n, got[n], ref[n], bar_of(key, n), *(zs if n in ("dq", "dk") else [])) for n in ("O", "lse", "Dd", "dq", "dk", "dv")])
    one = run_flash(qkv[:S], dO[:S], 1, S, d, h, p, seed)
    for k in ("O", "dq", "dk", "dv"):
        assert bits_equal(one[k], got[k][:S]), f"{tag}: image 0 of {k} depends on the batch"
    for k in ("lse", "Dd"):
        assert bits_equal(one[k], got[k][:h]), f"{tag}: image 0 of {k} depends on the batch"


# ------------------------------------------------------------------------------------------------------------------- CLS-row attention
def run_cls(i, B, S, d, h, p, seed):
    L = lib()
    X, Win, bin_, q, dO = (inp(t) for t in i)
    x0 = inp(i[0][:, 0])
    nf, nb = L.ocrl_vit_cls_part_floats(B, S, d, h, 0), L.ocrl_vit_cls_part_floats(B, S, d, h, 1)
    U, z, stat, o, pf = Out(B, h, d), Out(B, h, d), Out(B, h, 2), Out(B, d), Out(nf)
    ok(L.ocrl_vit_cls_attn_fwd(P(X), P(Win), P(bin_), P(q), P(U.t), P(z.t), P(stat.t), P(o.t), P(pf.t), nf, B, S, d, h, p, seed, SITE, stream()))
    G, gD, dX, w, dq, dW, db, pb = Out(B, h, d), Out(B, h, 2), Out(B, S, d), Out(B, h, d), Out(B, d), Out(3 * d, d), Out(3 * d), Out(nb)
    ok(L.ocrl_vit_cls_attn_bwd(P(X), P(Win), P(bin_), P(q), P(U.t), P(z.t), P(stat.t), P(dO), P(x0), P(G.t), P(gD.t), P(dX.t), P(w.t), P(dq.t),
                               P(dW.t), P(db.t), P(pb.t), nb, B, S, d, h, p, seed, SITE, stream()))
    sync()
    pf.done("part fwd"), pb.done("part bwd")
    return {n: t.done(n) for n, t in dict(U=U, z=z, stat=stat, o=o, G=G, gD=gD, dX=dX, w=w, dq=dq, dW=dW, db=db).items()}


CLS_OUT = ("U", "z", "stat", "o", "G", "gD", "dX", "w", "dq", "dW", "db")


@pytest.mark.parametrize("B,S,d,h,p,seed,kind,chunks", R.CLS_CASES, ids=[f"{c[6]}-B{c[0]}-S{c[1]}-d{c[2]}-h{c[3]}-p{c[4]}" for c in R.CLS_CASES])
def test_cls_row_attention(B, S, d, h, p, seed, kind, chunks):
    tag = f"cls {kind} B{B} S{S} d{d} h{h} p{p}"
    c = ctypes.c_int()
    assert lib().ocrl_vit_cls_nchunk(B, S, ctypes.byref(c)) == chunks and c.value % 64 == 0 and (chunks - 1) * c.value < S <= chunks * c.value
    if S in (65, 129):
        assert S - (chunks - 1) * c.value == 1                    # a last chunk of one row
    i = R.cls_inputs(B, S, d, h, kind)
    keep = keep_mask(SITE, B * h * S * S, p, seed)[R.cls_keep_index(B, S, h)] if p else None
    ref = R.cls_attn(*i[:4], B, S, d, h, keep, p, i[4])
    got = twice(tag, lambda: run_cls(i, B, S, d, h, p, seed))
    key = ("cls", B, S, d, h, kind)
    zs = {"w": [ref["zero_scale_w"]], "dq": [ref["zero_scale_dq"]]} if S == 1 else {}
    grade(tag, [(n, got[n], ref[n], bar_of(key, n), *zs.get(n, [])) for n in CLS_OUT])
    exact(tag + " k-bias rows of db", got["db"][d:2 * d], torch.zeros(d))
    if 1 < B <= 2:
        one = run_cls((i[0][:1], i[1], i[2], i[3][:1], i[4][:1]), 1, S, d, h, p, seed)
        for k in ("U", "z", "stat", "o", "G", "gD", "dX", "w", "dq"):
            assert bits_equal(one[k], got[k][:1]), f"{tag}: image 0 of {k} depends on the batch"


# ------------------------------------------------------------------------------------------------------------------- pool_cls_drop / _add / pool_cols
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [64, 512])
def test_cls_drop_and_add(B, N):
    L = lib()
    S, ldr = 33, N + 4
    g = R.gen(37, B, N)
    x, resid, dX = R.randn(g, B, N), R.randn(g, B, ldr), R.randn(g, B, S, N)
    for p, seed in ((0.0, 0), (0.1, R.SEED_LO), (0.5, R.SEED_HI)):
        kp = (keep_mask(SITE + 1, B * S * N, p, seed)[R.cls_drop_index(B, N, S)].reshape(B, N) if p else torch.ones(B, N, dtype=torch.float64))
        assert p == 0 or 0 < kp.mean().item() < 1
        for with_resid in (True, False):
            def run():
                o = Out(B, N)
                ok(L.ocrl_vit_cls_drop(P(inp(x)), P(inp(resid)) if with_resid else None, ldr if with_resid else 0, P(o.t), B, N, S, p, seed, SITE + 1, stream()))
                sync()
                return dict(o=o.done("cls_drop"))
            got = twice("cls_drop", run)["o"]
            scaled = x * (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))) if p else x      # the kernel's own fp32 product
            dropped = torch.where(kp > 0, scaled, torch.zeros_like(x))
            name = f"cls_drop B{B} N{N} p{p} resid{int(with_resid)}"
            if with_resid and p:                                  # a product and a sum: the compiler may fuse them
                grade(name, [("out", got, dropped.double() + resid[:, :N].double(), TOL)])
            else:
                exact(name, got, dropped + (resid[:, :N] if with_resid else 0.0))
    def run_add():
        t = Out(B, S, N)
        t.t.copy_(dX.cuda())
        ok(L.ocrl_vit_cls_add(P(t.t), P(inp(x)), B, N, S, stream()))
        sync()
        return dict(o=t.done("cls_add"))
    want = dX.clone()
    want[:, 0] += x
    exact(f"cls_add B{B} N{N}", twice("cls_add", run_add)["o"], want)


@pytest.mark.parametrize("Din", [3, 67])
@pytest.mark.parametrize("rows", [1, 5 * 77])
def test_pool_cols_pads_and_unpads(Din, rows):
    L = lib()
    Dp = (Din + 3) & ~3
    src = R.randn(R.gen(41, Din, rows), rows, Din)
    def pad():
        o = Out(rows, Dp)
        ok(L.ocrl_vit_pool_cols(P(inp(src)), Din, P(o.t), Dp, rows, Dp, Din, stream()))
        sync()
        return dict(o=o.done("pool_cols"))
    padded = twice("pool_cols", pad)["o"]
    exact(f"pool_cols pad Din{Din} rows{rows}", padded, R.pool_cols(src, Dp, Din))
    def unpad():
        o = Out(rows, Din)
        ok(L.ocrl_vit_pool_cols(P(inp(padded)), Dp, P(o.t), Din, rows, Din, Din, stream()))
        sync()
        return dict(o=o.done("pool_cols"))
    exact(f"pool_cols unpad Din{Din} rows{rows}", twice("pool_cols", unpad)["o"], src)


# ------------------------------------------------------------------------------------------------------------------- MAE: gather and row kernels
@pytest.mark.parametrize("S,p", R.GATHER_CASES)
def test_patch_gather(S, p):
    L = lib()
    Lp, Pp = (S // p) ** 2, 3 * p * p
    for B in (1, 3):
        obs = R.randn(R.gen(43, S, p, B), B, 3, S, S)
        for n, with_ids in ((Lp, False), (Lp, True), (Lp - 1, True), (1, True), (Lp - 1, False)):
            ids = torch.stack([torch.randperm(Lp, generator=R.gen(47, b, n))[:n] for b in range(B)]).int() if with_ids else None
            want = R.patch_gather(obs, ids, n, p)
            for force, shift in ((0, 0), (1, 0), (0, 1)):
                def run():
                    o = Out(B * n, Pp)
                    buf = torch.full((obs.numel() + shift + BAND,), NAN, device="cuda")
                    buf[shift:shift + obs.numel()] = obs.reshape(-1).cuda()
                    _KEEP.append(buf)
                    ok(L.ocrl_vit_patch_gather(P(buf[shift:]), P(inp(ids, torch.int32)) if with_ids else None, P(o.t), B, n, S, p, force, stream()))
                    sync()
                    return dict(o=o.done("gather"))
                exact(f"patch_gather S{S} p{p} B{B} n{n} ids{int(with_ids)} scalar{force} shift{shift}", twice("gather", run)["o"], want)


@pytest.mark.parametrize("D", [4, 36, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_tokens_and_unshuffle(D, B):
    L = lib()
    Lp = 9
    g = R.gen(53, D, B)
    cls, pos, mtok, dpos = R.randn(g, D), R.randn(g, Lp + 1, D), R.randn(g, D), R.randn(g, Lp + 1, D)
    for n in (1, Lp - 1, Lp):
        restore, keep, mask = R.mae_ids(B, Lp, n)
        embed, dx0 = R.randn(g, B, n, D), R.randn(g, B, n + 1, D)
        for ids in (None, keep):
            def fwd(embed=embed, ids=ids, B=B):
                o = Out(B, n + 1, D)
                ok(L.ocrl_vit_tokens_fwd(P(inp(embed)), P(inp(cls)), P(inp(pos)), None if ids is None else P(inp(ids, torch.int32)), P(o.t), B, n, Lp, D, stream()))
                sync()
                return dict(o=o.done("tokens"))
            got = twice("tokens", fwd)["o"]
            exact(f"tokens_fwd D{D} B{B} n{n} ids{int(ids is not None)}", got, R.tokens_fwd(embed, cls, pos, ids))
            assert bits_equal(fwd(embed[:1], None if ids is None else ids[:1], 1)["o"], got[:1])
        def bwd():
            de, dc = Out(B * n, D), Out(D)
            ok(L.ocrl_vit_tokens_bwd(P(inp(dx0)), P(de.t), P(dc.t), B, n, D, stream()))
            sync()
            return dict(de=de.done("dembed"), dc=dc.done("dcls"))
        got = twice("tokens_bwd", bwd)
        exact(f"tokens_bwd dembed D{D} B{B} n{n}", got["de"], dx0[:, 1:])
        grade(f"tokens_bwd dcls D{D} B{B} n{n}", [("dcls", got["dc"], dx0[:, 0].double().sum(0), TOL)])
        # unshuffle: len_keep = n
        e, dxd = R.randn(g, B, n + 1, D), R.randn(g, B, Lp + 1, D)
        def ufwd():
            o = Out(B, Lp + 1, D)
            ok(L.ocrl_vit_unshuffle_fwd(P(inp(e)), P(inp(mtok)), P(inp(dpos)), P(inp(restore, torch.int32)), P(o.t), B, Lp, n, D, stream()))
            sync()
            return dict(o=o.done("unshuffle"))
        exact(f"unshuffle_fwd D{D} B{B} keep{n}", twice("unshuffle", ufwd)["o"], R.unshuffle_fwd(e, mtok, dpos, restore))
        def ubwd():
            de, dm, part = Out(B, n + 1, D), Out(D), Out(B * D)
            ok(L.ocrl_vit_unshuffle_bwd(P(inp(dxd)), P(inp(keep, torch.int32)), P(inp(mask)), P(de.t), P(dm.t), P(part.t), B, Lp, n, D, stream()))
            sync()
            part.done("part")
            return dict(de=de.done("de"), dm=dm.done("dmtok"))
        got = twice("unshuffle_bwd", ubwd)
        ev, dv = e.double().requires_grad_(True), mtok.double().requires_grad_(True)
        (R.unshuffle_fwd(ev, dv, dpos.double(), restore) * dxd.double()).sum().backward()
        exact(f"unshuffle_bwd de D{D} B{B} keep{n}", got["de"], ev.grad)                          # a gather: the same bits
        if n == Lp:
            exact(f"unshuffle_bwd dmtok at len_keep = L D{D} B{B}", got["dm"], torch.zeros(D))
        else:
            grade(f"unshuffle_bwd dmtok D{D} B{B} keep{n}", [("dmtok", got["dm"], dv.grad, TOL)])


# ------------------------------------------------------------------------------------------------------------------- MAE: GELU, LayerNorm, loss
@pytest.mark.parametrize("n4", [1, 257])
def test_gelu(n4):
    L = lib()
    x, dy = R.gelu_inputs(n4)
    n = 4 * n4
    def run():
        y, dp = Out(n), Out(n)
        inplace = Out(n)
        inplace.t.copy_(dy.cuda())
        px = inp(x)
        ok(L.ocrl_vit_gelu_fwd(P(px), P(y.t), n, stream()))
        ok(L.ocrl_vit_gelu_bwd(P(inp(dy)), P(px), P(dp.t), n, stream()))
        ok(L.ocrl_vit_gelu_bwd(P(inplace.t), P(px), P(inplace.t), n, stream()))
        sync()
        return dict(y=y.done("y"), dpre=dp.done("dpre"), inplace=inplace.done("in place"))
    got = twice("gelu", run)
    grade(f"gelu n4 {n4}", [("y", got["y"], R.gelu(x), bar_of(("gelu",), "y")), ("dpre", got["dpre"], R.gelu_grad(x, dy), bar_of(("gelu",), "dpre"))])
    assert bits_equal(got["inplace"], got["dpre"])


def run_ln(x, gam, beta, dy, resid, R_, F_, eps):
    L = lib()
    n = L.ocrl_vit_ln_chunks(R_)
    y, mean, rstd, dx, dg, db, part = Out(R_, F_), Out(R_), Out(R_), Out(R_, F_), Out(F_), Out(F_), Out(2 * F_ * n)
    px, pg = inp(x), inp(gam)
    ok(L.ocrl_vit_ln_fwd(P(px), P(pg), P(inp(beta)), P(y.t), P(mean.t), P(rstd.t), R_, F_, eps, stream()))
    ok(L.ocrl_vit_ln_bwd(P(inp(dy)), P(px), P(mean.t), P(rstd.t), P(pg), None if resid is None else P(inp(resid)), P(dx.t), P(dg.t), P(db.t),
                         P(part.t), 2 * F_ * n, R_, F_, stream()))
    sync()
    part.done("part")
    return {k: t.done(k) for k, t in dict(y=y, mean=mean, rstd=rstd, dx=dx, dg=dg, db=db).items()}


def check_ln(tag, R_, F_, eps, kind="randn", with_resid=True, key=None):
    x, gam, beta, dy, resid = R.ln_inputs(R_, F_, kind)
    resid = resid if with_resid else None
    got = twice(tag, lambda: run_ln(x, gam, beta, dy, resid, R_, F_, eps))
    ref = {**R.layernorm(x, gam, beta, eps), **R.layernorm_bwd(dy, x, gam, eps, resid)}
    grade(tag, [(n, got[n], ref[n], TOL if key is None else bar_of(key, n)) for n in ("y", "mean", "rstd", "dx", "dg", "db")])
    if R_ > 1:
        one = run_ln(x[:1], gam, beta, dy[:1], None if resid is None else resid[:1], 1, F_, eps)
        for k in ("y", "mean", "rstd", "dx"):
            assert bits_equal(one[k], got[k][:1]), f"{tag}: row 0 of {k} depends on the other rows"


@pytest.mark.parametrize("F_", R.LN_F)
def test_layernorm(F_):
    for j, R_ in enumerate(R.LN_R):
        check_ln(f"ln F{F_} R{R_}", R_, F_, (1e-6, 1e-5)[j % 2], with_resid=bool((j // 2) % 2))
        assert lib().ocrl_vit_ln_chunks(R_) == R.ln_chunks(R_)[0]


def test_layernorm_hard_rows_and_the_chunk_cap():
    assert lib().ocrl_vit_ln_chunks(2049) == 228 and R.ln_chunks(2049) == (228, 9) and 2049 - 227 * 9 == 6       # 9-row chunks, a last one of 6
    assert lib().ocrl_vit_ln_chunks(2041) == 256 and R.ln_chunks(2041) == (256, 8) and 2041 - 255 * 8 == 1       # the 256-chunk cap, a last chunk of 1
    check_ln("ln F32 R2049", 2049, 32, 1e-6)
    check_ln("ln F32 R2041 cap", 2041, 32, 1e-6)


@pytest.mark.parametrize("kind,F_", R.LN_HARD)
def test_layernorm_hard_rows(kind, F_):
    """a row of mean 100 and spread 1; a constant row (fp64: y = beta, a zero variance, rstd = eps^-1/2); rows of spread 1e-3, where the
    variance is of the size of eps and a kernel that took 1e-5 for 1e-6 is off by a third.  Each at both eps, every output at TOL."""
    for eps in R.LN_EPS:
        check_ln(f"ln {kind} F{F_} eps{eps}", 5, F_, eps, kind, key=("ln", kind, F_, eps))


@pytest.mark.parametrize("S,p", R.LOSS_CASES)
@pytest.mark.parametrize("B", [1, 3])
def test_mae_loss(S, p, B):
    L = lib()
    Lp, Pp = (S // p) ** 2, 3 * p * p
    g = R.gen(59, S, p, B)
    obs, pred = torch.rand(B, 3, S, S, generator=g), R.randn(g, B, Lp, Pp)
    m = 2 * (Lp // 4)                                             # patches removed per image on average; the kernel divides by B m
    len_keep = Lp - m
    if B == 1:
        mask = R.mae_ids(1, Lp, len_keep)[2]
    else:                                                         # image 0's mask is all zero: the others carry its share
        mask = torch.cat([torch.zeros(1, Lp), R.mae_ids(B - 1, Lp, Lp - m * B // (B - 1))[2]])
    assert mask.sum().item() == B * m and (B == 1 or mask[0].sum().item() == 0)
    dloss = torch.tensor([0.37])
    ref = R.mae_loss(pred, obs, mask, p, 0.37)
    def run(want_loss=True, want_dpred=True):
        loss, dpred, part = Out(2), Out(B, Lp + 1, Pp), Out(B * Lp)
        ok(L.ocrl_vit_loss(P(inp(pred)), P(inp(obs)), P(inp(mask)), P(inp(dloss)) if want_dpred else None, P(part.t) if want_loss else None,
                           P(loss.t) if want_loss else None, P(dpred.t) if want_dpred else None, B, Lp, len_keep, S, p, stream()))
        sync()
        out = {}
        if want_loss:
            out["loss"] = loss.done("loss")
            part.done("part")
        else:
            assert bool(torch.isnan(loss.t).all()) and bool(torch.isnan(part.t).all())
        if want_dpred:
            out["dpred"] = dpred.done("dpred")
        else:
            assert bool(torch.isnan(dpred.t).all())
        return out
    tag = f"mae_loss S{S} p{p} B{B}"
    got = twice(tag, run)
    grade(tag, [("loss", got["loss"], ref["loss"].expand(2), TOL), ("dpred", got["dpred"], ref["dpred"], TOL)])
    exact(tag + " CLS rows of dpred", got["dpred"][:, 0], torch.zeros(B, Pp))
    assert bits_equal(run(True, False)["loss"], got["loss"]) and bits_equal(run(False, True)["dpred"], got["dpred"])
    if B == 1:                                                    # len_keep = L: the divisor is zero and the loss NaN, as in the reference
        loss, part = Out(2), Out(Lp)
        ok(L.ocrl_vit_loss(P(inp(pred)), P(inp(obs)), P(inp(torch.zeros(1, Lp))), None, P(part.t), P(loss.t), None, 1, Lp, Lp, S, p, stream()))
        sync()
        assert bool(torch.isnan(loss.t).all())


# ------------------------------------------------------------------------------------------------------------------- the short path's admissibility
SHORT_REFUSED = [(28, 128, 16, "LDS"), (31, 256, 8, "LDS"), (6, 192, 4, "head size")]          # (K, d, h, reason)


@pytest.mark.parametrize("K,d,h,why", SHORT_REFUSED)
def test_pool_transformer_refuses_what_its_backward_cannot_run(K, d, h, why):
    """both directions refuse before any launch: nothing is written"""
    from ocrl_amd import _lib
    L = lib()
    B, Din, ff, nl = 2, 64, 256, 1
    assert not L.ocrl_vit_pool_short_ok(K, Din, d, h) and why in L.ocrl_last_error().decode()
    n = L.ocrl_pool_transformer_ws_floats(B, K, d, h, ff, nl)
    assert n > 0
    shapes = [(d, Din), (d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (ff, d), (ff,), (d, ff), (d,), (d,), (d,), (d,), (d,)]
    w = [torch.zeros(s, device="cuda") for s in shapes]
    g = [torch.full(s, NAN, device="cuda") for s in shapes]
    ws, out, ds = torch.full((n,), NAN, device="cuda"), torch.full((B, d), NAN, device="cuda"), torch.full((B, K, Din), NAN, device="cuda")
    slots, dout = torch.zeros(B, K, Din, device="cuda"), torch.zeros(B, d, device="cuda")
    refused(L.ocrl_pool_transformer_fwd(_lib.ptr(slots), _lib.ptrs(w), None, _lib.ptr(out), B, K, Din, d, h, ff, nl, 0.0, 0, _lib.ptr(ws), n, None), why)
    refused(L.ocrl_pool_transformer_bwd(_lib.ptr(slots), _lib.ptr(dout), _lib.ptrs(w), _lib.ptr(ds), _lib.ptrs(g), B, K, Din, d, h, ff, nl, 0.0, 0,
                                        _lib.ptr(ws), n, None), why)
    sync()
    assert all(bool(torch.isnan(t).all()) for t in [ws, out, ds] + g)


@pytest.mark.parametrize("K,d,h,nl", [(31, 256, 8, 2), (6, 192, 4, 1)])
def test_module_takes_the_long_path_where_the_short_one_cannot_run(K, d, h, nl):
    """Transformer_Module at a shape the short path refuses (the LDS request of its backward; head size 48) and the long path accepts:
    forward and backward against the oracle in fp64 at the pooling files' bars"""
    from oracle import pooling_oracle as PO
    from ocrl_amd.poolings import Transformer_Module
    from tests.test_gpu_pooling_long import _pool_cfg, compare
    assert not lib().ocrl_vit_pool_short_ok(K, 64, d, h)
    cfg = PO.default_cfg(rep_dim=64, num_slots=K, d_model=d, nhead=h, num_layers=nl, pos_emb="ape")
    m = Transformer_Module(64, K, _pool_cfg(d_model=d, nhead=h, num_layers=nl)).cuda().eval()
    Pm = PO.formula_params(cfg)
    m.load_state_dict({**m.state_dict(), **Pm})
    g = torch.Generator().manual_seed(6)
    slots, cot = torch.randn(3, K, 64, generator=g), torch.randn(3, d, generator=g)
    x = slots.cuda().requires_grad_(True)
    out = m(x)
    (out * cot.cuda()).sum().backward()
    named = dict(m.named_parameters())
    r_out, r_g, r_ds = PO.loss_and_grads(Pm, slots, cfg, cot, dtype=torch.float64)
    compare(f"module K{K} d{d} h{h} L{nl}", (out.detach().cpu(), {n: named[n].grad.cpu() for n in r_g}, x.grad.cpu()), (r_out, r_g, r_ds))


@pytest.mark.parametrize("K,d,h,why", [(30, 128, 16, "LDS request"), (31, 256, 32, "LDS request"), (6, 64, 16, "head size 4")])
def test_module_refuses_at_the_first_forward_what_neither_path_runs(K, d, h, why):
    """head sizes 8 and 4 are the short path's alone (the long path has 16 / 32 / 48 / 64): where its backward does not fit, or the head size
    is not one of its own, the module says so at the first forward, in eval and in train mode, and not at the first backward"""
    from ocrl_amd.poolings import Transformer_Module
    from tests.test_gpu_pooling_long import _pool_cfg
    m = Transformer_Module(64, K, _pool_cfg(d_model=d, nhead=h)).cuda()
    for mode in (m.eval, m.train):
        mode()
        with pytest.raises(ValueError, match=why):
            m(torch.zeros(2, K, 64, device="cuda"))
