"""What the pooling-Transformer / MAE kernel tests rest on, without a GPU: the eleventh header (include/ocrl_hip_vit_kernels.h) parses, binds
and is exported while the older tables stay as they were; every refusal its entry points make before a launch; the short path's
admissibility rule and the two chunk rules against Python restatements; the references of tests/vit_kernels_ref.py against independent
torch code (scaled_dot_product_attention, an explicit masked soft-max, row 0 of the full attention through the in-projection, autograd,
Conv2d, patchify); that the cases of tests/test_gpu_vit_kernels.py are what they are named (dropout keeps and drops in every head, ragged
tails exist, wrong restatements move the outputs by more than 100 x the tolerance); and the fp32 floors its bars rest on."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from ocrl_amd import _abi, _lib
from tests import test_gpu_vit_kernels as G
from tests import vit_kernels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is refused before any launch
EXACT = 1e-10                   # fp64 against fp64: the same operation written twice


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_vit_kernels.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == G.ENTRIES and abi.consts == {} and abi.structs == {}
    assert set(_lib.ABI_VIT_KERNELS.functions) == set(G.ENTRIES)
    L = _lib.lib()
    for n, k in G.ENTRIES.items():
        assert len(getattr(L, n).argtypes) == k, n                                         # the symbol is exported and bound
    assert L.ocrl_vit_cls_part_floats.restype is ctypes.c_size_t
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_VIT_KERNELS_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                         # self-contained
    src = open(os.path.join(ROOT, "tests", "test_gpu_vit_kernels.py")).read()
    assert all(re.search(rf"\.{n}\(", src) for n in G.ENTRIES), [n for n in G.ENTRIES if not re.search(rf"\.{n}\(", src)]      # the GPU file runs each
    flat = " ".join(text.replace("\n *", " ").split())
    for word in ("S <= 32", "{8, 16, 32, 64}", "160 KiB", "{16, 32, 48, 64}", "d <= 256", "h <= 16", "h d <= 4096", "<= 1024", "S % p"):
        assert word in flat, word                                                          # the comment names the limits
    # the older tables are what they were: the additions are additive
    assert len(_lib.ABI.functions) == 146 and _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    older = (_lib.ABI, _lib.ABI_DQN, _lib.ABI_ROLLOUT, _lib.ABI_REPLAY, _lib.ABI_C51, _lib.ABI_NOISY, _lib.ABI_CLASSIFIER, _lib.ABI_IODINE, _lib.ABI_QR,
             _lib.ABI_SLATE_KERNELS)
    assert [len(a.functions) for a in older] == [146, 9, 1, 8, 6, 5, 1, 21, 6, 26]
    assert not any(set(G.ENTRIES) & set(a.functions) for a in older)
    mk = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    objs, hdrs = (re.search(rf"^{v} = (.*)$", mk, re.M).group(1).split() for v in ("OBJS", "HDRS"))
    assert "vit_kernels_unit.o" in objs and "../../include/ocrl_hip_vit_kernels.h" in hdrs


# ---- refusals before any launch
def refused(rc, *words):
    msg = _lib.lib().ocrl_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_arguments_are_checked_before_any_launch():
    L = _lib.lib()
    p, odd, big = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4), 1 << 40

    def emb(lin=p, cls=p, pos=p, x0=p, B=2, K=6, d=64):
        return L.ocrl_vit_pool_embed(lin, cls, pos, x0, B, K, d, None)
    refused(emb(d=6), "d % 4 == 0"), refused(emb(B=0), "B, K >= 1"), refused(emb(K=0), "B, K >= 1"), refused(emb(d=0), "d >= 4")
    refused(emb(lin=None), "null"), refused(emb(cls=None), "null"), refused(emb(x0=None), "null")
    for k in ("lin", "cls", "pos", "x0"):
        refused(emb(**{k: odd}), "aligned")
    refused(L.ocrl_vit_pool_rows(p, p, 2, 6, 64, 3, None), "mode"), refused(L.ocrl_vit_pool_rows(p, p, 2, 6, 64, -1, None), "mode")
    refused(L.ocrl_vit_pool_rows(p, p, 2, 6, 66, 0, None), "d % 4 == 0"), refused(L.ocrl_vit_pool_rows(p, None, 2, 6, 64, 0, None), "null")
    refused(L.ocrl_vit_pool_rows(odd, p, 2, 6, 64, 0, None), "aligned"), refused(L.ocrl_vit_pool_rows(p, odd, 2, 6, 64, 0, None), "aligned")
    refused(L.ocrl_vit_pool_rows(p, p, 0, 6, 64, 0, None), "B, K >= 1")

    def afwd(qkv=p, P=p, O=p, B=2, S=7, d=64, h=4, pr=0.0):
        return L.ocrl_vit_pool_attn_fwd(qkv, P, O, B, S, d, h, pr, 0, 1, None)

    def abwd(qkv=p, P=p, dO=p, dqkv=p, B=2, S=7, d=64, h=4, pr=0.0):
        return L.ocrl_vit_pool_attn_bwd(qkv, P, dO, dqkv, B, S, d, h, pr, 0, 1, None)
    for f in (afwd, abwd):
        refused(f(S=33), "tokens <= 32"), refused(f(S=0), "B, S, d, h >= 1"), refused(f(B=0), "B, S, d, h >= 1"), refused(f(h=0), "B, S, d, h >= 1")
        refused(f(h=3), "not divisible")
        refused(f(d=192, h=4), "head size 48"), refused(f(d=64, h=16), "head size 4"), refused(f(d=128, h=1), "head size 128")
        refused(f(pr=1.0), "0 <= p < 1"), refused(f(pr=-0.5), "0 <= p < 1"), refused(f(qkv=None), "null"), refused(f(P=None), "null")
        refused(f(qkv=odd), "aligned")
    refused(afwd(O=None), "null"), refused(afwd(O=odd), "aligned"), refused(abwd(dO=None), "null"), refused(abwd(dqkv=None), "null")
    refused(abwd(dO=odd), "aligned"), refused(abwd(dqkv=odd), "aligned")
    # the LDS request of either direction: the forward's 12 S d, the backward's 4 (4 S d + 2 h S S)
    refused(afwd(S=32, d=512, h=8), "fwd: LDS request 196608"), refused(abwd(S=29, d=128, h=16), "bwd: LDS request 167040")
    refused(abwd(S=32, d=256, h=8), "bwd: LDS request 196608")
    assert abwd(S=32, d=256, h=4, B=0) != 0 and afwd(S=29, d=128, h=16, B=0) != 0          # (accepted shapes: refused here only for B)

    refused(L.ocrl_vit_pool_cols(p, 3, p, 4, 0, 4, 3, None), "rows, ncols, ncopy >= 1"), refused(L.ocrl_vit_pool_cols(p, 3, p, 4, 5, 4, 5, None), "ncopy <= ncols")
    refused(L.ocrl_vit_pool_cols(p, 2, p, 4, 5, 4, 3, None), "lds >= ncopy"), refused(L.ocrl_vit_pool_cols(p, 3, p, 3, 5, 4, 3, None), "ldd >= ncols")
    refused(L.ocrl_vit_pool_cols(None, 3, p, 4, 5, 4, 3, None), "null"), refused(L.ocrl_vit_pool_cols(p, 3, None, 4, 5, 4, 3, None), "null")
    refused(L.ocrl_vit_cls_drop(p, p, 63, p, 2, 64, 5, 0.1, 0, 1, None), "ldr >= N"), refused(L.ocrl_vit_cls_drop(p, None, 0, p, 0, 64, 5, 0.1, 0, 1, None), "B, N, S >= 1")
    refused(L.ocrl_vit_cls_drop(p, None, 0, p, 2, 64, 5, 1.0, 0, 1, None), "0 <= p < 1"), refused(L.ocrl_vit_cls_drop(None, None, 0, p, 2, 64, 5, 0.1, 0, 1, None), "null")
    refused(L.ocrl_vit_cls_drop(p, None, 0, None, 2, 64, 5, 0.1, 0, 1, None), "null")
    refused(L.ocrl_vit_cls_add(p, p, 2, 0, 5, None), "B, d, S >= 1"), refused(L.ocrl_vit_cls_add(None, p, 2, 64, 5, None), "null"), refused(L.ocrl_vit_cls_add(p, None, 2, 64, 5, None), "null")

    def ffwd(qkv=p, O=p, lse=p, B=2, S=40, d=96, h=3, pr=0.0):
        return L.ocrl_vit_flash_fwd(qkv, O, lse, B, S, d, h, pr, 0, 1, None)

    def fbwd(qkv=p, O=p, lse=p, dO=p, Dd=p, dqkv=p, B=2, S=40, d=96, h=3, pr=0.0):
        return L.ocrl_vit_flash_bwd(qkv, O, lse, dO, Dd, dqkv, B, S, d, h, pr, 0, 1, None)
    for f in (ffwd, fbwd):
        refused(f(d=64, h=8), "16, 32, 48 or 64"), refused(f(d=128, h=1), "16, 32, 48 or 64"), refused(f(d=100, h=3), "16, 32, 48 or 64")
        refused(f(S=0), "B, S, d, h >= 1"), refused(f(B=0), "B, S, d, h >= 1"), refused(f(h=0), "B, S, d, h >= 1"), refused(f(pr=1.0), "0 <= p < 1")
        refused(f(B=30000), "B h <= 65535")
        refused(f(qkv=None), "null"), refused(f(O=None), "null"), refused(f(lse=None), "null"), refused(f(qkv=odd), "aligned")
    refused(ffwd(O=odd), "aligned"), refused(fbwd(dO=None), "null"), refused(fbwd(Dd=None), "null"), refused(fbwd(dqkv=None), "null")
    refused(fbwd(dO=odd), "aligned"), refused(fbwd(dqkv=odd), "aligned")

    def cfwd(X=p, q=p, U=p, o=p, part=p, n=big, B=2, S=65, d=128, h=8, pr=0.0):
        return L.ocrl_vit_cls_attn_fwd(X, p, p, q, U, p, p, o, part, n, B, S, d, h, pr, 0, 1, None)

    def cbwd(X=p, dO=p, dX=p, db=p, part=p, n=big, B=2, S=65, d=128, h=8, pr=0.0):
        return L.ocrl_vit_cls_attn_bwd(X, p, p, p, p, p, p, dO, p, p, p, dX, p, p, p, db, part, n, B, S, d, h, pr, 0, 1, None)
    for f, back in ((cfwd, 0), (cbwd, 1)):
        refused(f(d=320, h=5), "d <= 256"), refused(f(d=126, h=2), "d % 4 == 0"), refused(f(d=64, h=32), "h <= 16"), refused(f(d=128, h=3), "d % h == 0")
        refused(f(S=0), "B, S, d, h >= 1"), refused(f(B=0), "B, S, d, h >= 1"), refused(f(h=0), "B, S, d, h >= 1"), refused(f(pr=1.0), "0 <= p < 1")
        refused(f(B=70000, S=1), "B <= 65535")
        refused(f(X=None), "null"), refused(f(part=None), "null"), refused(f(X=odd), "aligned"), refused(f(part=odd), "aligned")
        need = L.ocrl_vit_cls_part_floats(2, 65, 128, 8, back)
        assert need == 2 * 2 * 8 * (128 if back else 132)
        refused(f(n=need - 1), "part too small"), refused(f(n=0), "part too small")
        assert L.ocrl_vit_cls_part_floats(2, 65, 320, 5, back) == 0 and L.ocrl_vit_cls_part_floats(0, 65, 128, 8, back) == 0
    refused(cfwd(q=None), "null"), refused(cfwd(U=None), "null"), refused(cfwd(o=None), "null"), refused(cbwd(dO=None), "null"), refused(cbwd(db=None), "null")
    refused(cbwd(dX=None), "null"), refused(cbwd(dX=odd), "aligned")
    assert L.ocrl_vit_cls_nchunk(0, 5, None) == 0 and L.ocrl_vit_cls_nchunk(5, 0, None) == 0

    def gat(obs=p, out=p, B=2, n=9, S=12, pp=4):
        return L.ocrl_vit_patch_gather(obs, None, out, B, n, S, pp, 0, None)
    refused(gat(S=14), "S % p == 0"), refused(gat(n=10), "n <= L"), refused(gat(n=0), "n <= L"), refused(gat(pp=0), "B, S, p >= 1"), refused(gat(B=0), "B, S, p >= 1")
    refused(gat(S=132, pp=4, n=5), "<= 1024"), refused(gat(obs=None), "null"), refused(gat(out=None), "null")

    def tok(embed=p, cls=p, pos=p, x0=p, B=2, n=4, Lp=9, D=64):
        return L.ocrl_vit_tokens_fwd(embed, cls, pos, None, x0, B, n, Lp, D, None)
    refused(tok(D=6), "% 4 == 0"), refused(tok(D=0), "% 4 == 0"), refused(tok(n=10), "<= L"), refused(tok(n=0), "<= L"), refused(tok(Lp=1025, n=4), "L <= 1024")
    refused(tok(B=0), "1 <= B <= 65535"), refused(tok(embed=None), "null"), refused(tok(x0=None), "null")
    for k in ("embed", "cls", "pos", "x0"):
        refused(tok(**{k: odd}), "aligned")
    refused(L.ocrl_vit_tokens_bwd(p, p, p, 2, 4, 6, None), "% 4 == 0"), refused(L.ocrl_vit_tokens_bwd(p, p, p, 0, 4, 64, None), "B, n >= 1")
    refused(L.ocrl_vit_tokens_bwd(p, p, None, 2, 4, 64, None), "null"), refused(L.ocrl_vit_tokens_bwd(odd, p, p, 2, 4, 64, None), "aligned")
    refused(L.ocrl_vit_tokens_bwd(p, odd, p, 2, 4, 64, None), "aligned")

    def ufwd(e=p, mtok=p, dpos=p, restore=p, xd=p, B=2, Lp=9, keep=4, D=64):
        return L.ocrl_vit_unshuffle_fwd(e, mtok, dpos, restore, xd, B, Lp, keep, D, None)

    def ubwd(dxd=p, keep_=p, mask=p, de=p, dm=p, part=p, B=2, Lp=9, keep=4, D=64):
        return L.ocrl_vit_unshuffle_bwd(dxd, keep_, mask, de, dm, part, B, Lp, keep, D, None)
    for f in (ufwd, ubwd):
        refused(f(D=6), "% 4 == 0"), refused(f(keep=0), "len_keep <= L"), refused(f(keep=10), "len_keep <= L"), refused(f(Lp=1025), "L <= 1024")
        refused(f(Lp=0), "L <= 1024"), refused(f(B=0), "1 <= B <= 65535")
    refused(ufwd(restore=None), "null"), refused(ufwd(mtok=None), "null"), refused(ubwd(part=None), "null"), refused(ubwd(mask=None), "null")
    for k in ("e", "mtok", "dpos", "xd"):
        refused(ufwd(**{k: odd}), "aligned")
    refused(ubwd(dxd=odd), "aligned"), refused(ubwd(de=odd), "aligned")

    refused(L.ocrl_vit_gelu_fwd(p, p, 6, None), "n % 4 == 0"), refused(L.ocrl_vit_gelu_fwd(p, p, 0, None), "n % 4 == 0"), refused(L.ocrl_vit_gelu_fwd(p, None, 8, None), "null")
    refused(L.ocrl_vit_gelu_fwd(odd, p, 8, None), "aligned"), refused(L.ocrl_vit_gelu_fwd(p, odd, 8, None), "aligned")
    refused(L.ocrl_vit_gelu_bwd(p, p, p, 6, None), "n % 4 == 0"), refused(L.ocrl_vit_gelu_bwd(None, p, p, 8, None), "null")
    for a in ((odd, p, p), (p, odd, p), (p, p, odd)):
        refused(L.ocrl_vit_gelu_bwd(*a, 8, None), "aligned")

    def lfwd(x=p, g=p, b=p, y=p, mean=p, Rr=5, F_=64, eps=1e-6):
        return L.ocrl_vit_ln_fwd(x, g, b, y, mean, p, Rr, F_, eps, None)

    def lbwd(dy=p, x=p, g=p, resid=p, dx=p, dg=p, part=p, n=big, Rr=5, F_=64):
        return L.ocrl_vit_ln_bwd(dy, x, p, p, g, resid, dx, dg, p, part, n, Rr, F_, None)
    for f in (lfwd, lbwd):
        refused(f(F_=6), "% 4 == 0"), refused(f(F_=0), "% 4 == 0"), refused(f(Rr=0), "R >= 1"), refused(f(x=None), "null"), refused(f(x=odd), "aligned"), refused(f(g=odd), "aligned")
    refused(lfwd(eps=0.0), "eps must be positive"), refused(lfwd(mean=None), "null"), refused(lfwd(b=odd), "aligned"), refused(lfwd(y=odd), "aligned")
    refused(lbwd(dg=None), "null"), refused(lbwd(part=None), "null"), refused(lbwd(dy=odd), "aligned"), refused(lbwd(resid=odd), "aligned"), refused(lbwd(dx=odd), "aligned")
    refused(lbwd(Rr=17, n=2 * 64 * L.ocrl_vit_ln_chunks(17) - 1), "part too small")
    assert L.ocrl_vit_ln_chunks(0) == 0 and L.ocrl_vit_ln_chunks(17) == 3

    def loss(pred=p, obs=p, mask=p, dloss=p, part=p, out=p, dpred=p, B=2, Lp=9, keep=4, S=12, pp=4):
        return L.ocrl_vit_loss(pred, obs, mask, dloss, part, out, dpred, B, Lp, keep, S, pp, None)
    refused(loss(part=None), "loss needs part"), refused(loss(dloss=None), "dpred needs dloss"), refused(loss(out=None, dpred=None), "nothing to compute")
    refused(loss(S=14), "S % p == 0"), refused(loss(Lp=8), "L == (S / p)^2"), refused(loss(keep=0), "len_keep <= L"), refused(loss(keep=10), "len_keep <= L")
    refused(loss(S=132, Lp=1089), "<= 1024"), refused(loss(B=0), "B, S, p >= 1"), refused(loss(pred=None), "null"), refused(loss(obs=None), "null"), refused(loss(mask=None), "null")
    refused(loss(B=70000, S=4, pp=4, Lp=1, keep=1), "B <= 65535")


# ---- the host rules against Python restatements
def test_short_path_admissibility_is_the_two_lds_formulas():
    L = _lib.lib()
    n_ok = n_no = 0
    for d in (64, 128, 192, 256):
        for h in (h for h in range(1, d + 1) if d % h == 0):
            for K in range(1, 32):
                want = R.pool_short_ok(K, 64, d, h)
                assert bool(L.ocrl_vit_pool_short_ok(K, 64, d, h)) == want, (K, d, h)
                n_ok, n_no = n_ok + want, n_no + (not want)
    assert n_ok > 100 and n_no > 100
    assert R.pool_attn_lds(32, 256, 4)[1] == 160 * 1024 and L.ocrl_vit_pool_short_ok(31, 64, 256, 4)          # exactly at the limit: accepted
    for K, d, h in ((28, 128, 16), (31, 256, 8)):
        assert not L.ocrl_vit_pool_short_ok(K, 64, d, h) and b"bwd: LDS request" in L.ocrl_last_error()
        assert max(R.pool_attn_lds(K + 1, d, h)) > 160 * 1024 >= R.pool_attn_lds(K + 1, d, h)[0]             # the forward alone would run
    assert L.ocrl_vit_pool_short_ok(27, 64, 128, 16) and L.ocrl_vit_pool_short_ok(31, 64, 128, 2)
    assert not L.ocrl_vit_pool_short_ok(6, 64, 192, 4) and b"head size 48" in L.ocrl_last_error()
    # where the refused shapes go: the long path takes head sizes 16 / 32 / 48 / 64, so d = 128, h = 16 (head size 8) has no path at all
    ws = L.ocrl_pool_transformer_long_ws_floats
    assert ws(2, 31, 64, 256, 8, 256, 1) > 0 and ws(2, 31, 64, 256, 16, 256, 2) > 0 and ws(2, 6, 64, 192, 4, 256, 2) > 0
    assert ws(2, 28, 64, 128, 16, 256, 1) == 0 and b"head size" in L.ocrl_last_error() and ws(2, 31, 64, 256, 32, 256, 1) == 0
    for K, Din, d, h in ((0, 64, 128, 8), (32, 64, 128, 8), (6, 67, 128, 8), (6, 64, 96, 4), (6, 64, 320, 5), (6, 64, 128, 0), (6, 64, 128, 3)):
        assert not L.ocrl_vit_pool_short_ok(K, Din, d, h) and not R.pool_short_ok(K, Din, d, h)


def test_chunk_rules_yield_nonempty_chunks():
    L = _lib.lib()
    c = ctypes.c_int()
    near = lambda xs, top: sorted({v + k for v in xs for k in (-1, 0, 1) if 1 <= v + k <= top})
    Bs = near((1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 32, 64, 100, 128, 204, 205, 256, 341, 342, 512, 1023, 1024, 1025, 2048), 2048)
    Ss = near((1, 2, 63, 64, 65, 127, 128, 129, 130, 192, 193, 256, 300, 320, 321, 640, 1024, 1025, 4096, 4097, 5000), 5000) + list(range(1, 5000, 37))
    seen = set()
    for B in Bs:
        for S in Ss:
            n = L.ocrl_vit_cls_nchunk(B, S, ctypes.byref(c))
            assert (n, c.value) == R.cls_nchunk(B, S), (B, S)
            assert c.value % 64 == 0 and (n - 1) * c.value < S <= n * c.value and n <= max(1, -(-1024 // B))          # every chunk non-empty
            seen.add(min(n, 3))
            if B >= 1024:
                assert n == 1
    assert seen == {1, 2, 3} and R.cls_nchunk(2, 129) == (3, 64) and R.cls_nchunk(1024, 130) == (1, 192)
    for Rr in list(range(1, 2200)) + near((2040, 2041, 2048, 2049, 2056, 4096, 5000), 5000):
        n, rpc = R.ln_chunks(Rr)
        assert L.ocrl_vit_ln_chunks(Rr) == n and 1 <= n <= 256 and (n - 1) * rpc < Rr <= n * rpc
    assert R.ln_chunks(2041) == (256, 8) and R.ln_chunks(2049) == (228, 9)


# ---- the references against independent torch code
@pytest.mark.parametrize("B,S,d,h", [(2, 7, 64, 4), (2, 33, 96, 3), (1, 40, 64, 1)])
def test_attention_reference_is_torchs(B, S, d, h):
    qkv, dO = R.attn_inputs(B, S, d, h)
    x = qkv.double().reshape(B, S, 3, h, d // h).requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * S, d)
    (o * dO.double()).sum().backward()
    ref = R.attention(qkv, B, S, d, h, dO=dO)
    gx = x.grad.reshape(B * S, 3, d)
    assert R.rel(ref["O"], o) < EXACT and all(R.rel(ref[n], gx[:, i]) < EXACT for i, n in enumerate(("dq", "dk", "dv")))
    s = (q @ k.transpose(-1, -2) / math.sqrt(d // h)).detach()
    assert R.rel(ref["lse"], s.logsumexp(-1).reshape(B * h, S)) < EXACT and R.rel(ref["P"], s.softmax(-1)) < EXACT
    assert R.rel(ref["Dd"], (ref["P"] * (dO.double().reshape(B, S, h, -1).transpose(1, 2) @ v.detach().transpose(-1, -2))).sum(-1).reshape(B * h, S)) < EXACT
    # with dropout: an explicit masked soft-max under autograd
    p = 0.5
    keep = R.host_keep(R.SEED_HI, R.SITE, p, B * h * S * S)
    x.grad = None
    o = ((s_ := (q @ k.transpose(-1, -2) / math.sqrt(d // h))).softmax(-1) * keep.reshape(B, h, S, S) / (1 - p) @ v).transpose(1, 2).reshape(B * S, d)
    (o * dO.double()).sum().backward()
    ref = R.attention(qkv, B, S, d, h, keep, p, dO)
    gx = x.grad.reshape(B * S, 3, d)
    assert R.rel(ref["O"], o) < EXACT and all(R.rel(ref[n], gx[:, i]) < EXACT for i, n in enumerate(("dq", "dk", "dv")))


@pytest.mark.parametrize("B,S,d,h,p", [(2, 65, 64, 2, 0.0), (2, 9, 192, 3, 0.1), (1, 130, 128, 8, 0.5)])
def test_cls_reference_is_row_0_of_the_full_attention(B, S, d, h, p):
    X, Win, bin_, q, dO = R.cls_inputs(B, S, d, h)
    hd = d // h
    keep = R.host_keep(R.SEED_LO, R.SITE, p, B * h * S * S)[R.cls_keep_index(B, S, h)].reshape(B, h, S) if p else torch.ones(B, h, S, dtype=torch.float64)
    Xv, Wv, bv = X.double().requires_grad_(True), Win.double().requires_grad_(True), bin_.double().requires_grad_(True)
    x0 = Xv[:, 0].detach()                                       # q is an input of its own: its path back into X belongs to the caller
    qv = x0 @ Wv[:d].t() + bv[:d]
    qv.retain_grad()
    kk, vv = (Xv @ Wv[i * d:(i + 1) * d].t() + bv[i * d:(i + 1) * d] for i in (1, 2))                          # the in-projection, k bias included
    heads = lambda t: t.reshape(B, -1, h, hd).transpose(1, 2)
    s = heads(qv[:, None]) @ heads(kk).transpose(-1, -2) / math.sqrt(hd)                                       # [B, h, 1, S]
    o = ((s.softmax(-1) * keep[:, :, None] / (1 - p)) @ heads(vv)).transpose(1, 2).reshape(B, d)
    (o * dO.double()).sum().backward()
    ref = R.cls_attn(X, Win, bin_, qv.detach(), B, S, d, h, keep if p else None, p, dO)
    assert R.rel(ref["o"], o) < EXACT and R.rel(ref["dX"], Xv.grad) < EXACT and R.rel(ref["dq"], qv.grad) < EXACT
    assert R.rel(ref["dW"], Wv.grad) < EXACT and R.rel(ref["db"], bv.grad) < 1e-9                               # autograd's k-bias rows: rounding residue
    assert bool((ref["db"][d:2 * d] == 0).all()) and bv.grad[d:2 * d].abs().max() < 1e-12 * bv.grad.abs().max()
    assert R.rel(ref["stat"][..., 1], (s[:, :, 0] - (heads(qv[:, None]) @ bv[d:2 * d].reshape(1, h, hd, 1))[:, :, 0] / math.sqrt(hd)).logsumexp(-1)) < EXACT


def test_layernorm_and_gelu_references_against_autograd():
    for eps in (1e-6, 1e-5):
        x, gam, beta, dy, resid = R.ln_inputs(7, 36)
        xv, gv, bv = (t.double().requires_grad_(True) for t in (x, gam, beta))
        y = F.layer_norm(xv, (36,), gv, bv, eps)
        (y * dy.double()).sum().backward()
        f, b = R.layernorm(x, gam, beta, eps), R.layernorm_bwd(dy, x, gam, eps, resid)
        assert R.rel(f["y"], y) < EXACT and R.rel(b["dx"], xv.grad + resid.double()) < EXACT and R.rel(b["dg"], gv.grad) < EXACT and R.rel(b["db"], bv.grad) < EXACT
        assert R.rel(f["rstd"], (x.double().var(-1, unbiased=False) + eps).rsqrt()) < EXACT
    x, dy = R.gelu_inputs(257)
    xv = x.double().requires_grad_(True)
    y = F.gelu(xv, approximate="none")
    (y * dy.double()).sum().backward()
    assert R.rel(R.gelu(x), y) < EXACT and R.rel(R.gelu_grad(x, dy), xv.grad) < EXACT
    assert x.min() == -12 and x.max() == 12 and bool((x == 0).any()) and bool(((x == 0) & torch.signbit(x)).any())


def test_mae_row_references():
    g = R.gen(1)
    B, Lp, D, n = 3, 9, 8, 4
    restore, keep, mask = R.mae_ids(B, Lp, n)
    noise_rank = restore.long()
    assert torch.equal(mask, (noise_rank >= n).float()) and torch.equal(noise_rank.gather(1, keep.long()), torch.arange(n).expand(B, n))
    e, mtok, dpos = R.randn(g, B, n + 1, D).double(), R.randn(g, D).double(), R.randn(g, Lp + 1, D).double()
    want = torch.empty(B, Lp + 1, D, dtype=torch.float64)
    for b in range(B):                                           # position by position
        want[b, 0] = e[b, 0] + dpos[0]
        for l in range(Lp):
            r = int(restore[b, l])
            want[b, 1 + l] = (e[b, 1 + r] if r < n else mtok) + dpos[1 + l]
    assert torch.equal(R.unshuffle_fwd(e, mtok, dpos, restore), want)
    embed, cls, pos = R.randn(g, B, n, D), R.randn(g, D), R.randn(g, Lp + 1, D)
    t = R.tokens_fwd(embed, cls, pos, keep)
    assert torch.equal(t[1, 0], cls + pos[0]) and torch.equal(t[2, 3], embed[2, 2] + pos[1 + int(keep[2, 2])])
    assert torch.equal(R.tokens_fwd(embed, cls, pos, None)[0, 4], embed[0, 3] + pos[4])
    # patch gather: the rows times the Conv2d weight, flattened in its own order, are the convolution
    for S, p in R.GATHER_CASES:
        obs, W = R.randn(g, 2, 3, S, S).double(), R.randn(g, 5, 3, p, p).double()
        conv = F.conv2d(obs, W, stride=p).flatten(2).transpose(1, 2).reshape(-1, 5)
        Lp = (S // p) ** 2
        assert R.rel(R.patch_gather(obs, None, Lp, p) @ W.reshape(5, -1).t(), conv) < EXACT
        ids = torch.stack([torch.randperm(Lp, generator=g)[:Lp - 1] for _ in range(2)])
        assert torch.equal(R.patch_gather(obs, ids, Lp - 1, p).reshape(2, Lp - 1, -1), R.patch_gather(obs, None, Lp, p).reshape(2, Lp, -1).gather(1, ids[..., None].expand(2, Lp - 1, 3 * p * p)))
        assert R.rel(R.patch_gather(obs, None, Lp, p, "pqc"), R.patch_gather(obs, None, Lp, p)) > 100 * G.TOL          # (ph, pw, c) for (c, ph, pw)
        assert torch.equal(R.patch_gather(obs, None, Lp, p, "pqc").reshape(2, Lp, -1), R.patchify(obs, p))
    # the loss target is patchify's, the loss the mean over removed patches, its gradient autograd's
    for (S, p), B in ((c, b) for c in R.LOSS_CASES for b in (1, 3)):
        Lp = (S // p) ** 2
        obs, pred = torch.rand(B, 3, S, S, generator=g), R.randn(g, B, Lp, 3 * p * p)
        mask = R.mae_ids(B, Lp, Lp // 2)[2]
        pv = pred.double().requires_grad_(True)
        tgt = obs.double().reshape(B, 3, S // p, p, S // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, Lp, p * p * 3)
        loss = (((pv - tgt) ** 2).mean(-1) * mask).sum() / mask.sum()
        (0.37 * loss).backward()
        ref = R.mae_loss(pred, obs, mask, p, 0.37)
        assert R.rel(ref["loss"], loss) < EXACT and R.rel(ref["dpred"][:, 1:], pv.grad) < EXACT and bool((ref["dpred"][:, 0] == 0).all())
        assert (3 * p * p < 256) == ((S, p) in ((12, 2), (16, 4), (24, 8))) and (3 * p * p > 512) == ((S, p) == (64, 16))


# ---- the cases are what they are named
def test_every_dropout_case_keeps_and_drops_in_every_head():
    for B, S, d, h, p, seed in R.POOL_ATTN_CASES:
        if p:
            k = R.host_keep(seed, R.SITE, p, B * h * S * S).reshape(B * h, -1).mean(-1)
            assert bool(((k > 0) & (k < 1)).all()), (B, S, d, h, p)
    for B, S, d, h, p, seed, kind in R.FLASH_CASES:
        if p:
            k = R.host_keep(seed, R.SITE, p, B * h * S * S).reshape(B * h, -1).mean(-1)
            assert bool(((k > 0) & (k < 1)).all()), (B, S, d, h, p)
    n = 0
    for B, S, d, h, p, seed, kind, _ in R.CLS_CASES:
        if p:
            k = R.host_keep(seed, R.SITE, p, B * h * S * S)[R.cls_keep_index(B, S, h)].reshape(B * h, S)
            assert bool(((k.mean(-1) > 0) & (k.mean(-1) < 1)).all()), (B, S, d, h, p)
            n += 1
    assert n >= 20 and {c[5] > 2 ** 32 for c in R.FLASH_CASES if c[4]} == {True, False}


def test_ragged_cases_have_the_tails_they_name():
    assert any(h * S > 256 for _, S, _, h, _, _ in R.POOL_ATTN_CASES) and max(h * S for _, S, d, h, _, _ in R.POOL_ATTN_CASES if d == 64) == 256
    assert any(R.pool_attn_lds(S, d, h)[1] == 160 * 1024 for _, S, d, h, _, _ in R.POOL_ATTN_CASES)
    assert {hd for hd in (8, 16, 32, 64)} == {d // h for _, _, d, h, _, _ in R.POOL_ATTN_CASES if d == 64}
    S = set(c[1] for c in R.FLASH_CASES)
    assert {s % 8 for s in S} >= {0, 1, 7} and {s % 32 for s in S} >= {0, 1, 31} and {s % 128 for s in S} >= {0, 1, 127} and max(S) > 256
    assert {c[2] // c[3] for c in R.FLASH_CASES} == {16, 32, 48, 64} and {c[3] for c in R.FLASH_CASES} == {1, 3}
    # the CLS kernels: wave hg of four takes heads hg, hg + 4, ...: h = 1, 2, 3, 6 leave waves with 0, 1 or 2 heads
    assert {tuple(len(range(hg, h, 4)) for hg in range(4)) for _, h in R.CLS_DH} >= {(1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (2, 2, 1, 1), (4, 4, 4, 4)}
    for B, S, d, h, p, seed, kind, chunks in R.CLS_CASES:
        assert R.cls_nchunk(B, S)[0] == chunks
    assert {min(c[7], 3) for c in R.CLS_CASES} == {1, 2, 3} and R.cls_nchunk(2, 65) == (2, 64) and R.cls_nchunk(2, 129) == (3, 64)
    assert {(F_ // 4) % 64 for F_ in R.LN_F} >= {0, 1, 63} and max(R.LN_F) == 1024 and {r % 4 for r in R.LN_R} == {0, 1, 3}
    for kind in ("wide",):
        for hd in (16, 32, 48, 64):
            qkv, _ = R.attn_inputs(2, 40, 3 * hd, 3, kind)
            s = R.attention(qkv, 2, 40, 3 * hd, 3)["s"]
            rest = torch.cat([s[..., :R.WIDE_KEY], s[..., R.WIDE_KEY + 1:]], -1)
            assert bool((s[..., R.WIDE_KEY] < -0.9e6).all()) and rest.max() > 35 and rest.min() < -35, (hd, rest.max(), rest.min())
        i = R.cls_inputs(2, 129, 128, 8, kind)
        s = R.cls_attn(*i[:4], 2, 129, 128, 8)["s"]
        assert s.max() > 35 and s.min() < -35


def test_wrong_restatements_move_the_outputs_by_100_tolerances():
    far = 100 * G.TOL
    B, S, d, h = 2, 33, 96, 3
    qkv, dO = R.attn_inputs(B, S, d, h)
    ref = R.attention(qkv, B, S, d, h, dO=dO)
    for wrong in (R.attention(qkv, B, S, d, h, dO=dO, scale=1.0), R.attention(qkv, B, S, d, h, dO=dO, head_perm=[1, 2, 0])):
        assert all(R.rel(wrong[n], ref[n]) > far for n in ("O", "lse", "dq", "dk", "dv"))
    p, n = 0.1, B * h * S * S
    keep = R.host_keep(R.SEED_LO, R.SITE, p, n)
    ref = R.attention(qkv, B, S, d, h, keep, p, dO)
    idx = torch.arange(n)
    rowstart = (idx // S) * S                                    # `key & 3` from the row start: element (row start & ~3) + (key & 3) + (key & ~3)
    wrong_idx = (rowstart // 4) * 4 + (idx - rowstart)
    wrong_keep = R.host_keep(R.SEED_LO, R.SITE, p, n + 4)[wrong_idx]
    assert not torch.equal(wrong_keep, keep)
    for wrong in (R.attention(qkv, B, S, d, h, wrong_keep, p, dO), R.attention(qkv, B, S, d, h, keep * (1 - p), p, dO)):          # and 1 / (1 - p) missing
        assert all(R.rel(wrong[n_], ref[n_]) > far for n_ in ("O", "dq", "dk", "dv"))
    i = R.cls_inputs(2, 65, 192, 6)
    ref, wrong = R.cls_attn(*i[:4], 2, 65, 192, 6, dO=i[4]), R.cls_attn(*i[:4], 2, 65, 192, 6, dO=i[4], bv_term=False)
    assert R.rel(wrong["o"], ref["o"]) > far
    for kind, F_ in R.LN_HARD:                                   # exactly what test_layernorm_hard_rows hands the kernels, at both eps
        if kind in ("small", "const"):
            x, gam, beta, dy, _ = R.ln_inputs(5, F_, kind)
            for eps, other in ((1e-6, 1e-5), (1e-5, 1e-6)):
                assert R.rel(R.layernorm(x, gam, beta, other)["y"], R.layernorm(x, gam, beta, eps)["y"]) > far or kind == "const"
                assert R.rel(R.layernorm(x, gam, beta, other)["rstd"], R.layernorm(x, gam, beta, eps)["rstd"]) > far
                assert R.rel(R.layernorm_bwd(dy, x, gam, other)["dx"], R.layernorm_bwd(dy, x, gam, eps)["dx"]) > far


# ---- the conditions the GPU bars rest on
def test_fp32_floors():
    """The reference's formulas in fp32 (torch, CPU) against fp64, per input set and output.  Where the GPU test applies plain TOL the
    formulas themselves must hold TOL / 4 in fp32, or TOL would not be a fair bar; an output above that must stand in G.FLOORS within a
    factor 1.5 of this measurement, and its bar is then 4 x floor."""
    seen = set()
    for key, outs in R.floor_cases():
        for n, (hi, lo) in outs.items():
            assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())
            v = R.rel(lo, hi)
            if (key, n) in G.FLOORS:
                t = G.FLOORS[(key, n)]
                seen.add((key, n))
                assert 4 * t > G.TOL and t / 1.5 <= v <= 1.5 * t, (key, n, v, t)
                assert G.bar_of(key, n) == 4 * t
            else:
                assert v <= G.TOL / 4, (key, n, v)
                assert G.bar_of(key, n) == G.TOL
    assert seen == set(G.FLOORS)
