"""What the SLATE token-path kernel tests rest on, without a GPU: the tenth header (include/ocrl_hip_slate_kernels.h) parses, binds and is
exported while the older tables stay as they were; every refusal its entry points make before a launch; the scratch rule of the
dictionary gradient; the references of tests/token_path_ref.py against themselves (analytic against autograd, an operator against its
transpose, torch's own attention); and the conditions the bars of tests/test_gpu_token_path_kernels.py rest on: what the soft-max
family's formulas lose when torch evaluates them in fp32, per input set and output, against the table of floors kept there; the top-two
gap of every row whose token is compared; and that an honest sample stays inside the statistical bounds."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from ocrl_amd import _abi, _lib
from tests import attention_ref
from tests import test_gpu_token_path_kernels as G
from tests import token_path_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is refused before any launch
EXACT = 1e-10                   # fp64 against fp64: the same operation written twice
FUNCTIONS = {"ocrl_tp_gumbel_softmax": 11, "ocrl_tp_softmax_bwd_rows": 6, "ocrl_tp_softmax_stat_combine": 16, "ocrl_tp_exp_rows": 6,
             "ocrl_tp_rowdot_bias64": 6, "ocrl_tp_embed_fwd": 11, "ocrl_tp_embed_bwd_ws_floats": 3, "ocrl_tp_embed_bwd": 12,
             "ocrl_tp_embed_step": 10, "ocrl_tp_dropout_apply": 7, "ocrl_tp_dropout_mask": 6, "ocrl_tp_colsum": 10, "ocrl_tp_mse": 11,
             "ocrl_tp_pixel_shuffle": 9, "ocrl_tp_nchw_to_nhwc8": 7, "ocrl_tp_patchify4": 6, "ocrl_tp_pad_cols": 8, "ocrl_tp_im2col5": 8,
             "ocrl_tp_unpack5": 5, "ocrl_tp_posmap": 6, "ocrl_tp_posgrid": 3, "ocrl_tp_onehot": 5, "ocrl_tp_slot_init": 8,
             "ocrl_tp_slot_init_bwd": 9, "ocrl_tp_argmax_pos": 8, "ocrl_tp_decode_attn": 9}


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_slate_kernels.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {} and abi.structs == {}
    assert set(_lib.ABI_SLATE_KERNELS.functions) == set(FUNCTIONS)
    L = _lib.lib()
    for n, k in FUNCTIONS.items():
        assert len(getattr(L, n).argtypes) == k, n                                         # the symbol is exported and bound
    assert all(getattr(L, n).restype is ctypes.c_size_t for n in FUNCTIONS if n.endswith("_ws_floats"))
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_SLATE_KERNELS_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                         # self-contained
    assert not any(n.startswith("ocrl_slate_") for n in FUNCTIONS)
    # the older tables are what they were: the additions are additive
    assert len(_lib.ABI.functions) == 146 and _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    older = (_lib.ABI, _lib.ABI_DQN, _lib.ABI_ROLLOUT, _lib.ABI_REPLAY, _lib.ABI_C51, _lib.ABI_NOISY, _lib.ABI_CLASSIFIER, _lib.ABI_IODINE, _lib.ABI_QR)
    assert [len(a.functions) for a in older] == [146, 9, 1, 8, 6, 5, 1, 21, 6]
    assert not any(set(FUNCTIONS) & set(a.functions) for a in older)
    mk = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    objs, hdrs = (re.search(rf"^{v} = (.*)$", mk, re.M).group(1).split() for v in ("OBJS", "HDRS"))
    assert "slate_kernels_unit.o" in objs and "../../include/ocrl_hip_slate_kernels.h" in hdrs


# ---- refusals before any launch
def refused(rc, *words):
    msg = _lib.lib().ocrl_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_arguments_are_checked_before_any_launch():
    L = _lib.lib()
    p, odd, big = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4), 1 << 40

    for V in (0, 128, 300, 4352):
        refused(L.ocrl_tp_gumbel_softmax(p, p, p, p, p, None, 2, V, 1.0, 0, None), "V % 256 == 0")
        refused(L.ocrl_tp_softmax_bwd_rows(p, p, 2, V, 1.0, None), "V % 256 == 0")
    refused(L.ocrl_tp_gumbel_softmax(p, p, p, p, p, None, 0, 256, 1.0, 0, None), "R")
    refused(L.ocrl_tp_gumbel_softmax(p, p, p, p, p, None, 2, 256, 0.0, 0, None), "tau")
    refused(L.ocrl_tp_gumbel_softmax(p, p, None, p, p, None, 2, 256, 1.0, 0, None), "both noise tensors")
    refused(L.ocrl_tp_gumbel_softmax(None, p, p, p, p, None, 2, 256, 1.0, 0, None), "null")
    refused(L.ocrl_tp_gumbel_softmax(p, p, p, p, None, None, 2, 256, 1.0, 0, None), "null")
    refused(L.ocrl_tp_softmax_bwd_rows(p, None, 2, 256, 1.0, None), "null")
    refused(L.ocrl_tp_softmax_bwd_rows(p, p, 0, 256, 1.0, None), "R")

    def comb(stat=p, nseg=4, R_=5, lse=p, hstat=p, hidx=p, tokens=p, pred=p, ldp=256, V=256, tok=p, out=p, ws=p, n=big):
        return L.ocrl_tp_softmax_stat_combine(stat, nseg, R_, lse, hstat, hidx, tokens, pred, ldp, V, tok, out, 1.0, ws, n, None)
    for nseg in (0, 65):
        refused(comb(nseg=nseg), "1 <= nseg <= 64")
    refused(comb(R_=0), "R"), refused(comb(stat=None), "null"), refused(comb(lse=None), "null")
    refused(comb(hidx=None), "hstat, hidx and tokens"), refused(comb(hstat=None), "hstat, hidx and tokens"), refused(comb(tokens=None), "hstat, hidx and tokens")
    refused(comb(tok=None), "pred, tok, out and ws"), refused(comb(out=None), "pred, tok, out and ws"), refused(comb(ws=None), "pred, tok, out and ws")
    refused(comb(ldp=255), "ldp >= V"), refused(comb(V=0), "ldp >= V")
    refused(comb(R_=33, n=2), "workspace too small")

    refused(L.ocrl_tp_exp_rows(p, p, p, 3, 6, None), "V % 4 == 0"), refused(L.ocrl_tp_exp_rows(p, p, p, 0, 8, None), "R >= 1")
    refused(L.ocrl_tp_exp_rows(p, None, p, 3, 8, None), "null"), refused(L.ocrl_tp_exp_rows(odd, p, p, 3, 8, None), "aligned")
    refused(L.ocrl_tp_exp_rows(p, p, odd, 3, 8, None), "aligned")
    refused(L.ocrl_tp_rowdot_bias64(p, p, p, 0, p, None), "R"), refused(L.ocrl_tp_rowdot_bias64(p, p, p, 3, None, None), "null")
    for a in ((odd, p, p), (p, odd, p), (p, p, odd)):
        refused(L.ocrl_tp_rowdot_bias64(*a, 3, p, None), "aligned")

    def efwd(tokens=p, dic=p, bos=p, pe=p, out=p, B=2, T=4, d=64, pr=0.0):
        return L.ocrl_tp_embed_fwd(tokens, dic, bos, pe, out, B, T, d, pr, 0, None)
    refused(efwd(d=6), "d % 4 == 0"), refused(efwd(B=0), "B, T, d >= 1"), refused(efwd(T=0), "B, T, d >= 1"), refused(efwd(d=0), "B, T, d >= 1")
    refused(efwd(pr=1.0), "0 <= p < 1"), refused(efwd(pr=-0.1), "0 <= p < 1"), refused(efwd(tokens=None), "null"), refused(efwd(bos=None), "null")
    for k in ("dic", "bos", "pe", "out"):
        refused(efwd(**{k: odd}), "aligned")

    def ebwd(g=p, tokens=p, ddict=p, B=2, T=4, V=8, d=64, pr=0.0, ws=p, n=big):
        return L.ocrl_tp_embed_bwd(g, tokens, ddict, B, T, V, d, pr, 0, ws, n, None)
    for d in (0, 6, 1028):
        refused(ebwd(d=d), "d % 4 == 0")
        assert L.ocrl_tp_embed_bwd_ws_floats(8, 8, d) == 0
    for V in (0, 16384):
        refused(ebwd(V=V), "V + 1 <= 16384")
        assert L.ocrl_tp_embed_bwd_ws_floats(8, V, 64) == 0
    assert L.ocrl_tp_embed_bwd_ws_floats(0, 8, 64) == 0 and L.ocrl_tp_embed_bwd_ws_floats(8, 16383, 1024) > 0
    refused(ebwd(B=0), "B, T >= 1"), refused(ebwd(pr=1.0), "0 <= p < 1"), refused(ebwd(g=None), "null"), refused(ebwd(ws=None), "null")
    refused(ebwd(ddict=None), "null"), refused(ebwd(g=odd), "aligned"), refused(ebwd(ws=odd), "aligned")
    refused(ebwd(n=L.ocrl_tp_embed_bwd_ws_floats(8, 8, 64) - 1), "workspace too small")
    refused(L.ocrl_tp_embed_step(p, p, p, p, p, 2, 4, 64, 4, None), "0 <= t < T"), refused(L.ocrl_tp_embed_step(p, p, p, p, p, 2, 4, 64, -1, None), "0 <= t < T")
    refused(L.ocrl_tp_embed_step(p, p, p, p, None, 2, 4, 64, 0, None), "null"), refused(L.ocrl_tp_embed_step(p, p, p, p, p, 0, 4, 64, 0, None), "B, T, d >= 1")

    refused(L.ocrl_tp_dropout_apply(p, p, 6, 0.1, 0, 1, None), "n % 4 == 0"), refused(L.ocrl_tp_dropout_apply(p, p, 0, 0.1, 0, 1, None), "n % 4 == 0")
    refused(L.ocrl_tp_dropout_apply(p, p, 8, 1.0, 0, 1, None), "0 <= p < 1"), refused(L.ocrl_tp_dropout_apply(p, None, 8, 0.1, 0, 1, None), "null")
    refused(L.ocrl_tp_dropout_apply(odd, p, 8, 0.1, 0, 1, None), "aligned"), refused(L.ocrl_tp_dropout_apply(p, odd, 8, 0.1, 0, 1, None), "aligned")
    refused(L.ocrl_tp_dropout_mask(p, 1, 0, 0.1, 0, None), "n"), refused(L.ocrl_tp_dropout_mask(None, 1, 8, 0.1, 0, None), "null")
    refused(L.ocrl_tp_dropout_mask(p, 1, 8, 1.5, 0, None), "0 <= p < 1")

    refused(L.ocrl_tp_colsum(p, 63, p, 5, 64, 0, 1.0, p, big, None), "ld >= F"), refused(L.ocrl_tp_colsum(p, 64, p, 5, 64, 0, 1.0, odd, big, None), "aligned")
    refused(L.ocrl_tp_colsum(p, 64, p, 0, 64, 0, 1.0, p, big, None), "R"), refused(L.ocrl_tp_colsum(p, 64, p, 5, 0, 0, 1.0, p, big, None), "F")
    refused(L.ocrl_tp_colsum(None, 64, p, 5, 64, 0, 1.0, p, big, None), "null"), refused(L.ocrl_tp_colsum(p, 64, p, 5, 64, 0, 1.0, None, big, None), "null")
    refused(L.ocrl_tp_colsum(p, 64, p, 2048, 64, 0, 1.0, p, 15 * 64, None), "workspace too small")          # the launcher's own refusal
    refused(L.ocrl_tp_colsum(p, 3, p, 5, 3, 0, 1.0, p, 2, None), "workspace too small")

    def mse(obs=p, recon=p, drecon=p, out=p, B=2, C=3, H=8, W=8, ws=p, n=1024):
        return L.ocrl_tp_mse(obs, recon, drecon, out, B, C, H, W, ws, n, None)
    refused(mse(C=5), "C <= 4"), refused(mse(C=0), "C <= 4"), refused(mse(n=1023), "workspace too small"), refused(mse(B=0), "B, H, W >= 1")
    refused(mse(obs=None), "null"), refused(mse(ws=None), "null"), refused(mse(recon=odd), "aligned"), refused(mse(drecon=odd), "aligned")

    refused(L.ocrl_tp_pixel_shuffle(p, p, 2, 0, 4, 3, 1, None, None), "B, h, w, Cout >= 1"), refused(L.ocrl_tp_pixel_shuffle(p, None, 2, 4, 4, 3, 1, None, None), "null")
    refused(L.ocrl_tp_pixel_shuffle(p, p, 2, 4, 4, 3, 1, p, None), "mask")
    for a in ((odd, p, None), (p, odd, None), (p, p, odd)):
        refused(L.ocrl_tp_pixel_shuffle(a[0], a[1], 2, 4, 4, 3, 0, a[2], None), "aligned")
    refused(L.ocrl_tp_nchw_to_nhwc8(p, p, 2, 9, 4, 4, None), "C <= 8"), refused(L.ocrl_tp_nchw_to_nhwc8(p, p, 2, 0, 4, 4, None), "C <= 8")
    refused(L.ocrl_tp_nchw_to_nhwc8(p, odd, 2, 3, 4, 4, None), "aligned"), refused(L.ocrl_tp_nchw_to_nhwc8(None, p, 2, 3, 4, 4, None), "null")
    refused(L.ocrl_tp_patchify4(p, p, 2, 3, 6, None), "S % 4 == 0"), refused(L.ocrl_tp_patchify4(p, p, 2, 3, 0, None), "S % 4 == 0")
    refused(L.ocrl_tp_patchify4(odd, p, 2, 3, 8, None), "aligned"), refused(L.ocrl_tp_patchify4(p, odd, 2, 3, 8, None), "aligned")
    refused(L.ocrl_tp_pad_cols(p, 19, p, 23, 5, 19, 24, None), "ldo >= Cout"), refused(L.ocrl_tp_pad_cols(p, 18, p, 24, 5, 19, 24, None), "ldi >= C")
    refused(L.ocrl_tp_pad_cols(p, 19, p, 24, 0, 19, 24, None), "R"), refused(L.ocrl_tp_pad_cols(p, 19, None, 24, 5, 19, 24, None), "null")
    refused(L.ocrl_tp_im2col5(p, p, 2, 6, 9, 3, 74, None), "ldc >= 25 C"), refused(L.ocrl_tp_im2col5(p, p, 2, 6, 9, 9, 400, None), "C <= 8")
    refused(L.ocrl_tp_im2col5(p, p, 0, 6, 9, 3, 76, None), "B, H, W >= 1"), refused(L.ocrl_tp_im2col5(p, None, 2, 6, 9, 3, 76, None), "null")
    refused(L.ocrl_tp_unpack5(p, p, 3, 74, None), "25 C <= ldc"), refused(L.ocrl_tp_unpack5(p, p, 9, 400, None), "C <= 8"), refused(L.ocrl_tp_unpack5(None, p, 3, 76, None), "null")
    refused(L.ocrl_tp_posmap(p, p, p, 0, 64, None), "S, C >= 1"), refused(L.ocrl_tp_posmap(p, None, p, 4, 64, None), "null")
    refused(L.ocrl_tp_posgrid(p, 0, None), "S"), refused(L.ocrl_tp_posgrid(None, 4, None), "null"), refused(L.ocrl_tp_posgrid(odd, 4, None), "aligned")
    refused(L.ocrl_tp_onehot(p, p, 0, 256, None), "rows, V >= 1"), refused(L.ocrl_tp_onehot(p, p, 5, 0, None), "rows, V >= 1"), refused(L.ocrl_tp_onehot(None, p, 5, 8, None), "null")
    refused(L.ocrl_tp_slot_init(p, p, None, p, 0, 64, 0, None), "BK, D >= 1"), refused(L.ocrl_tp_slot_init(p, None, None, p, 4, 64, 0, None), "null")
    refused(L.ocrl_tp_slot_init_bwd(p, p, None, p, p, 4, 0, 0, None), "BK, D >= 1"), refused(L.ocrl_tp_slot_init_bwd(p, p, None, None, p, 4, 64, 0, None), "null")
    refused(L.ocrl_tp_argmax_pos(p, p, 3, 5, 256, 5, 0, None), "0 <= t < T"), refused(L.ocrl_tp_argmax_pos(p, p, 3, 5, 256, -1, 1, None), "0 <= t < T")
    refused(L.ocrl_tp_argmax_pos(p, p, 3, 5, 0, 0, 0, None), "B, T, V >= 1"), refused(L.ocrl_tp_argmax_pos(p, None, 3, 5, 256, 0, 0, None), "null")

    def dec(qkv=p, out=p, B=2, T=16, t=3, d=192, h=4, ld=576):
        return L.ocrl_tp_decode_attn(qkv, out, B, T, t, d, h, ld, None)
    refused(dec(h=0), "B, T, d, h >= 1"), refused(dec(h=5), "d % h == 0"), refused(dec(d=24, h=4, ld=72), "multiple of 4"), refused(dec(d=192, h=2), "<= 64")
    refused(dec(t=16), "0 <= t < T"), refused(dec(t=-1), "0 <= t < T"), refused(dec(ld=575), "ld % 4 == 0"), refused(dec(ld=572), "ld >= 3 d")
    refused(dec(qkv=odd), "aligned"), refused(dec(out=None), "null"), refused(dec(T=20000, t=5), "sequence too long")


@pytest.mark.parametrize("BT,V,d", [(32, 8, 64), (640, 8, 64), (300, 4096, 192)])
def test_embed_bwd_scratch_is_the_launchers_formula(BT, V, d):
    """chunk histograms | totals | bases | sorted row list | unit partials, each rounded up to 64 floats"""
    al = lambda n: (n + 63) // 64 * 64
    nchunk, nunit = -(-BT // 512), -(-BT // 128)
    assert _lib.lib().ocrl_tp_embed_bwd_ws_floats(BT, V, d) == al(nchunk * (V + 1)) + 2 * al(V + 2) + al(BT) + al(nunit * 2 * d)


# ---- the references against themselves
def test_softmax_backward_analytic_against_autograd():
    z, d = R.softmax_bwd_inputs(3, 768)
    x = z.double().log().requires_grad_(True)
    z = torch.softmax(x, -1)                              # the fp32 rows do not sum to 1 to the last bit: take the soft-max autograd sees
    (z * d.double()).sum().backward()
    z = z.detach()
    assert R.rel(R.softmax_bwd_rows(z, d, 1.0), x.grad) < EXACT
    assert R.rel(R.softmax_bwd_rows(z, d, 0.37), x.grad * R.f32(0.37)) < EXACT


def test_gumbel_reference_is_the_oracles_and_the_tie_inputs_tie():
    raw, e1, e2 = R.gumbel_inputs("well", 5, 768)
    ref = R.gumbel_softmax(raw, e1, e2, 0.1)
    assert R.rel(ref["z"].sum(-1), torch.ones(5)) < EXACT and torch.equal(ref["zst"].round(), R.onehot(ref["z"].argmax(-1), 768).double())
    assert torch.equal(ref["z"].argmax(-1), ref["s1"].argmax(-1))
    for where, (a, b) in R.TIE_PAIRS.items():
        for V in (768, 4096):
            ref = R.gumbel_softmax(*R.gumbel_tie_inputs(where, V), 1.0)
            for s in (ref["s1"], ref["s2"]):
                assert torch.equal(s[:, a], s[:, b]) and bool((s[:, a] == s.max(-1).values).all()) and bool((s.argmax(-1) == a).all())
    assert R.TIE_PAIRS["thread"][1] - R.TIE_PAIRS["thread"][0] == 256 and R.TIE_PAIRS["waves"][0] // 64 != R.TIE_PAIRS["waves"][1] // 64


@pytest.mark.parametrize("nseg,Rr", R.STAT_CASES)
def test_segment_statistics_recombine_to_the_logsumexp(nseg, Rr):
    i = R.stat_inputs(nseg, Rr)
    m, s = i["stat"][..., 0].double(), i["stat"][..., 1].double()
    M = m.max(-1, keepdim=True).values
    lse = (M[:, 0] + (s * (m - M).exp()).sum(-1).log())
    assert R.rel(lse, R.stat_combine(i["scores"], i["pred"], i["tok"], 1.0)[0]) < 1e-6            # stat is rounded to fp32
    assert bool((i["tok"] >= 0).all()) and bool((i["tok"] < i["V"]).all()) and bool((i["hidx"] < i["V"]).all())
    if nseg == 6:
        assert bool((m[:, 5] == -math.inf).all()) and bool((s[:, 5] == 0).all()) and bool((i["hstat"][:, 5] == -math.inf).all())
    # the compared score is an fp32 input, so its error is zero: the rows only have to have one greatest value
    assert bool((R.top_two_gap(i["hard"]) > 0).all()) if i["V"] > 1 else True
    assert torch.equal(i["hidx"].long().gather(1, i["hstat"].argmax(-1, keepdim=True))[:, 0], i["hard"].argmax(-1))


def test_embed_bwd_is_the_gradient_of_embed_fwd():
    B, T, V, d = 3, 37, 8, 64
    tok, dic, bos, pe, g = R.embed_inputs(B, T, V, d)
    D = dic.double().requires_grad_(True)
    (R.embed_fwd(tok, D, bos, pe) * g.double()).sum().backward()
    assert R.rel(R.embed_bwd(g, tok, V), D.grad) < EXACT
    for t in (0, T - 1):
        assert torch.equal(R.embed_step(tok, dic, bos, pe, t), R.embed_fwd(tok, dic, bos, pe)[:, t])
    other = tok.clone()
    other[:, T - 1] = 0
    assert torch.equal(R.embed_fwd(other, dic, bos, pe), R.embed_fwd(tok, dic, bos, pe))
    # the named token sets are what the GPU test says they are
    assert bool((R.embed_inputs(5, 128, 8, 64, "const3")[0] == 3).all())
    assert torch.equal(R.embed_inputs(4, 129, 8, 64, "image")[0][:, 5], torch.arange(4, dtype=torch.int32))


def test_layout_references():
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(2, 3, 5, 12, generator=g).double(), torch.randn(2, 6, 10, 3, generator=g).double()
    assert abs((R.pixel_shuffle(x) * y).sum().item() - (x * R.pixel_unshuffle(y)).sum().item()) < EXACT * (x.abs().sum().item())     # transpose
    assert torch.equal(R.pixel_unshuffle(R.pixel_shuffle(x)), x)
    assert R.pixel_shuffle(x)[1, 2 * 2 + 1, 2 * 4 + 0, 2] == x[1, 2, 4, 4 * 2 + 2 * 1 + 0]
    img = torch.randn(2, 3, 8, 8, generator=g)
    W = torch.randn(64, 3, 4, 4, generator=g)
    conv = F.conv2d(img, W, stride=4).permute(0, 2, 3, 1).reshape(-1, 64)
    assert R.rel(R.patchify4(img).double() @ W.reshape(64, -1).double().t(), conv) < 1e-5
    x8 = torch.randn(2, 6, 9, 8, generator=g).double()
    W5 = torch.randn(64, 3, 5, 5, generator=g).double()
    col = R.im2col5(x8, 3, 80)
    Wp = F.pad(W5.permute(0, 2, 3, 1).reshape(64, 75), (0, 5))
    assert R.rel(col @ Wp.t(), F.conv2d(x8[..., :3].permute(0, 3, 1, 2), W5, padding=2).permute(0, 2, 3, 1).reshape(-1, 64)) < EXACT
    assert bool((col[:, 75:] == 0).all()) and torch.equal(R.unpack5(Wp, 3), W5)
    assert torch.equal(R.posgrid(1), torch.tensor([[1.0, 0.0, 1.0, 0.0]])) and torch.equal(R.posgrid(2)[3], torch.tensor([0.0, 1.0, 0.0, 1.0]))
    Wpos, bpos = torch.randn(64, 4, generator=g), torch.randn(64, generator=g)
    assert R.rel(R.posmap(Wpos, bpos, 16).reshape(256, 64), F.linear(R.posgrid(16).double(), Wpos.double(), bpos.double())) < EXACT


def test_slot_init_bwd_against_autograd():
    g = torch.Generator().manual_seed(1)
    mu, ls = torch.randn(100, generator=g).double().requires_grad_(True), torch.randn(100, generator=g).double().requires_grad_(True)
    eps, d = torch.randn(33, 100, generator=g), torch.randn(33, 100, generator=g)
    (R.slot_init(mu, ls, eps) * d.double()).sum().backward()
    dmu, dls = R.slot_init_bwd(d, ls.detach(), eps)
    assert R.rel(dmu, mu.grad) < EXACT and R.rel(dls, ls.grad) < EXACT


@pytest.mark.parametrize("case", R.DECODE_CASES)
def test_decode_attn_is_a_row_of_torchs_attention(case):
    B, T, d, h, ld = case
    x = R.decode_inputs(case).double()
    q, k, v = (x[..., i * d:(i + 1) * d].reshape(B, T, h, d // h).transpose(1, 2) for i in range(3))
    full = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, T, d)
    mine = attention_ref.attention_ref(x[..., :d], x[..., d:2 * d], x[..., 2 * d:3 * d], h)["o"]
    for t in R.decode_ts(case):
        assert R.rel(R.decode_attn(x, t, d, h), full[:, t]) < EXACT and R.rel(R.decode_attn(x, t, d, h), mine[:, t]) < EXACT


# ---- the conditions the GPU bars rest on
def test_fp32_floors_of_the_softmax_family():
    """The reference's formulas in fp32 (torch, CPU) against fp64, per input set and output.  Where the GPU test applies plain TOL the
    formulas themselves must hold TOL / 4 in fp32, or TOL would not be a fair bar; an output above that must stand in G.FLOORS within a
    factor 1.5 of this measurement, and its bar is then max(TOL, 4 x floor)."""
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


@pytest.mark.parametrize("kind,Rr,V,tau", R.GUMBEL_CASES)
def test_token_rows_are_decided_by_100_times_the_fp32_error(kind, Rr, V, tau):
    """tokens = argmax(logp + g2) and the straight-through index = argmax(logp + g1): every row's fp64 top-two gap is at least 100 x the
    largest fp32-against-fp64 error of that score on this input set, so no rounding can change the answer"""
    inp = R.gumbel_inputs(kind, Rr, V)
    hi, lo = R.gumbel_softmax(*inp, tau), R.gumbel_softmax(*inp, tau, dtype=torch.float32)
    for s in ("s1", "s2"):
        e = (lo[s].double() - hi[s]).abs().max().item()
        assert R.top_two_gap(hi[s]).min().item() >= 100 * e, (s, R.top_two_gap(hi[s]).min().item(), e)


def test_argmax_inputs_have_one_greatest_value_and_ties_are_planted():
    hm, hidx, want = R.stat_tie(64, 33)
    top = hm.double().topk(2, -1)
    assert bool((top.values[:, 0] == top.values[:, 1]).all()) and bool((top.values[:, 0] == 7.5).all())
    assert torch.equal(want, torch.minimum(hidx.long().gather(1, top.indices[:, :1]), hidx.long().gather(1, top.indices[:, 1:]))[:, 0])


def test_honest_samples_stay_inside_the_statistical_bounds():
    g = torch.Generator().manual_seed(5)
    n, p = 1 << 20, 0.1
    keep = (torch.rand(n, generator=g) >= p).double()
    assert abs(keep.mean().item() - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n)
    n = 1 << 16
    eps = torch.randn(n, generator=g).double()
    assert abs(eps.mean().item()) < 5 / math.sqrt(n) and abs(eps.var().item() - 1) < 5 * math.sqrt(2 / n)
