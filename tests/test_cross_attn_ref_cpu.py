"""The fp64 cross-attention reference of the kernel tests (tests/cross_attn_ref.py) proved without a GPU, and the inputs and cases of
tests/test_gpu_cross_attention.py proved non-vacuous: the case table reaches every folded instantiation a legal model configuration can
reach (through ocrl_xattn_plan, the launcher's own rule) and every (MAXK, d/h) of the plain kernels; every dropout case drops and keeps
entries in every head; the soft-maxes are neither uniform nor saturated; and each deliberately wrong restatement of the operation
(cross_attn_ref.WRONG) moves the output it touches by more than 100 x the GPU test's tolerance at the very inputs that test runs."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import slate_oracle as O
from tests import cross_attn_ref as R
from tests.gpu_util import drop_thresh, dropout_keep, relerr

TOL = 2e-5                       # the kernel-level standard, tests/test_gpu_attention_edges.TOL
MOVED = 100 * TOL
_fid = lambda c: "B{}-T{}-K{}-d{}-h{}-p{}-seed{}".format(*c)


def _plan(K, d, h):
    from ocrl_amd import _lib
    out = (ctypes.c_int * 5)()
    assert _lib.lib().ocrl_xattn_plan(K, d, h, out) == 0
    return tuple(out)


def _masks(case, wrong=()):
    B, T, K, d, h, p, seed = case
    if p == 0:
        return None, None
    return R.keep_masks(seed, R.SITE_P, R.SITE_O, p, B, h, T, K, d, wrong)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("B,T,K,d,h,p", [(2, 5, 3, 64, 4, 0.0), (2, 7, 9, 64, 2, 0.5), (1, 4, 5, 32, 1, 0.1), (2, 3, 7, 48, 3, 0.1)])
def test_block_ref_matches_the_oracle_mha(B, T, K, d, h, p):
    inp = {k: v.double() for k, v in R.make_inputs(B, T, K, d, h).items()}
    kp, ko = R.keep_masks(R.SEED_HI, R.SITE_P, R.SITE_O, p, B, h, T, K, d) if p > 0 else (None, None)
    ref = R.block_ref(*R.weights_of(inp), h, kp, ko, p, inp["gd"])
    W = {"c.proj_q.weight": inp["Wq"], "c.proj_k.weight": inp["Wk"], "c.proj_v.weight": inp["Wv"], "c.proj_o.weight": inp["Wo"]}
    masks = None if p == 0 else {"m.attn": kp.double(), "m.out": ko.double()}
    x = inp["x"].clone().requires_grad_(True)
    branch = O.mha(W, "c.", x, inp["mem"], inp["mem"], h, False, masks, "m", float(np.float32(p)))
    assert torch.allclose(ref["y"], (inp["resid"] + branch).detach(), rtol=1e-12, atol=1e-12)
    # gd is the gradient wrt the branch before the output dropout: dy = gd / (keep_o / (1 - p)) where kept; compare through dy = ones * mask
    dy = torch.randn(B, T, d, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    branch.backward(dy)
    gd = dy if p == 0 else dy * ko.double() / (1.0 - float(np.float32(p)))
    ref2 = R.block_ref(*R.weights_of(inp), h, kp, ko, p, gd)
    assert torch.allclose(ref2["dx"], x.grad, rtol=1e-11, atol=1e-12)
    # the plain core on the reference's q, ck, cv is the same function: O = ao, and dO = d ao gives dq, d ck, d cv
    core = R.core_ref(ref2["q"], ref2["ck"], ref2["cv"], h, kp, p, ref2["dao"])
    for a, b in (("O", "ao"), ("P", "P"), ("dQ", "dq"), ("dKm", "dck"), ("dVm", "dcv")):
        assert torch.allclose(core[a], ref2[b], rtol=1e-11, atol=1e-12), a
    assert torch.allclose(ref2["dao"], gd @ inp["Wo"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", [(2, 5, 3, 64, 4, 0.1, R.SEED_LO), (2, 6, 9, 64, 2, 0.5, R.SEED_HI), (1, 4, 5, 64, 1, 0.0, 0), (2, 3, 16, 128, 4, 0.0, 0),
                                  (2, 4, 8, 64, 8, 0.0, 0)], ids=_fid)
def test_fold_ref_reproduces_block_ref(case):
    B, T, K, d, h, p, seed = case
    inp = {k: v.double() for k, v in R.make_inputs(B, T, K, d, h).items()}
    kp, ko = _masks(case)
    a = R.block_ref(*R.weights_of(inp), h, kp, ko, p, inp["gd"])
    b = R.block_ref(*R.weights_of(inp), h, kp, ko, p, inp["gd"], folded=True)
    for n in ("S", "out", "y", "P", "Pd"):
        assert torch.allclose(a[n], b[n], rtol=1e-12, atol=1e-12), n
    for n in ("dx", "dWq", "dWo", "dck", "dcv", "dS"):
        assert torch.allclose(a[n], b[n], rtol=1e-11, atol=1e-12), n
    Ab, Vo = R.fold_ref(a["ck"], a["cv"], inp["Wq"], inp["Wo"], h)
    KP = R.kp_of(K, h)
    assert Ab.shape == Vo.shape == (B, h * KP, d)
    pad = torch.ones(h, KP, dtype=torch.bool)
    pad[:, :K] = False
    assert (Ab[:, pad.reshape(-1)] == 0).all() and (Vo[:, pad.reshape(-1)] == 0).all()
    S = R.unfold_cols(inp["x"] @ Ab.transpose(1, 2), h, K).permute(0, 2, 1, 3)
    assert torch.allclose(S, a["S"], rtol=1e-12, atol=1e-12)
    # element by element: column head * KP + slot
    hd, k, e = h - 1, K - 1, 5
    dh = d // h
    want = dh ** -0.5 * (inp["Wq"][hd * dh:(hd + 1) * dh, e] * a["ck"][1 % B, k, hd * dh:(hd + 1) * dh]).sum()
    assert abs(Ab[1 % B, hd * KP + k, e] - want) < 1e-12
    want = (a["cv"][0, k, hd * dh:(hd + 1) * dh] * inp["Wo"][e, hd * dh:(hd + 1) * dh]).sum()
    assert abs(Vo[0, hd * KP + k, e] - want) < 1e-12


def test_keep_masks_follow_the_index_contracts():
    B, h, T, K, d, p = 2, 3, 5, 7, 12, 0.5
    kp, ko = R.keep_masks(R.SEED_HI, R.SITE_P, R.SITE_O, p, B, h, T, K, d)
    assert kp.shape == (B, h, T, K) and ko.shape == (B, T, d) and kp.dtype == ko.dtype == torch.bool
    for (b, hd, t, s) in ((0, 0, 0, 0), (1, 2, 4, 6), (1, 0, 3, 2), (0, 1, 2, 5)):
        i = ((b * h + hd) * T + t) * K + s
        assert bool(kp[b, hd, t, s]) == bool(dropout_keep(R.SEED_HI, R.SITE_P, p, np.array([i]))[0])
    for (b, t, o) in ((0, 0, 0), (1, 4, 11), (1, 2, 7)):
        assert bool(ko[b, t, o]) == bool(dropout_keep(R.SEED_HI, R.SITE_O, p, np.array([(b * T + t) * d + o]))[0])
    assert R.SEED_LO < 2 ** 32 < R.SEED_HI and R.SITE_P != R.SITE_O


# ------------------------------------------------------------------------------------------------ coverage of the case tables
def _reachable():
    """{(NM, NT, KP)} of every legal model configuration with a folded form, from the launcher's own rule"""
    out = set()
    for d in R.D_MODELS:
        for h in R.legal_heads(d):
            for K in range(1, 17):
                sup, KP, NC, NM, lds = _plan(K, d, h)
                if sup:
                    assert KP == R.kp_of(K, h) and NC == h * KP and NM == d // 16 and lds == (NC * (d + 4) + d * (NC + 4)) * 4
                    out.add((NM, NC // 16, KP))
    return out


def test_case_table_reaches_every_folded_instantiation():
    reach = _reachable()
    assert reach == {(4, 1, 8), (4, 2, 8), (4, 4, 8), (4, 1, 16), (4, 2, 16), (4, 4, 16),
                     (8, 1, 8), (8, 2, 8), (8, 4, 8), (8, 2, 16), (8, 4, 16),
                     (12, 2, 8), (12, 4, 8), (12, 4, 16),
                     (16, 2, 8), (16, 4, 8), (16, 4, 16)}
    covered, drop = set(), {}
    for (B, T, K, d, h, p, seed) in R.FOLDED_GRID:
        sup, KP, NC, NM, _ = _plan(K, d, h)
        assert sup and (B, T) == (2, 36), (K, d, h)
        assert K in R.slot_classes(h) and h in R.legal_heads(d)
        covered.add((NM, NC // 16, KP))
        drop.setdefault((NM, NC // 16, KP), set()).add(p > 0)
    assert covered == reach
    assert all(v == {True, False} for v in drop.values()), drop          # every instantiation runs with and without dropout
    for d in R.D_MODELS:                                                  # every (d, h) with a folded form runs all its slot classes
        for h in R.folded_heads(d):
            assert {c[2] for c in R.FOLDED_GRID if c[3:5] == (d, h)} == set(R.slot_classes(h))
    assert _plan(16, 256, 4) == (1, 16, 64, 16, 136192)                   # the largest dynamic-LDS request
    for c in R.all_folded_cases():
        assert _plan(c[2], c[3], c[4])[0] == 1, c
        assert c[5] == 0 or c[2] % 4 != 0, c                              # dropout only where K % 4 != 0
    assert {c[1] for c in R.FOLDED_SWEEP} == {1, 15, 16, 17, 36, 200} and {R.kp_of(c[2], c[4]) for c in R.FOLDED_SWEEP} == {8, 16}
    assert {(c[0], c[1]) for c in R.FOLDED_SWEEP} == set(R.SWEEP_T)
    seeds = {c[6] for c in R.all_folded_cases() if c[5] > 0}
    assert seeds == {R.SEED_LO, R.SEED_HI}
    for K, d, h in R.UNSUPPORTED:
        assert _plan(K, d, h) == (0, 0, 0, 0, 0), (K, d, h)
    from ocrl_amd import _lib
    assert b"no folded form" in _lib.lib().ocrl_last_error()
    assert _lib.lib().ocrl_xattn_plan(3, 192, 4, None) != 0 and b"null" in _lib.lib().ocrl_last_error()
    assert _lib.lib().ocrl_xattn_desc_size() == ctypes.sizeof(_lib.XattnDesc)


def test_case_table_covers_every_plain_kernel():
    want = {(mk, dh) for mk in (8, 16) for dh in (4, 8, 16, 24, 32, 48, 64)}
    for table in (R.PLAIN_GRID, R.PLAIN_LONG):
        got = {(8 if c[2] <= 8 else 16, c[3] // c[4]) for c in table}
        assert got == want
    assert {(c[0], c[1]) for c in R.PLAIN_LONG} == {(2, 300)} and {c[1] for c in R.PLAIN_SWEEP} == {1, 15, 16, 17}
    assert {c[4] for c in R.PLAIN_GRID} >= {3, 6, 12, 16, 8}              # the head counts the model sends to the plain kernels
    for c in R.all_plain_cases():
        assert c[5] == 0 or c[2] % 4 != 0, c
        assert c[3] % c[4] == 0 and (c[3] // c[4]) % 4 == 0 and c[3] // c[4] <= 64 and 1 <= c[2] <= 16
    assert {c[6] for c in R.all_plain_cases() if c[5] > 0} == {R.SEED_LO, R.SEED_HI}


def _dropout_cases():
    seen, out = set(), []
    for c in R.all_folded_cases() + R.all_plain_cases():
        if c[5] > 0 and c not in seen:
            seen.add(c)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _dropout_cases(), ids=_fid)
def test_dropout_cases_are_not_vacuous(case):
    B, T, K, d, h, p, seed = case
    kp, ko = _masks(case)
    both, share, z = R.non_vacuity(kp.transpose(0, 1).reshape(1, h, -1), p)           # per head, over images, tokens and slots
    assert both, "a head whose probabilities are all kept or all dropped"
    assert z < 5.0, (share, drop_thresh(p) / 65536.0, z)
    both, share, z = R.non_vacuity(ko.reshape(1, 1, -1), p)
    assert both and z < 5.0, (share, z)


# ------------------------------------------------------------------------------------------------ the inputs separate right from wrong
def _grid_ids(cases):
    return [_fid(c) for c in cases]


@pytest.mark.parametrize("case", R.FOLDED_GRID + R.FOLDED_SWEEP[:6] + R.SHARED, ids=_fid)
def test_wrong_restatements_move_the_folded_outputs(case):
    B, T, K, d, h, p, seed = case
    inp = R.make_inputs(B, T, K, d, h)
    KP = R.kp_of(K, h)
    kp, ko = _masks(case)
    ref = R.block_ref(*R.weights_of(inp), h, kp, ko, p)
    moved = {}

    def run(w):
        mp, mo = _masks(case, (w,))
        return R.block_ref(*R.weights_of(inp), h, mp, mo, p, wrong=(w,))
    if h > 1 and K < KP:
        Ab, Vo = R.fold_ref(ref["ck"], ref["cv"], inp["Wq"].double(), inp["Wo"].double(), h)
        Aw, Vw = R.fold_ref(ref["ck"], ref["cv"], inp["Wq"].double(), inp["Wo"].double(), h, wrong=("head_stride_K",))
        moved["head_stride_K"] = min(relerr(Aw, Ab), relerr(Vw, Vo))
    if K >= 2:
        moved["no_scale"] = relerr(run("no_scale")["P"], ref["P"])
    if K < KP:
        moved["padded_weight"] = relerr(run("padded_weight")["P"], ref["P"])
    if h > 1:
        moved["heads_permuted"] = relerr(run("heads_permuted")["y"], ref["y"])
    if p > 0:
        for w in ("mask_stride_4", "no_rescale", "sites_swapped"):
            o = run(w)
            moved[w] = min(relerr(o["Pd"], ref["Pd"]), relerr(o["y"], ref["y"]))
    bad = {k: v for k, v in moved.items() if not v > MOVED}
    assert not bad, bad
    # the soft-max is neither uniform nor saturated
    if K >= 3:
        plain = R.block_ref(*R.weights_of(inp), h)
        assert relerr(R.uniform_out(*R.weights_of(inp), h), plain["y"]) > 1e-2
        top = plain["P"].max(-1).values
        assert top.median() < 0.99 and top.min() < 0.9, (float(top.median()), float(top.min()))


def test_every_wrong_restatement_is_exercised_for_every_folded_instantiation():
    """which restatements can differ from the right one depends on the shape (a head stride needs two heads and K < KP, ...): over the
    grid, each one applies at least once in every instantiation where it can"""
    seen = {}
    for (B, T, K, d, h, p, seed) in R.FOLDED_GRID:
        KP = R.kp_of(K, h)
        s = seen.setdefault((d // 16, h * KP // 16, KP), set())
        s |= {"no_scale"} if K >= 2 else set()
        s |= {"padded_weight"} if K < KP else set()
        s |= {"head_stride_K"} if h > 1 and K < KP else set()
        s |= {"heads_permuted"} if h > 1 else set()
        s |= {"mask_stride_4", "no_rescale", "sites_swapped"} if p > 0 else set()
    for inst, s in seen.items():
        one_head = inst[1] == 1 and inst[2] == 16
        assert s == set(R.WRONG) - ({"head_stride_K", "heads_permuted"} if one_head else set()), (inst, s)


@pytest.mark.parametrize("case", R.PLAIN_GRID, ids=_fid)
def test_wrong_restatements_move_the_plain_outputs(case):
    B, T, K, d, h, p, seed = case
    inp = R.make_inputs(B, T, K, d, h)
    full = R.block_ref(*R.weights_of(inp), h)
    q, ck, cv = full["q"], full["ck"], full["cv"]
    kp, _ = _masks(case)
    ref = R.core_ref(q, ck, cv, h, kp, p)
    moved = {"no_scale": relerr(R.core_ref(q, ck, cv, h, kp, p, wrong=("no_scale",))["P"], ref["P"]),
             "heads_permuted": relerr(R.core_ref(q, ck, cv, h, kp, p, wrong=("heads_permuted",))["O"], ref["O"])}
    if p > 0:
        for w in ("mask_stride_4", "no_rescale", "sites_swapped"):
            moved[w] = relerr(R.core_ref(q, ck, cv, h, _masks(case, (w,))[0], p, wrong=(w,))["O"], ref["O"])
    bad = {k: v for k, v in moved.items() if not v > MOVED}
    assert not bad, bad
    top = ref["P"].max(-1).values
    assert relerr(R.core_ref(q * 0, ck, cv, h)["O"], R.core_ref(q, ck, cv, h)["O"]) > 1e-2 and top.median() < 0.99


@pytest.mark.parametrize("case", R.WIDE, ids=lambda c: "B{}-T{}-K{}-d{}-h{}".format(*c))
def test_wide_range_inputs_reach_the_range(case):
    B, T, K, d, h = case
    inp = R.make_wide_range_inputs(B, T, K, d, h)
    ref = R.block_ref(*R.weights_of(inp), h, gd=inp["gd"])
    S = ref["S"]
    assert S.max() > 40 and S.min() < -40 and S.abs().max() < 90, (float(S.min()), float(S.max()))
    assert (S.max(-1).values - S.min(-1).values).median() > 30                      # the range inside a row, not only across rows
    assert all(torch.isfinite(t).all() for t in ref.values())
    assert _plan(K, d, h)[0] == 1
