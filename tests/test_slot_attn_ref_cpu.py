"""CPU-only: the cases, the reference and the grader of the slot-attention kernel tests (tests/slot_attn_ref.py) are sound before the GPU
suite uses them -- every case finds guarded inputs, the fp32 CPU restatement passes the grader against the fp64 reference, the grader
fails on the corruptions a wrong kernel would produce -- and ocrl_slot_attention_plan reports the geometry csrc/slot_attn.hip documents."""
import copy

import pytest
import torch

from tests import slot_attn_ref as R


def test_case_list():
    assert len(R.EXISTING) == 14 and len(R.NEW) == 76 and len(set(R.ALL)) == 90
    single = {c.K for c in R.ALL if c.heads == 1}
    assert single == set(range(1, 17))
    # the streaming kernels are instantiated per soft-max column count: the composite counts with heads, all of 1..16 at one head
    assert {c.heads * c.K for c in R.SET_E} == set(range(2, 17)) - {5, 7, 11, 13} and {c.heads for c in R.SET_E} == {2, 3, 4, 8, 16}
    assert {c.heads * c.K for c in R.SET_A + R.SET_E} == set(range(1, 17))
    # set A: K <= 8 runs one full group and a group of one image; three iterations reach the first / middle / final backward variants
    assert all(c.I == 3 and c.N == 261 and c.B == (16 // c.K + 1 if c.K <= 8 else 2) for c in R.SET_A)
    assert {(c.K, c.I) for c in R.SET_B} == {(K, I) for K in (2, 8, 9, 16) for I in (1, 2)}
    assert {c.N for c in R.SET_C} == {1, 15, 16, 17} and {c.K for c in R.SET_C} == {3, 10}
    assert set(R.PROPERTY_KS) <= {c.K for c in R.SET_A}


@pytest.mark.parametrize("c", R.ALL, ids=R.case_id)
def test_case_is_guarded_and_the_fp32_restatement_passes(c):
    pr = R.prepare(c)
    assert pr.tried <= R.MAX_SEEDS and pr.ref["min_pre"] >= R.RELU_GUARD
    ref, r32 = pr.ref, R.cpu32(c)
    assert R.zero_class(ref) == R.expected_zero(c)
    gm = R.gmax_of(ref)
    for n in R.expected_zero(c):      # the residue the zero-gradient bound is built from is rounding noise, not a gradient
        assert float(r32["grads"][n].abs().max()) <= 1e-6 * gm, (n, float(r32["grads"][n].abs().max()) / gm)
    e = R.grade(c, r32, tag="cpu fp32 ")
    assert max(e[k] for k in R.TENSORS) < R.TOL
    assert R.attn_sum_error(r32["attn"])[0] < R.ATTN_SUM_TOL


# ---- the grader has teeth: the fp32 restatement stands in for the kernel's outputs
TEETH_A = R.SET_A[12]                  # K = 13: two uneven row blocks
TEETH_H = R.SET_E[8 + 5 + 2]           # 4 heads, K = 3


def _stand_in(c):
    return copy.deepcopy(R.cpu32(c))


def test_grader_passes_the_uncorrupted_stand_in():
    assert TEETH_A.K == 13 and (TEETH_H.heads, TEETH_H.K) == (4, 3)
    R.grade(TEETH_A, _stand_in(TEETH_A))
    R.grade(TEETH_H, _stand_in(TEETH_H))


def test_grader_fails_a_slot_row_scaled_by_1e_4():
    """passes the former 1e-4 tolerance"""
    c, got = TEETH_A, _stand_in(TEETH_A)
    got["slots"][:, -1] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match=rf"slots error .* at slots\[image \d+, slot {c.K - 1}, column \d+\]"):
        R.grade(c, got)
    ref = R.prepare(c).ref["slots"]
    assert float((got["slots"].double() - ref).abs().max() / ref.abs().max()) < 1e-4


def test_grader_fails_dx_of_the_last_position_zeroed():
    c, got = TEETH_A, _stand_in(TEETH_A)
    got["dx"][:, -1] = 0.0
    with pytest.raises(AssertionError, match=rf"dx error .* at dx\[image \d+, position {c.N - 1}, channel \d+\]"):
        R.grade(c, got)


def test_grader_fails_the_last_head_of_project_k_scaled_by_1e_4():
    c, got = TEETH_H, _stand_in(TEETH_H)
    dh = c.D // c.heads
    got["grads"]["project_k.weight"][-dh:] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match=r"project_k\.weight error .* at project_k\.weight\[row (\d+), column \d+\]") as ei:
        R.grade(c, got)
    import re
    assert int(re.search(r"project_k\.weight\[row (\d+)", str(ei.value)).group(1)) >= c.D - dh


def test_grader_fails_two_attn_columns_swapped():
    for c in (TEETH_A, TEETH_H):
        got = _stand_in(c)
        got["attn"][..., [0, c.K - 1]] = got["attn"][..., [c.K - 1, 0]]
        with pytest.raises(AssertionError, match=r"attn error .* at attn\[image \d+, position \d+, slot \d+\]"):
            R.grade(c, got)
        assert R.attn_sum_error(got["attn"])[0] < R.ATTN_SUM_TOL         # the row sums cannot see this one


def test_grader_fails_non_finite_and_a_nonzero_zero_gradient():
    c, got = TEETH_A, _stand_in(TEETH_A)
    got["dslots0"][1, 2, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"dslots0 error inf .* at dslots0\[image 1, slot 2, column 3\]"):
        R.grade(c, got)
    got = _stand_in(c)
    got["grads"]["norm_slots.bias"][5] += 1e-6 * R.gmax_of(R.prepare(c).ref)
    with pytest.raises(AssertionError, match=r"norm_slots\.bias error .* at norm_slots\.bias\[row 5\]"):
        R.grade(c, got)


# ---- the plan query
SA_LDS_MAX = 160 * 1024 - 256


def _lds(K, G, D, H, NH=1):
    """the slot-side kernels' LDS maps (csrc/slot_attn.hip SaFwdLds / SaBwdLds), in bytes"""
    NB, KB = (2, (K + 1) // 2) if K > 8 else (1, G * K)
    KP = NB * KB
    fwd = KP * D + KB * D * 3 + KB * 3 * D * 2 + KB * H + NH * KP * 64 * 3 + 32
    bwd = KP * D * 2 + KB * D * 2 + KB * 3 * D * 2 + KB * H + NH * KP * 64 * 5 + 80 + 4 * D + 2 * 64
    return 4 * fwd, 4 * bwd


@pytest.mark.parametrize("D,H", [(64, 64)] + R.WIDTHS_D)
def test_plan_reports_the_documented_geometry(D, H):
    for K in range(1, 17):
        p = R.plan(K, D, H, 1)
        if K > 8:        # one image, two row blocks of (K + 1) / 2 rows
            want_g = 1
            assert (p["NB"], p["KB"]) == (2, (K + 1) // 2)
        else:            # 16 / K images fill the 16-row tile unless either direction's rows do not fit the LDS
            gm = 16 // K
            want_g = gm if max(_lds(K, gm, D, H)) <= SA_LDS_MAX else 1
            assert (p["NB"], p["KB"]) == (1, want_g * K)
        assert p["G"] == want_g and p["KS"] == K
        assert (p["lds_fwd"], p["lds_bwd"]) == _lds(K, want_g, D, H) and max(p["lds_fwd"], p["lds_bwd"]) <= SA_LDS_MAX
        if (D, H) == (64, 64):
            assert p["G"] == (16 // K if K <= 8 else 1)


def test_plan_flips_64_bytes_over_the_limit():
    """K = 2, D = 192: the grouped backward asks for 159,552 of 163,584 bytes at H = 192 and for 64 bytes too many at H = 256"""
    assert _lds(2, 8, 192, 192)[1] == 159552 and _lds(2, 8, 192, 256)[1] == SA_LDS_MAX + 64
    p = R.plan(2, 192, 192, 1)
    assert (p["G"], p["KB"], p["lds_bwd"]) == (8, 16, 159552)
    p = R.plan(2, 192, 256, 1)
    assert (p["G"], p["KB"]) == (1, 2) and p["lds_bwd"] == _lds(2, 1, 192, 256)[1]


def test_plan_of_the_head_splits():
    for c in R.SET_E:
        p = R.plan(c.K, c.D, c.H, c.heads)
        assert (p["G"], p["NB"], p["KB"], p["KS"]) == (1, 1, c.K, c.heads * c.K)
        assert (p["lds_fwd"], p["lds_bwd"]) == _lds(c.K, 1, c.D, c.H, c.heads)


def test_set_d_reaches_both_forms_at_every_slot_count():
    for K in R.KS_D:
        forms = {R.plan(c.K, c.D, c.H, 1)["G"] for c in R.SET_D if c.K == K}
        assert forms == {1, 16 // K}, (K, forms)


@pytest.mark.parametrize("K,D,H,heads", [(0, 64, 64, 1), (17, 64, 64, 1), (4, 96, 64, 1), (4, 320, 64, 1), (4, 64, 96, 1), (6, 192, 192, 3), (2, 128, 64, 9),
                                         (9, 64, 64, 2), (16, 64, 64, 2), (2, 192, 64, 8), (2, 64, 64, 8), (3, 64, 64, 0), (3, 64, 64, 5)])
def test_plan_refuses_what_the_launch_refuses(K, D, H, heads):
    import ctypes
    from ocrl_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 6)(*[-7] * 6)
    assert L.ocrl_slot_attention_plan(K, D, H, heads, ctypes.byref(out)) != 0
    msg = L.ocrl_last_error().decode()
    assert msg.startswith("slot_attn:") and len(msg) > 20
    with pytest.raises(RuntimeError, match="slot_attn"):
        R.plan(K, D, H, heads)
    assert L.ocrl_slot_attention_plan(4, 64, 64, 1, None) != 0 and b"null" in L.ocrl_last_error()
