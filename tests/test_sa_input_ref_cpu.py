"""CPU-only: the cases, the reference and the grader of the slot-attention input-chain tests (tests/sa_input_ref.py) are sound before the
GPU suite uses them -- every case finds guarded inputs, the fp32 CPU restatement passes the grader against the fp64 reference, and the
grader fails on the corruptions a wrong kernel would produce."""
import copy

import pytest
import torch

from tests import sa_input_ref as R


def test_case_list():
    t = R.plan(1000)["tile"]
    assert [c.name for c in R.cases()] == R.CASE_NAMES
    assert [c.R for c in R.cases()] == [1, t - 1, t, t + 1, 2 * t + 5, 1000, 5 * t]
    assert [c.max_wgs for c in R.cases()] == [0, 0, 0, 0, 0, 0, 2]
    assert t % 32 == 0 and R.plan(1000)["slab"] == 2 * 64 * 64 + 4 * 64
    assert R.plan(1)["wgs"] == 1 and R.plan(2 * t + 5)["wgs"] == 3           # one workgroup per tile while there are fewer tiles than workgroups


def test_plan_refuses_no_rows():
    from ocrl_amd import _lib
    assert _lib.lib().ocrl_sa_input_plan(0, None) != 0
    with pytest.raises(RuntimeError, match="sa_input"):
        R.plan(0)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_is_guarded_and_the_fp32_restatement_passes(name):
    c = R.case(name)
    pr = R.prepare(c)
    assert pr.tried <= R.MAX_SEEDS and pr.ref["min_pre"] >= R.RELU_GUARD
    inp = pr.inputs
    assert all(float(inp[k].abs().min()) > 0 for k in ("gamma", "beta", "b0", "b2"))
    assert not torch.equal(inp["W0"], inp["W0"].T) and not torch.equal(inp["W2"], inp["W2"].T)
    e = R.grade(pr.ref, R.cpu32(c), R.TOL, tag="cpu fp32 ")
    assert set(e) == set(R.QUANTITIES)


# ---- the grader has teeth: the fp32 restatement stands in for the kernel's outputs
TEETH = "2tile+5"


def _stand_in():
    c = R.case(TEETH)
    return c, R.prepare(c).ref, copy.deepcopy(R.cpu32(c))


def test_grader_fails_a_row_scaled_by_1e_4():
    for k in ("h1", "x", "de4"):
        c, ref, got = _stand_in()
        row = int(ref[k].abs().max(-1).values.argmax())          # the row that holds the tensor's maximum: the scaled error is 1e-4 of it
        got[k][row] *= 1.0 + 1e-4
        with pytest.raises(AssertionError, match=rf"{k} error .* at {k}\[{row}, \d+\]"):
            R.grade(ref, got, R.TOL)


def test_grader_fails_a_zeroed_last_row():
    for k in ("h1", "x", "de4"):
        c, ref, got = _stand_in()
        got[k][-1] = 0.0
        with pytest.raises(AssertionError, match=rf"{k} error .* at {k}\[{c.R - 1}, \d+\]"):
            R.grade(ref, got, R.TOL)
    c, ref, got = _stand_in()
    got["rstd"][-1] = 0.0
    with pytest.raises(AssertionError, match=rf"rstd error .* at rstd\[{c.R - 1}\]"):
        R.grade(ref, got, R.TOL)


def test_grader_fails_a_nan():
    for k in R.QUANTITIES:
        c, ref, got = _stand_in()
        got[k].view(-1)[3] = float("nan")
        with pytest.raises(AssertionError, match=rf"{k} error inf"):
            R.grade(ref, got, R.TOL)


def test_grader_fails_two_swapped_weight_gradient_rows():
    for k in ("dW0", "dW2"):
        c, ref, got = _stand_in()
        got[k][[0, 63]] = got[k][[63, 0]]
        with pytest.raises(AssertionError, match=rf"{k} error .* at {k}\[(0|63), \d+\]"):
            R.grade(ref, got, R.TOL)


def test_grader_holds_a_measured_bar_per_quantity():
    """the GPU suite's form: a bar per quantity, twice another fp32 evaluation's error; the stand-in passes, a corrupted one does not"""
    c, ref, got = _stand_in()
    bars = {k: 2.0 * v[0] for k, v in R.errors(ref, got).items()}
    R.grade(ref, got, bars)
    got["dbeta"][5] += 1e-4 * float(ref["dbeta"].abs().max())
    with pytest.raises(AssertionError, match=r"dbeta error .* at dbeta\[5\]"):
        R.grade(ref, got, bars)
