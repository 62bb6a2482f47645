"""The north-star kernel on its own: ocrl_slot_attention_fwd/bwd (C ABI) against the oracle's slot_attention
(ocrs/common/slot_attn.py:47-102 restated in oracle/slate_oracle.py) evaluated in float64 under autograd; cases, reference and grader in
tests/slot_attn_ref.py (proved sound on the CPU by tests/test_slot_attn_ref_cpu.py).  Every slot count 1..16, every soft-max column count
of the streaming kernels 2..16, 1..16 attention heads through ocrl_slot_attention_mh_fwd/bwd, one to three iterations (the four backward
streaming variants), N from 1 to 8200 (ragged tiles, fewer tiles than waves, several workgroups per image), slot / MLP widths 64..256 on
both sides of the LDS limit of the grouped form, and the development forms OCRL_SA_FWD=1 / OCRL_SA_BWD=1 / OCRL_SA_GROUP=0 in processes
of their own.  Outputs and workspace hold NaN before every forward call."""
import json
import os
import sys

import pytest
import torch

from tests import slot_attn_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_and_grade(c, tag=""):
    pr = R.prepare(c)
    got = R.run_kernel(c, pr.inputs)
    p = R.plan(c.K, c.D, c.H, c.heads)
    e = R.grade(c, got, tag=tag + f"G{p['G']} NB{p['NB']} KS{p['KS']} ", log=log)
    return got, e, p


# the last four single-head shapes take the split forward (several workgroups per image, one launch per iteration): 4, 8, 16 and 8 workgroups per image
@pytest.mark.parametrize("B,N,K,D,H,I,NH", [(3, 200, 5, 128, 192, 3, 1), (2, 1024, 6, 192, 192, 3, 1), (2, 77, 16, 64, 64, 2, 1), (1, 16, 1, 256, 256, 1, 1),
                                            (2, 300, 11, 192, 128, 2, 1), (3, 2100, 6, 192, 192, 3, 1), (2, 4099, 16, 64, 64, 2, 1), (2, 8200, 11, 192, 128, 2, 1),
                                            (1, 4096, 1, 128, 64, 3, 1),
                                            # several heads: 12, 12, 16, 16 and 15 soft-max columns; head widths 96, 32, 16, 96, 64
                                            (2, 1024, 6, 192, 192, 3, 2), (3, 200, 3, 128, 192, 3, 4), (2, 4099, 4, 64, 64, 2, 4), (1, 2100, 8, 192, 128, 2, 2),
                                            (2, 300, 5, 192, 192, 3, 3)])
def test_slot_attention_unit(B, N, K, D, H, I, NH):
    c = R.Case(B, N, K, D, H, I, NH)
    assert c in R.EXISTING
    run_and_grade(c, "unit ")


@pytest.mark.parametrize("c", R.NEW, ids=R.case_id)
def test_slot_attention_case(c):
    got, _, p = run_and_grade(c)
    if c in R.SET_A or c in R.SET_E:
        d, (b, n) = R.attn_sum_error(got["attn"])
        assert d < R.ATTN_SUM_TOL, f"{R.case_id(c)}: attn of image {b}, position {n} sums to 1 + {d:.2e} over the slots"
    if c.heads > 1:
        assert (p["G"], p["KS"]) == (1, c.heads * c.K)


def test_set_d_runs_both_forms_at_every_slot_count():
    for K in R.KS_D:
        forms = {R.plan(c.K, c.D, c.H, 1)["G"] for c in R.SET_D if c.K == K}
        assert forms == {1, 16 // K}, (K, forms)


# ---- properties at set A's shape
def _a(K):
    c = R.SET_A[K - 1]
    assert c.K == K
    return c


def _rel(a, b, den):
    return float((a.double() - b.double()).abs().max()) / den


@pytest.mark.parametrize("K", R.PROPERTY_KS)
def test_slots_do_not_depend_on_the_attn_output(K):
    c = _a(K)
    pr = R.prepare(c)
    with_attn = R.run_kernel(c, pr.inputs, backward=False)
    without = R.run_kernel(c, pr.inputs, want_attn=False, backward=False)
    assert torch.equal(with_attn["slots"], without["slots"])
    d, (b, n) = R.attn_sum_error(with_attn["attn"])
    assert d < R.ATTN_SUM_TOL, f"K {K}: attn of image {b}, position {n} sums to 1 + {d:.2e}"


@pytest.mark.parametrize("K", R.PROPERTY_KS)
def test_slot_permutation(K):
    """slots0 and dslots permuted along K: slots, dslots0 and the columns of attn follow, dx and the weight gradients stay -- what a
    slot-index mix-up in the uneven two-block split or in a padded row would break"""
    c = _a(K)
    pr = R.prepare(c)
    perm = [(5 * i + 3) % K for i in range(K)]
    assert sorted(perm) == list(range(K)) and perm != list(range(K))
    P, x, s0, dsl = pr.inputs
    base = R.run_kernel(c, pr.inputs)
    got = R.run_kernel(c, (P, x, s0[:, perm].contiguous(), dsl[:, perm].contiguous()))
    ref = pr.ref
    want = dict(slots=base["slots"][:, perm], attn=base["attn"][..., perm], dx=base["dx"], dslots0=base["dslots0"][:, perm])
    ref_p = dict(slots=ref["slots"][:, perm], attn=ref["attn"][..., perm], dx=ref["dx"], dslots0=ref["dslots0"][:, perm], grads=ref["grads"])
    # against the permuted run of the kernel itself ...
    err = {k: _rel(got[k], want[k], float(ref[k].abs().max())) for k in R.TENSORS}
    gm, zero = R.gmax_of(ref), R.zero_class(ref)
    for n in R.NAMES:
        if n not in zero:         # (an identically zero gradient is rounding residue in both runs: graded below)
            err[n] = _rel(got["grads"][n], base["grads"][n], max(float(ref["grads"][n].abs().max()), R.GRAD_FLOOR * gm))
    worst = max(err, key=err.get)
    log(f"[slot_attention permutation K{K}] " + " ".join(f"{k}={err[k]:.2e}" for k in R.TENSORS) + f" worst {worst}={err[worst]:.2e}")
    assert err[worst] < R.TOL, err
    # ... and against the permuted fp64 reference, with the grader
    R.check(c, R.errors(c, ref_p, got, R.cpu32(c)), tag="permuted ")


@pytest.mark.parametrize("K", R.PROPERTY_KS)
def test_image_independence(K):
    """every image of the batched call (full groups and the group of one image) equals, bit for bit, the same image run alone: N = 261
    gives both calls two streaming workgroups per image, so the partial sums group alike"""
    c = _a(K)
    pr = R.prepare(c)
    P, x, s0, dsl = pr.inputs
    base = R.run_kernel(c, pr.inputs)
    c1 = c._replace(B=1)
    for b in range(c.B):
        one = R.run_kernel(c1, (P, x[b:b + 1], s0[b:b + 1], dsl[b:b + 1]))
        for k in R.TENSORS:
            assert torch.equal(one[k][0], base[k][b]), \
                f"K {K}: {k} of image {b} differs between the batch of {c.B} and the image alone by {float((one[k][0] - base[k][b]).abs().max()):.2e}"


# ---- the unit entry point against the model: one host description of the module (csrc/slot_attn_host.h) behind both
@pytest.mark.parametrize("name", ["SMALL", "K11", "HEADS2"])      # one group form, the uneven two-block split, two heads
def test_unit_entry_equals_the_model(name):
    """the engine's encode(), then ocrl_slot_attention_mh_fwd on the model's own sa_inputs / slots0 and its 17 weights: the same pack
    table, arguments and kernels (the model only issues the preparation launch ahead of the rest), so slots and attn are equal bit for bit"""
    from oracle import slate_oracle as O
    from ocrl_amd import _lib
    from tests import test_gpu_slate as S
    from tests.gpu_util import load_params
    cfg = O.default_cfg(**getattr(S, name))
    B, N, K, D, H, I, NH = 3, cfg.obs_size ** 2, cfg.num_slots, cfg.slot_size, cfg.mlp_hidden, cfg.num_iterations, int(getattr(cfg, "num_slot_heads", 1))
    eng = S.make_engine(cfg, B)
    load_params(eng, O.formula_params(cfg))
    eng.encode(torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(11)).cuda(), seed=7)
    torch.cuda.synchronize()
    x, s0 = eng.tensor("sa_inputs", (B, N, R.C)), eng.tensor("slots0", (B, K, D))
    w = [eng.param(R.PRE + n) for n in R.NAMES]
    assert [tuple(t.shape) for t in w] == R.shapes(D, H)
    L, p = _lib.lib(), _lib.ptr
    nan = lambda *shp: torch.full(shp, float("nan"), device="cuda")
    slots, attn = nan(B, K, D), nan(B, N, K)
    nws = L.ocrl_slot_attention_mh_ws_floats(B, N, K, D, H, I, NH)
    ws = nan(nws)
    _lib.check(L.ocrl_slot_attention_mh_fwd(p(x), p(s0), _lib.ptrs(w), p(slots), p(attn), B, N, K, D, H, I, NH, p(ws), nws, None))
    torch.cuda.synchronize()
    for k, got, want in (("slots", slots, eng.tensor("slots", (B, K, D))), ("attn", attn, eng.tensor("attn", (B, N, K)))):
        log(f"[slot_attention unit == model {name}] {k} max |difference| {float((got - want).abs().max()):.2e}")
        assert torch.equal(got, want), f"{name}: {k} of the unit entry point differs from the model's"


# ---- the development forms, one fresh process each (the knobs are read once per process)
SETTINGS = [("fwd1-bwd1", dict(OCRL_SA_FWD="1", OCRL_SA_BWD="1")), ("group0", dict(OCRL_SA_GROUP="0"))]


def test_development_forms(tmp_path, rank_launcher):
    for name, env in SETTINGS:          # one after the other; a child that exits abnormally ends the test before the next one starts
        out = os.path.join(str(tmp_path), name + ".json")
        rcs = rank_launcher.run([sys.executable, os.path.join(ROOT, "tests", "sa_variant_worker.py"), out], world=1, env=env, timeout=300)
        assert rcs == [0], f"{name}: worker exit status {rcs}"
        with open(out) as f:
            res = json.load(f)
        assert res["env"] == env and [r["case"] for r in res["cases"]] == [list(c) for c in R.SET_A]
        for r in res["cases"]:
            c = R.Case(*r["case"])
            e = {k: tuple(v) for k, v in r["errors"].items()}
            assert set(e) == set(R.TENSORS) | set(R.NAMES)
            assert r["G"] == (1 if name == "group0" or c.K > 8 else 16 // c.K), (name, c, r["G"])
            R.check(c, e, tag=f"{name} G{r['G']} ", log=log, seed=r["seed"])
            assert r["attn_sum"] < R.ATTN_SUM_TOL
