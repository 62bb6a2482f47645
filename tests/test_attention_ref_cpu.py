"""The fp64 attention reference of the kernel tests (tests/attention_ref.py) proved without a GPU, and the inputs of
tests/test_gpu_attention_edges.py proved non-vacuous: every dropout case drops and keeps entries inside every causal triangle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as R
from tests.gpu_util import drop_thresh, dropout_keep


@pytest.mark.parametrize("B,T,h,dh", [(2, 1, 2, 16), (2, 9, 3, 48), (1, 67, 2, 32), (2, 130, 2, 64)])
def test_reference_matches_sdpa_without_dropout(B, T, h, dh):
    q, k, v, dO = (t.double() for t in R.make_inputs(B, T, h, dh))
    ref = R.attention_ref(q, k, v, h, dO)
    x = [t.clone().requires_grad_(True) for t in (q, k, v)]
    Q, K, V = (t.view(B, T, h, dh).transpose(1, 2) for t in x)
    o = F.scaled_dot_product_attention(Q, K, V, is_causal=True).transpose(1, 2).reshape(B, T, h * dh)
    o.backward(dO)
    assert torch.allclose(ref["o"], o.detach(), rtol=1e-12, atol=1e-12)
    for name, t in zip(("dq", "dk", "dv"), x):
        assert torch.allclose(ref[name], t.grad, rtol=1e-11, atol=1e-11), name
    S = (Q.detach() * dh ** -0.5) @ K.detach().transpose(-1, -2)
    for t in (0, T // 2, T - 1):                               # lse of a row = logsumexp over its keys 0..t
        assert torch.allclose(ref["lse"][:, :, t], torch.logsumexp(S[:, :, t, :t + 1], -1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,T,h,dh,p", [(2, 7, 2, 16, 0.5), (1, 9, 3, 16, 0.1)])
def test_reference_matches_row_loop_with_mask(B, T, h, dh, p):
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    keep = R.keep_mask(R.SEED_HI, R.SITE_BLK, p, B, h, T)
    assert keep.any() and not keep[:, :, torch.tril(torch.ones(T, T, dtype=torch.bool))].all()
    ref = R.attention_ref(q, k, v, h, dO, keep, p)
    rows = R.attention_rows(q, k, v, h, dO, keep, p)
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert torch.allclose(ref[name], rows[name], rtol=1e-11, atol=1e-11), name
    # and the mask matters: without it the outputs differ
    assert not torch.allclose(ref["o"], R.attention_ref(q, k, v, h)["o"], atol=1e-3)


def test_keep_mask_follows_the_index_contract():
    """element (b, head, q, key) = flat index ((b*h + head)*T + q)*T4 + key; for T % 4 == 0 that is the dense [B,h,T,T] index"""
    B, h, p = 2, 3, 0.5
    for T in (8, 9):
        T4 = (T + 3) & ~3
        m = R.keep_mask(R.SEED_LO, R.SITE_POOL, p, B, h, T)
        assert m.shape == (B, h, T, T) and m.dtype == torch.bool
        for (b, hd, qq, key) in ((0, 0, 0, 0), (1, 2, T - 1, T - 1), (1, 0, 3, 2), (0, 1, 5, 7)):
            i = ((b * h + hd) * T + qq) * T4 + key
            assert bool(m[b, hd, qq, key]) == bool(dropout_keep(R.SEED_LO, R.SITE_POOL, p, np.array([i]))[0])
    dense = dropout_keep(R.SEED_LO, R.SITE_POOL, p, np.arange(B * h * 8 * 8)).reshape(B, h, 8, 8)
    assert np.array_equal(R.keep_mask(R.SEED_LO, R.SITE_POOL, p, B, h, 8).numpy(), dense)
    assert R.SEED_LO < 2 ** 32 < R.SEED_HI


def test_case_tables_cover_what_the_kernels_dispatch():
    assert {c[1] for c in R.LENGTH_CASES if c[3] == 48} == {1, 3, 9, 25, 63, 64, 65, 67, 127, 128, 129, 193, 260}
    for dh in (16, 32, 64):
        assert {c[1] for c in R.LENGTH_CASES if c[3] == dh} == {1, 65, 129}
    assert {(c[4], c[1]) for c in R.DROPOUT_CASES} == {(p, T) for p in (0.1, 0.5) for T in (16, 64, 68, 132, 200)}
    assert {c[3] for c in R.DROPOUT_CASES} == {16, 32, 48, 64}
    assert {c[6] for c in R.DROPOUT_CASES} == {R.SITE_BLK, R.SITE_POOL} and {c[5] for c in R.DROPOUT_CASES} == {R.SEED_LO, R.SEED_HI}
    assert [(c[1], c[4]) for c in R.ODD_DROPOUT_CASES] == [(9, 0.1), (25, 0.1), (67, 0.1)]
    for c in R.LENGTH_CASES + R.DROPOUT_CASES + R.ODD_DROPOUT_CASES + R.STRIDE_CASES + R.REPRO_CASES:
        assert c[0] <= 3 and c[2] <= 4


@pytest.mark.parametrize("case", R.all_dropout_cases(), ids=lambda c: "B{}-T{}-h{}-dh{}-p{}-seed{}-site{}".format(*c))
def test_dropout_cases_are_not_vacuous(case):
    B, T, h, dh, p, seed, site = case
    both, share, z = R.non_vacuity(R.keep_mask(seed, site, p, B, h, T), p)
    assert both, "an (image, head) whose causal triangle is all kept or all dropped"
    assert z < 5.0, (share, drop_thresh(p) / 65536.0, z)


def test_wide_range_inputs_reach_the_range():
    B, T, h, dh = 1, 200, 2, 48
    q, k, v, dO = R.make_wide_range_inputs(B, T, h, dh)
    Q, K = (t.double().view(B, T, h, dh).transpose(1, 2) for t in (q, k))
    S = (Q * dh ** -0.5) @ K.transpose(-1, -2)
    tri = torch.tril(torch.ones(T, T, dtype=torch.bool))
    planted = torch.zeros(T, T, dtype=torch.bool)
    planted[:, R.PLANT_KEY] = True
    body = S[:, :, tri & ~planted]
    assert body.max() > 50 and body.min() < -50 and body.abs().max() < 90
    assert (S[:, :, 1:, R.PLANT_KEY] < -0.9e6).all()                  # one very large negative logit in every row below the first
    ref = R.attention_ref(q, k, v, h, dO)
    assert all(torch.isfinite(t).all() for t in ref.values())
