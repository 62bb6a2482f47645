"""CPU checks of the Transformer pooling head over long token sequences (a CNN feature map, ocrl_pool_transformer_long_*): the oracle
against the reference fixture at feature-map shapes, and the workspace contract (linear in the token count, no S^2 term)."""
import os

import numpy as np
import pytest
import torch

from oracle import pooling_oracle as PO
from tests.golden.make_golden_pooling_long import CASES, REP, cotangent, sample, tokens

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("tag,K,L,B", CASES)
def test_oracle_matches_reference_fixture(tag, K, L, B):
    fx = np.load(os.path.join(GOLD, "pooling_cnnfeat.npz"))
    rep, K_, d, nhead, L_, ff, has_pos, B_ = [int(v) for v in fx[tag + ":cfg"]]
    assert (rep, K_, L_, B_, has_pos) == (REP, K, L, B, 1)
    cfg = PO.default_cfg(rep_dim=rep, num_slots=K, d_model=d, nhead=nhead, num_layers=L, dim_feedforward=ff, pos_emb="ape")
    P = PO.formula_params(cfg)
    out, g, ds = PO.loss_and_grads(P, tokens(B, K, rep), cfg, cotangent(B, d))
    ref = torch.from_numpy(fx[tag + ":out"])
    assert (out - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    gmax = max(np.abs(fx[tag + ":g:" + n][3:]).max() for n in g)
    for n, t in list(g.items()) + [("dslots", ds)]:
        r = fx[tag + (":dslots" if n == "dslots" else ":g:" + n)]
        got = sample(t)[3:]
        assert np.abs(got - r[3:]).max() < 3e-4 * max(np.abs(r[3:]).max(), 1e-3 * gmax), n


def _ws(B, K, L=1, Din=67, d=128, h=8, ff=2048):
    from ocrl_amd import _lib
    return _lib.lib().ocrl_pool_transformer_long_ws_floats(B, K, Din, d, h, ff, L)


def test_workspace_is_linear_in_tokens():
    a, b = _ws(32, 4096), _ws(32, 1024)
    assert a > 0 and b > 0
    assert a / b < 4.5, a / b
    for L in (1, 2):          # no S^2 term at any depth: doubling the tokens at most doubles the workspace
        assert _ws(4, 8192, L) <= 2.05 * _ws(4, 4096, L)


def test_workspace_of_the_ppo_minibatch_fits():
    """B = 32 (PPO minibatch), a 64x64 feature map (S = 4097), one layer: below 1 GiB (the S^2 score matrix alone would be 17 GB)"""
    assert _ws(32, 4096) * 4 < 2 ** 30


def test_workspace_rejects_bad_shapes():
    """the shapes fwd / bwd reject get no workspace size"""
    assert _ws(32, 4096, L=0) == 0
    assert _ws(0, 4096) == 0
    assert _ws(4, 0) == 0
    assert _ws(4, 4096, Din=0) == 0
    assert _ws(4, 4096, h=16 * 8) == 0          # head size 1
    assert _ws(4, 4096, d=96, h=2) == 0         # d_model not a multiple of 64
    assert _ws(4, 4096, ff=2050) == 0
    assert _ws(4, 4096, L=9) == 0


def test_one_layer_has_no_row_times_ff_limit():
    """at L = 1 the FFN runs on the B CLS rows only: B * S * ff beyond 2^31 is served (128x128 map, B = 64), at L = 2 it is not"""
    assert _ws(64, 16384, L=1) > 0
    assert _ws(64, 16384, L=2) == 0
