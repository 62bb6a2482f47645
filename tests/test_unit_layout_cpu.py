"""The workspace sizes of the stateless heads, pinned: every value below is what commit 352b163 (the parent of the change that moved the
units' shared host-side rules into csrc/unit_base.h) returned for the same arguments.  A workspace size is the end of the unit's layout,
so it moves when an offset rule moves: the conv slab rule, the split-k scratch rule (which also decides the summation order of the weight
gradients), the stride-4 padding, the order of the carves.  The table reaches every branch of every layout: scratch of 0, a few and the
cap of 32 splits, each widest-weight term, padded and unpadded widths, one and several layers, both attention forms, 64 slabs and fewer,
the conv.hip branch of the VAE decoder.  Refused shapes (size 0) are covered by the units' own CPU tests."""
import ctypes

import pytest

# (entry, arguments, floats).  pool_rn: (B, K, D, g_dims, f_dims); probe: (B, K, N, D, O, slot_rows, dims, P); the rest as in ocrl_hip.h
TABLE = [
    ('pool_transformer', (4, 6, 64, 4, 64, 1), 165696),
    ('pool_transformer', (4, 6, 64, 4, 64, 2), 182784),
    ('pool_transformer', (128, 6, 64, 4, 64, 1), 1283008),
    ('pool_transformer', (128, 6, 64, 4, 64, 2), 1827776),
    ('pool_transformer', (2048, 6, 64, 4, 64, 1), 18293120),
    ('pool_transformer', (2048, 6, 64, 4, 64, 2), 27009408),
    ('pool_transformer', (128, 6, 128, 8, 2048, 1), 6565824),
    ('pool_transformer', (128, 6, 256, 8, 256, 2), 7189056),
    ('pool_transformer_long', (4, 40, 64, 64, 4, 64, 1), 181696),
    ('pool_transformer_long', (4, 4096, 64, 64, 4, 64, 1), 4806336),
    ('pool_transformer_long', (4, 40, 64, 64, 4, 64, 2), 341312),
    ('pool_transformer_long', (4, 4096, 64, 64, 4, 64, 2), 20735680),
    ('pool_transformer_long', (4, 40, 67, 64, 4, 64, 1), 212160),
    ('pool_transformer_long', (4, 4096, 67, 64, 4, 64, 1), 7043264),
    ('pool_transformer_long', (4, 40, 67, 64, 4, 64, 2), 371776),
    ('pool_transformer_long', (4, 4096, 67, 64, 4, 64, 2), 22972608),
    ('pool_transformer_long', (4, 40, 67, 128, 8, 2048, 2), 1244928),
    ('pool_transformer_long', (32, 40, 300, 64, 4, 64, 1), 631104),
    ('pool_rn', (4, 5, 64, (64, 64), (64, 32)), 43264),
    ('pool_rn', (32, 6, 64, (64, 64), (64, 32)), 345664),
    ('pool_rn', (4, 5, 67, (64, 64), (64, 32)), 47104),
    ('pool_rn', (32, 6, 67, (64, 64), (64, 32)), 374336),
    ('pool_rn', (32, 6, 67, (32, 128), (256, 32)), 587648),
    ('pool_rn', (512, 6, 64, (64,), (32,)), 4133120),
    ('naturecnn', (2, 64, 64, 3, 1, 4, 0, 32), 194240),
    ('naturecnn', (2, 64, 64, 3, 2, 4, 0, 32), 388480),
    ('naturecnn', (2, 64, 64, 3, 1, 2, 0, 32), 270144),
    ('naturecnn', (2, 64, 64, 3, 2, 2, 0, 32), 540288),
    ('naturecnn', (2, 64, 64, 3, 1, 4, 1, 32), 194112),
    ('naturecnn', (2, 64, 64, 3, 1, 2, 1, 32), 270016),
    ('naturecnn', (2, 84, 84, 3, 1, 4, 0, 32), 337280),
    ('naturecnn', (2, 84, 84, 3, 2, 4, 0, 32), 674496),
    ('naturecnn', (2, 84, 84, 3, 1, 2, 0, 32), 423936),
    ('naturecnn', (2, 84, 84, 3, 2, 2, 0, 32), 847808),
    ('naturecnn', (2, 84, 84, 3, 1, 4, 1, 32), 337152),
    ('naturecnn', (2, 84, 84, 3, 1, 2, 1, 32), 423808),
    ('naturecnn', (32, 64, 64, 3, 1, 4, 0, 32), 1951360),
    ('naturecnn', (3, 64, 84, 1, 2, 2, 0, 64), 749120),
    ('pool_cnn', (2, 36, 36, 3, 0), 211648),
    ('pool_cnn', (2, 36, 36, 67, 0), 735936),
    ('pool_cnn', (2, 64, 84, 3, 0), 489920),
    ('pool_cnn', (2, 64, 84, 67, 0), 1800640),
    ('pool_cnn', (2, 36, 36, 3, 32), 211776),
    ('pool_cnn', (2, 36, 36, 67, 32), 736064),
    ('pool_cnn', (2, 64, 84, 3, 32), 490048),
    ('pool_cnn', (2, 64, 84, 67, 32), 1800768),
    ('pool_cnn', (32, 64, 64, 3, 32), 2119808),
    ('vae', (2, 16, 3, 4, 32, 0, 0), 4405120),
    ('vae', (2, 16, 3, 4, 32, 1, 0), 4405120),
    ('vae', (2, 16, 3, 4, 32, 0, 1), 4757568),
    ('vae', (2, 16, 3, 4, 32, 1, 1), 4757568),
    ('vae', (2, 64, 3, 4, 32, 0, 0), 5495680),
    ('vae', (2, 64, 3, 4, 32, 1, 0), 5495680),
    ('vae', (2, 64, 3, 4, 32, 0, 1), 8848960),
    ('vae', (2, 64, 3, 4, 32, 1, 1), 8848960),
    ('vae', (32, 64, 1, 4, 64, 0, 1), 72582080),
    ('probe', (16, 6, 5, 192, 15, 1, (15,), 4), 12544),
    ('probe', (128, 6, 5, 192, 15, 1, (15,), 4), 65472),
    ('probe', (16, 6, 5, 192, 15, 1, (256, 256, 256, 15), 4), 134400),
    ('probe', (128, 6, 5, 192, 15, 1, (256, 256, 256, 15), 4), 1214144),
    ('probe', (16, 6, 5, 192, 15, 0, (90,), 4), 41600),
    ('probe', (1024, 6, 5, 192, 15, 0, (90,), 4), 489600),
    ('probe', (16, 6, 5, 192, 15, 0, (256, 256, 256, 90), 4), 70912),
    ('probe', (1024, 6, 5, 192, 15, 0, (256, 256, 256, 90), 4), 1815872),
    ('probe', (16, 6, 5, 67, 15, 1, (15,), 4), 15104),
    ('probe', (128, 6, 5, 67, 15, 1, (15,), 4), 107776),
    ('probe', (16, 6, 5, 67, 15, 1, (256, 256, 256, 15), 4), 158336),
    ('probe', (128, 6, 5, 67, 15, 1, (256, 256, 256, 15), 4), 1283776),
    ('probe', (16, 6, 5, 67, 15, 0, (90,), 4), 19904),
    ('probe', (1024, 6, 5, 67, 15, 0, (90,), 4), 490816),
    ('probe', (16, 6, 5, 67, 15, 0, (256, 256, 256, 90), 4), 89408),
    ('probe', (1024, 6, 5, 67, 15, 0, (256, 256, 256, 90), 4), 1902912),
    ('mae', (2, 16, 4, 64, 2, 2, 32, 1, 2, 0, 0), 33655552),
    ('mae', (2, 16, 4, 64, 2, 2, 32, 1, 2, 4, 1), 33614208),
    ('probe_match', (16, 4), 96),
    # the IODINE / broadcast-decoder kernel entries (include/ocrl_hip_iodine.h), newer than that commit: the launchers' own scratch rules
    # (66 floats per 256-pixel block of the ELBO, one float per sampled element, the two packed 64 -> 4 weight tensors, 1024 loss partials)
    ('iodine_elbo', (2, 3, 32), 528),
    ('iodine_elbo', (1, 16, 16), 66),
    ('iodine_elbo', (1, 3, 48), 594),
    ('iodine_sample', (3077,), 3077),
    ('bcdec_c4', (), 4608),
    ('bcdec_mix', (), 1024),
]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _ws_floats(entry, a):
    from ocrl_amd import _lib
    L = _lib.lib()
    if entry == "pool_rn":
        B, K, D, g, f = a
        return L.ocrl_pool_rn_ws_floats(B, K, D, len(g), _ints(g), len(f), _ints(f))
    if entry == "probe":
        B, K, N, D, O, slot_rows, dims, P = a
        return L.ocrl_probe_ws_floats(B, K, N, D, O, slot_rows, len(dims), _ints(dims), P)
    return getattr(L, f"ocrl_{entry}_ws_floats")(*a)


@pytest.mark.parametrize("entry", sorted({t[0] for t in TABLE}))
def test_workspace_sizes_are_the_recorded_ones(entry):
    rows = [t for t in TABLE if t[0] == entry]
    got = [(a, _ws_floats(entry, a)) for _, a, _ in rows]
    assert got == [(a, n) for _, a, n in rows]
