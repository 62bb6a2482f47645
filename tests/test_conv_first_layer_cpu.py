"""CPU-only: the entry points of the first encoder layer's own kernels (csrc/conv_first.hip) are declared and exported, and the workspace
queries of the weight-gradient kernels cover what the kernels write: the partial dW slabs and one 64-float bias partial per slab.  The
slab counts are recomputed here from the tile arithmetic (4 x 32 pixel tiles, capped workers), not read back from the library."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1, 1), (1, 3, 5), (1, 4, 32), (1, 7, 33), (1, 9, 65), (3, 13, 100), (2, 33, 31), (3, 20, 44), (5, 30, 70),
          (4, 16, 992), (4, 16, 1024), (4, 17, 1000), (128, 128, 128)]
NEW = ["ocrl_conv2d_first_fwd_ws_floats", "ocrl_conv2d_first_fwd", "ocrl_conv2d_first_wgrad_ws_floats", "ocrl_conv2d_first_bwd_weight"]


def tiles(B, H, W):
    return -(-W // 32) * -(-H // 4) * B


@pytest.fixture(scope="module")
def lib():
    from ocrl_amd import _lib
    return _lib.lib()


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ocrl_hip.h")).read()
    declared = set(re.findall(r"\b(ocrl_[a-z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert lib.ocrl_abi_version() == 5
    assert lib.ocrl_conv2d_first_fwd_ws_floats() >= 76 * 64          # the packed weights [k = 75 (+1)][64]


@pytest.mark.parametrize("B,H,W", SHAPES, ids=lambda v: str(v))
def test_workspace_queries_cover_dw_and_bias_slabs(lib, B, H, W):
    nt = tiles(B, H, W)
    for ks, cpad in ((5, 64), (5, 8), (3, 64)):
        slabs = min(512 // ks, nt) * (1 if cpad == 64 else 2)
        got = lib.ocrl_conv2d_wgrad_ws_floats(B, H, W, ks, cpad)
        assert got >= slabs * (ks * ks * 64 * cpad + 64), (ks, cpad, got)
    workers = min(512, nt)
    got = lib.ocrl_conv2d_first_wgrad_ws_floats(B, H, W)
    assert got >= workers * (64 * 75 + 64), got
    assert got % workers == 0                                        # whole slabs: the GPU test reads the worker count off this
