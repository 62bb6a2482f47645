"""What the multi-segment clip + optimiser step (ocrl_flat_clip_adam_l2_multi, ocrl_flat_clip_rmsprop_l2_multi) promises without a GPU: the
three symbols are exported and declared, the workspace size, and every rejection the header lists, each made before any launch (the
segment table is host memory; its device pointers are fake addresses that are never read)."""
import ctypes
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
SYMBOLS = ("ocrl_flat_clip_multi_ws_floats", "ocrl_flat_clip_adam_l2_multi", "ocrl_flat_clip_rmsprop_l2_multi")


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def test_symbols_are_exported_and_declared():
    lib, L = _lib()
    header = open(os.path.join(ROOT, "include", "ocrl_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in header, name
    assert "#define OCRL_FLAT_MAX_SEGMENTS 8" in header and "ocrl_flat_segment;" in header
    assert lib.FLAT_MAX_SEGMENTS == 8 and ctypes.sizeof(lib.FlatSegment) == 40         # four pointers and a long long
    assert len(L.ocrl_flat_clip_adam_l2_multi.argtypes) == 12 and len(L.ocrl_flat_clip_rmsprop_l2_multi.argtypes) == 10
    assert len(L.ocrl_flat_clip_multi_ws_floats.argtypes) == 0
    assert L.ocrl_flat_clip_multi_ws_floats() > 0
    # the single-buffer entry points keep their signatures
    assert len(L.ocrl_flat_clip_adam_l2.argtypes) == 15 and len(L.ocrl_flat_clip_rmsprop_l2.argtypes) == 12


def _table(nseg=2, **over):
    """`nseg` good segments of 8 floats; over: field -> value for segment `at` (default the last one)"""
    lib, _ = _lib()
    at = over.pop("at", nseg - 1)
    rows = [dict(p=FAKE, g=FAKE, s0=FAKE, s1=FAKE, n=8) for _ in range(nseg)]
    if rows:
        rows[at].update(over)
    return lib.flat_segments([(r["p"], r["g"], r["s0"], r["s1"], r["n"]) for r in rows])


def _call(algo, seg="table", nseg=None, norm=FAKE, ws=FAKE, ws_floats=None, step=1, alpha=0.99, eps=1e-5, table_nseg=2, **over):
    lib, L = _lib()
    if seg == "table":
        seg = _table(table_nseg, **over)
    n = (len(seg) if seg is not None else 2) if nseg is None else nseg
    nws = L.ocrl_flat_clip_multi_ws_floats() if ws_floats is None else ws_floats
    if algo == "adam":
        rc = L.ocrl_flat_clip_adam_l2_multi(seg, n, 0.5, 3e-4, 0.9, 0.999, eps, step, norm, ws, nws, None)
    else:
        rc = L.ocrl_flat_clip_rmsprop_l2_multi(seg, n, 0.5, 7e-4, alpha, eps, norm, ws, nws, None)
    return rc, L.ocrl_last_error().decode()


BOTH = [(dict(nseg=0), "nseg"), (dict(nseg=-1), "nseg"), (dict(nseg=9, table_nseg=8), "nseg"), (dict(seg=None), "null"),
        (dict(norm=None), "norm_out"), (dict(ws=None), "ws"), (dict(p=None), "null"), (dict(g=None), "null"), (dict(s0=None), "null"),
        (dict(p=None, at=0), "segment 0"), (dict(n=0), "n >= 1"), (dict(n=-4), "n >= 1"), (dict(n=0, at=0), "segment 0"),
        (dict(p=FAKE + 4), "aligned"), (dict(g=FAKE + 8), "aligned"), (dict(s0=FAKE + 12), "aligned"), (dict(g=FAKE + 4, at=0), "segment 0"),
        (dict(ws_floats="short"), "workspace"), (dict(ws_floats=0), "workspace")]
ADAM_ONLY = [(dict(s1=None), "null"), (dict(s1=FAKE + 4), "aligned"), (dict(step=0), "step"), (dict(step=-3), "step")]
RMS_ONLY = [(dict(alpha=0.0), "alpha"), (dict(alpha=1.0), "alpha"), (dict(alpha=-0.5), "alpha"), (dict(alpha=1.5), "alpha"),
            (dict(alpha=math.nan), "alpha"), (dict(eps=0.0), "eps"), (dict(eps=-1e-5), "eps"), (dict(eps=math.nan), "eps")]
CASES = [("adam", kw, word) for kw, word in BOTH + ADAM_ONLY] + [("rmsprop", kw, word) for kw, word in BOTH + RMS_ONLY]


@pytest.mark.parametrize("algo,kw,word", CASES, ids=[f"{a}-{'-'.join(f'{k}_{v}' for k, v in kw.items())}" for a, kw, _ in CASES])
def test_rejects_before_any_launch(algo, kw, word):
    kw = dict(kw)
    if kw.get("ws_floats") == "short":
        kw["ws_floats"] = _lib()[1].ocrl_flat_clip_multi_ws_floats() - 1
    rc, msg = _call(algo, **kw)
    assert rc != 0 and f"ocrl_flat_clip_{algo}_l2_multi" in msg and word in msg, msg


def test_eight_segments_pass_the_checks_that_nine_fail():
    """the bound is OCRL_FLAT_MAX_SEGMENTS itself: eight good segments get past the segment count (and are then stopped by the next
    check, a short workspace, still before any launch)"""
    rc, msg = _call("adam", table_nseg=8, ws_floats=1)
    assert rc != 0 and "workspace" in msg and "nseg" not in msg
    rc, msg = _call("rmsprop", table_nseg=8, ws_floats=1)
    assert rc != 0 and "workspace" in msg and "nseg" not in msg


def test_rmsprop_ignores_the_unused_second_state_pointer():
    """s1 is unused by RMSprop: a null or misaligned one is not what a call is rejected for"""
    for s1 in (None, FAKE + 4):
        rc, msg = _call("rmsprop", s1=s1, ws_floats=1)
        assert rc != 0 and "workspace" in msg, msg
