"""GPU checks of the multi-segment clip + optimiser step (ocrl_flat_clip_adam_l2_multi, ocrl_flat_clip_rmsprop_l2_multi) against the fp64
single-buffer restatements (ppo_ref.clip_adam_l2, a2c_ref.rmsprop_tf_l2) applied to the concatenation of the segments.

Bounds are those of tests/test_gpu_ppo.py::test_flat_clip_adam_step, whose case construction (step_case), learning rate (STEP_LR) and modes
(STEP_MODES) are used as they are: the norm within 1e-6 relative, dp / lr within 4 x STEP_DEV of the fp64 step, the optimiser's state within
1e-6 of its maximum.  STEP_DEV is set by the rounding of p + dp at |p| < 0.5 and lr = 3e-3 (half an ulp of p over lr), which is the same for
the RMSprop update on the same p at the same lr, so the RMSprop cases carry the same bound."""
import functools
import math

import pytest
import torch

from tests import a2c_ref as A
from tests import ppo_ref as P
from tests.gpu_util import log
from tests.test_gpu_acnet import err, nanlike
from tests.test_gpu_ppo import MAX_NORM, STEP_DEV, STEP_LR, STEP_MODES, step_case

pytestmark = pytest.mark.gpu

LENGTHS = [(1,), (3, 1027), (70001, 5, 4096), (1, 2, 3, 4, 255, 1024, 1025, 4099)]
IDS = ["1", "3+1027", "70001+5+4096", "eight"]
PAD, GUARD = 8, 77.0
RMS_ALPHA, RMS_EPS = 0.99, 1e-5


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


@functools.lru_cache(maxsize=None)
def case(lengths, t, scale):
    """the planted state of one step over the concatenation, built once on the CPU: p, g, m, v float32 [sum(lengths)] (step_case)"""
    return step_case(sum(lengths), t, scale)


@functools.lru_cache(maxsize=None)
def adam_ref(lengths, t, scale, max_norm):
    return P.clip_adam_l2(*case(lengths, t, scale), max_norm, STEP_LR, t)


def rms_state(lengths, t, scale):
    """the square average on entry: ones at the first step, else ones plus the planted second moment (positive, varied)"""
    v = case(lengths, t, scale)[3]
    return torch.ones_like(v) if t == 1 else 1.0 + 100.0 * v


@functools.lru_cache(maxsize=None)
def rms_ref(lengths, t, scale, max_norm):
    p, g, _, _ = case(lengths, t, scale)
    return A.rmsprop_tf_l2(p, g, rms_state(lengths, t, scale), max_norm, STEP_LR, RMS_ALPHA, RMS_EPS)


def run_multi(algo, lengths, flats, max_norm, t=1, lr=STEP_LR):
    """one call on device copies of the flat CPU tensors `flats` = (p, g, s0[, s1]) cut into `lengths`, each segment in a buffer of its
    own with PAD guard floats behind it.  Checks the guards and g, returns ([p, s0[, s1]] re-joined on the CPU, norm)."""
    lib, L = _lib()
    bufs = []                                                           # [segment][tensor]
    for part in zip(*[f.split(list(lengths)) for f in flats]):
        row = []
        for src in part:
            b = torch.full((src.numel() + PAD,), GUARD, device="cuda")
            b[:src.numel()] = src.cuda()
            row.append(b)
        bufs.append(row)
    seg = lib.flat_segments([(lib.ptr(r[0]), lib.ptr(r[1]), lib.ptr(r[2]), lib.ptr(r[3]) if len(r) > 3 else None, n) for r, n in zip(bufs, lengths)])
    nws = L.ocrl_flat_clip_multi_ws_floats()
    ws, norm = nanlike(nws), nanlike(1)
    if algo == "adam":
        rc = L.ocrl_flat_clip_adam_l2_multi(seg, len(seg), max_norm, lr, 0.9, 0.999, 1e-5, t, lib.ptr(norm), lib.ptr(ws), nws, lib.stream())
    else:
        rc = L.ocrl_flat_clip_rmsprop_l2_multi(seg, len(seg), max_norm, lr, RMS_ALPHA, RMS_EPS, lib.ptr(norm), lib.ptr(ws), nws, lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ocrl_last_error().decode()
    for r, n in zip(bufs, lengths):
        for b in r:
            assert (b[n:] == GUARD).all(), "the step wrote past a segment's n floats"
    assert torch.equal(torch.cat([r[1][:n] for r, n in zip(bufs, lengths)]).cpu(), flats[1]), "g was written"
    out = [torch.cat([r[k][:n] for r, n in zip(bufs, lengths)]).cpu() for k in range(len(flats)) if k != 1]
    return out, norm.cpu()[0]


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("lengths", LENGTHS, ids=IDS)
def test_adam_multi_against_the_fp64_step_on_the_concatenation(lengths, t):
    for tag, scale, max_norm in STEP_MODES:
        p, g, m, v = case(lengths, t, scale)
        r = adam_ref(lengths, t, scale, max_norm)
        (p1, m1, v1), norm = run_multi("adam", lengths, (p, g, m, v), max_norm, t)
        (p2, m2, v2), norm2 = run_multi("adam", lengths, (p, g, m, v), max_norm, t)
        assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(norm, norm2)
        e_n = abs(norm.item() - r.norm.item()) / r.norm.item()
        dev = ((p1.double() - p.double()) - (r.p - p.double())).abs().max().item() / STEP_LR
        moved = (p1 != p).double().mean().item()
        e_m, e_v = err(m1, r.m), err(v1, r.v)
        log(f"adam multi {lengths} t{t} {tag}: norm rel err {e_n:.2e}, dp/lr dev {dev:.2e} (bound {4 * STEP_DEV:.1e}), m {e_m:.2e} v {e_v:.2e}, "
            f"coef {r.coef.item():.4f}, {moved:.2f} of p moved")
        assert e_n <= 1e-6 and dev <= 4 * STEP_DEV
        assert (r.coef.item() < 1.0) == (tag in ("at", "above")) and moved > 0.9
        assert e_m <= 1e-6 and e_v <= 1e-6


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("lengths", LENGTHS, ids=IDS)
def test_rmsprop_multi_against_the_fp64_step_on_the_concatenation(lengths, t):
    """t only chooses the planted state: the square average at ones (1) or varied (7)"""
    for tag, scale, max_norm in STEP_MODES:
        p, g, _, _ = case(lengths, t, scale)
        sq = rms_state(lengths, t, scale)
        r = rms_ref(lengths, t, scale, max_norm)
        (p1, s1), norm = run_multi("rmsprop", lengths, (p, g, sq), max_norm)
        (p2, s2), norm2 = run_multi("rmsprop", lengths, (p, g, sq), max_norm)
        assert torch.equal(p1, p2) and torch.equal(s1, s2) and torch.equal(norm, norm2)
        e_n = abs(norm.item() - r.norm.item()) / r.norm.item()
        dev = ((p1.double() - p.double()) - (r.p - p.double())).abs().max().item() / STEP_LR
        e_s = err(s1, r.sq)
        log(f"rmsprop multi {lengths} t{t} {tag}: norm rel err {e_n:.2e}, dp/lr dev {dev:.2e} (bound {4 * STEP_DEV:.1e}), sq {e_s:.2e}, "
            f"coef {r.coef.item():.4f}")
        assert e_n <= 1e-6 and dev <= 4 * STEP_DEV and e_s <= 1e-6
        assert (r.coef.item() < 1.0) == (tag in ("at", "above")) and not torch.equal(p1, p)


@pytest.mark.parametrize("algo", ["adam", "rmsprop"])
def test_a_segment_without_a_gradient_keeps_its_parameters(algo):
    """the middle segment's g is all zero (and m = v = 0): its p comes back bit for bit, and with Adam its m and v too -- what the gaps of
    an encoder's range rely on.  RMSprop's square average decays towards zero there, as in a buffer of its own."""
    lengths, mid = (5, 1027, 3), slice(5, 5 + 1027)
    p, g, m, v = (x.clone() for x in step_case(sum(lengths), 1, 100.0))
    g[mid] = 0.0
    p[5] = -0.0                                                        # a signed zero stays what it is
    if algo == "adam":
        (p1, m1, v1), norm = run_multi(algo, lengths, (p, g, m, v), MAX_NORM, 1)
        assert torch.equal(m1[mid].view(torch.int32), m[mid].view(torch.int32)) and torch.equal(v1[mid].view(torch.int32), v[mid].view(torch.int32))
        assert (m1[:5] != 0).all() and (v1[-3:] != 0).all()
    else:
        (p1, s1), norm = run_multi(algo, lengths, (p, g, torch.ones_like(p)), MAX_NORM)
        assert (s1[mid] == s1[mid][0]).all() and 0.98 < s1[mid][0].item() < 1.0
    assert torch.equal(p1[mid].view(torch.int32), p[mid].view(torch.int32))
    assert (p1[:5] != p[:5]).all() and (p1[-3:] != p[-3:]).all()
    assert abs(norm.item() - g.double().norm().item()) <= 1e-6 * g.double().norm().item()


@pytest.mark.parametrize("algo", ["adam", "rmsprop"])
def test_a_nan_in_one_segment_reaches_the_norm_and_every_weight_of_every_segment(algo):
    lengths = (3, 1027, 4096)
    p, g, m, v = (x.clone() for x in step_case(sum(lengths), 1, 100.0))
    g[3 + 515] = float("nan")                                          # inside the second segment
    flats = (p, g, m, v) if algo == "adam" else (p, g, torch.ones_like(p))
    lib, L = _lib()
    # run_multi compares g with equal(), which a NaN fails: compare the bits here
    bufs = [[torch.full((n + PAD,), GUARD, device="cuda") for _ in flats] for n in lengths]
    for row, part, n in zip(bufs, zip(*[f.split(list(lengths)) for f in flats]), lengths):
        for b, src in zip(row, part):
            b[:n] = src.cuda()
    seg = lib.flat_segments([(lib.ptr(r[0]), lib.ptr(r[1]), lib.ptr(r[2]), lib.ptr(r[3]) if len(r) > 3 else None, n) for r, n in zip(bufs, lengths)])
    nws = L.ocrl_flat_clip_multi_ws_floats()
    ws, norm = nanlike(nws), torch.zeros(1, device="cuda")
    if algo == "adam":
        rc = L.ocrl_flat_clip_adam_l2_multi(seg, 3, MAX_NORM, STEP_LR, 0.9, 0.999, 1e-5, 1, lib.ptr(norm), lib.ptr(ws), nws, lib.stream())
    else:
        rc = L.ocrl_flat_clip_rmsprop_l2_multi(seg, 3, MAX_NORM, STEP_LR, RMS_ALPHA, RMS_EPS, lib.ptr(norm), lib.ptr(ws), nws, lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ocrl_last_error().decode()
    assert math.isnan(norm.item())
    for r, n in zip(bufs, lengths):
        assert torch.isnan(r[0][:n]).all() and all((b[n:] == GUARD).all() for b in r)
    got_g = torch.cat([r[1][:n] for r, n in zip(bufs, lengths)]).cpu()
    assert torch.equal(got_g.view(torch.int32), g.view(torch.int32))


def test_bad_arguments_leave_the_buffers_alone():
    """with real device buffers: a rejected call has launched nothing"""
    lib, L = _lib()
    nws = L.ocrl_flat_clip_multi_ws_floats()
    b = [torch.zeros(8, device="cuda") for _ in range(4)]
    ws, norm = torch.zeros(nws, device="cuda"), nanlike(1)
    good = (lib.ptr(b[0]), lib.ptr(b[1]), lib.ptr(b[2]), lib.ptr(b[3]), 8)
    call = lambda segs, nseg, nw=nws, step=1: L.ocrl_flat_clip_adam_l2_multi(lib.flat_segments(segs), nseg, 0.5, 1e-3, 0.9, 0.999, 1e-5, step,
                                                                             lib.ptr(norm), lib.ptr(ws), nw, lib.stream())
    assert call([good], 0) != 0 and call([good] * 8, 9) != 0 and call([good], 1, nws - 1) != 0 and call([good], 1, step=0) != 0
    assert call([good, good[:4] + (0,)], 2) != 0 and call([good, (None,) + good[1:]], 2) != 0
    assert call([good, (b[0].data_ptr() + 4,) + good[1:]], 2) != 0 and "aligned" in L.ocrl_last_error().decode()
    torch.cuda.synchronize()
    assert all((t == 0).all() for t in b) and torch.isnan(norm).all()
