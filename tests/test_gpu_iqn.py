"""GPU checks of DQN's implicit quantile head: the entry points of include/ocrl_hip_iqn.h through the C ABI, ``DQN._train_step_iqn``,
checkpoints, ``train_sb3.build`` and the entry points, against the fp64 restatement of tests/iqn_ref.py.

Bounds.  They are tests/test_gpu_qr.py's, for the same tile arithmetic: the TD step's scalars 1e-4 relative with a floor of 1e-3 of the
largest scalar, every gradient (the embedding's, the chain's, the output Linear's, dfeatures) and row_loss 3e-4 of its tensor's maximum
with a floor of 1e-3 of the largest gradient.  The embedding Linear and the product with the features are one more link of the same
chain; the loss and its gradient are continuous at u = 0, at |u| = kappa and at phi = 0, so a value that lands on the other side of a
decision in fp32 moves the result by no more than the rounding that put it there.  The generic path (ocrl_iqn_fwd with save, torch
autograd on its quantile values, ocrl_iqn_bwd) meets the same bound.  The forward's quantile values are a Linear chain's outputs: within
1e-5 of the largest; q, a mean of them, 1e-4.  The integer rules (actions, the fractions' bits) are exact.  ``train_step()`` is graded on
dp / lr, elementwise, against the fp64 restatement fed the batches and the fractions the run drew; the bound is the one of
test_gpu_c51.py::test_three_updates_against_the_restatement: 4 x the largest deviation of the fp32 torch restatement from the fp64 one on
the very inputs of the test, measured by the test itself on the CPU.  The fractions are always the GPU's own (``ocrl_iqn_taus``), never
re-derived; with ``noisy`` both restatements are fed the factors the GPU drew."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import dqn_ref as R
from tests import iqn_ref as I
from tests import qr_ref as Q
from tests import replay_ext_ref as X
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
# (B, F, A, N, N', C): the smallest; a general small one; a tile is exactly one batch row; a batch row straddles tiles and N != N';
# several batch rows per tile; the limits of N, N' and C; many actions; 65 tiles, so the slabs wrap
SHAPES = [(1, 4, 1, 1, 1, 4), (5, 8, 2, 5, 3, 8), (3, 8, 3, 16, 16, 64), (2, 12, 3, 17, 7, 64), (37, 128, 4, 8, 8, 64), (3, 12, 4, 64, 64, 64),
          (20, 12, 64, 4, 4, 12), (130, 8, 4, 8, 8, 64)]
LAYOUTS = {"none": ((), ()), "mlp": ((64, 64), (1, 1)), "tanh": ((4,), (2,))}
GAMMA, KAPPA = 0.9, 1.0
SITE_IQN_TAU = 450


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def nanlike(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def err(got, want, floor=0.0):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert torch.isfinite(got).all(), "non-finite entries (an output the kernels did not write?)"
    return (got - want).abs().max().item() / max(want.abs().max().item(), floor, 1e-30)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def random_taus(gen, B, N):
    """random k / 2^24 with the two ends of the range among them (a single fraction stays random: at tau = 0 a non-negative u weighs
    nothing, and the one-row case would have no gradient at all)"""
    t = torch.randint(0, 2 ** 24, (B, N), generator=gen).float() / 2 ** 24
    if t.numel() > 1:
        t[0, 0], t[-1, -1] = 0.0, 1.0 - 2.0 ** -24
    return t


# ------------------------------------------------------------------------------------------------------------ 1. the TD step, 2. the forward
@functools.lru_cache(maxsize=None)
def td_case(B, F, A, N, Np, C, lname):
    """the inputs of a case on the CPU, built once (test_gpu_qr.py's pattern): every third row done with next_quantiles = NaN and next_q =
    inf there, two actions outside [0, A), rewards 6 / -6 on rows 2 .. 4 (not done, not done, done), per-row discounts and weights, and
    fractions k / 2^24 that include 0 and 1 - 2^-24"""
    dims, _ = LAYOUTS[lname]
    gen = torch.Generator().manual_seed(311 + B + N)
    ps = I.make_params(F, A, C, dims, 83)
    x = torch.randn(B, F, generator=gen)
    taus = random_taus(gen, B, N)
    next_quantiles = torch.randn(B, A, Np, generator=gen) * 2
    next_q = torch.randn(B, A, generator=gen)
    actions = torch.randint(0, A, (B,), generator=gen)
    rewards = torch.randn(B, generator=gen) * 1.5
    dones = (torch.arange(B) % 3 == 1).to(torch.uint8)
    next_quantiles[dones.bool()] = float("nan")
    next_q[dones.bool()] = float("inf")
    if B > 1:
        actions[0], actions[-1] = -3, A + 5
    if B > 4:
        rewards[2], rewards[3], rewards[4] = 6.0, -6.0, -6.0
        next_quantiles[2:4] = next_quantiles[2:4].clamp(-1.0, 1.0)               # the shift of rows 2 and 3 stays inside the reward's reach
    discounts = GAMMA ** torch.randint(1, 4, (B,), generator=gen).float()
    weights = torch.rand(B, generator=gen) * 0.9 + 0.1
    return dict(x=x, taus=taus, ps=ps, next_quantiles=next_quantiles, next_q=next_q, actions=actions, rewards=rewards, dones=dones, discounts=discounts,
                weights=weights)


def options(case, opt):
    return (case["discounts"], case["weights"]) if opt else (None, None)


@functools.lru_cache(maxsize=None)
def td_ref(B, F, A, N, Np, C, lname, opt):
    c = td_case(B, F, A, N, Np, C, lname)
    disc, wts = options(c, opt)
    return I.iqn_step(c["x"], c["taus"], c["ps"], LAYOUTS[lname][1], A, C, c["next_quantiles"], c["next_q"], c["actions"], c["rewards"], c["dones"], GAMMA,
                      KAPPA, disc, wts)


def run_td(c, layout, A, C, opt=False, want_dx=True, rows=None, kappa=KAPPA, given=None):
    """ocrl_iqn_td_fwd_bwd on a case; ``given`` = (discounts, weights) replaces the case's"""
    lib, L = _lib()
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    x, taus = sel(c["x"]), sel(c["taus"])
    (B, F), N, Np = x.shape, taus.shape[1], c["next_quantiles"].shape[2]
    d = lib.iqn_desc(B, F, A, N, C, *layout)
    n = L.ocrl_iqn_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, ts, pd = x.cuda(), taus.cuda().contiguous(), [p.cuda() for p in c["ps"]]
    disc, wts = options(c, opt) if given is None else given
    t = [sel(c["next_q"]).cuda().contiguous(), sel(c["actions"]).cuda().long(), sel(c["rewards"]).cuda(), sel(c["dones"]).cuda(),
         None if disc is None else sel(disc).cuda(), None if wts is None else sel(wts).cuda()]
    nq = sel(c["next_quantiles"]).cuda().contiguous()
    scal, row_loss, dw = nanlike(3), nanlike(B), [nanlike(*p.shape) for p in c["ps"]]
    dx, ws = nanlike(B, F) if want_dx else None, nanlike(n)
    lib.check(L.ocrl_iqn_td_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptr(ts), lib.ptrs(pd), lib.ptr(nq), Np, *[lib.ptr(v) for v in t], GAMMA, kappa,
                                    lib.ptr(scal), lib.ptr(row_loss), lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(scal=scal, row_loss=row_loss, dw=dw, dx=dx)


def run_fwd(x, taus, ps, layout, A, C, save=0, outs=(1, 1)):
    lib, L = _lib()
    (B, F), N = x.shape, taus.shape[1]
    d = lib.iqn_desc(B, F, A, N, C, *layout)
    n = L.ocrl_iqn_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, ts, pd, ws = x.cuda(), taus.cuda().contiguous(), [p.cuda() for p in ps], nanlike(n)
    th, q = (nanlike(B, A, N) if outs[0] else None), (nanlike(B, A) if outs[1] else None)
    need = save or not outs[0]
    lib.check(L.ocrl_iqn_fwd(ctypes.byref(d), lib.ptr(xs), lib.ptr(ts), lib.ptrs(pd), lib.ptr(th), lib.ptr(q), save, lib.ptr(ws) if need else None,
                             n if need else 0, lib.stream()))
    torch.cuda.synchronize()
    return (th, q), (d, xs, ts, pd, ws, n)


def run_generic(c, layout, A, C, opt):
    """the same gradients without the fused step: ocrl_iqn_fwd with save, dquantiles formed by torch autograd (fp32, on the CPU) from its
    quantile values, then ocrl_iqn_bwd"""
    lib, L = _lib()
    (th, _), (d, xs, ts, pd, ws, n) = run_fwd(c["x"], c["taus"], c["ps"], layout, A, C, save=1, outs=(1, 0))
    th = th.cpu().requires_grad_(True)
    disc, wts = options(c, opt)
    I.iqn_loss(th, c["taus"], c["next_quantiles"], c["next_q"], c["actions"], c["rewards"], c["dones"], GAMMA, KAPPA, disc, wts)[0].backward()
    dq = th.grad.cuda().contiguous()
    dw, dx = [nanlike(*p.shape) for p in c["ps"]], nanlike(*c["x"].shape)
    lib.check(L.ocrl_iqn_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptr(ts), lib.ptrs(pd), lib.ptr(dq), lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    nodx = [nanlike(*p.shape) for p in c["ps"]]
    lib.check(L.ocrl_iqn_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptr(ts), lib.ptrs(pd), lib.ptr(dq), None, lib.ptrs(nodx), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(nodx, dw))                         # without dfeatures: the same dw
    return dict(dw=dw, dx=dx)


def check_inputs(c, layout, B, A, C, tag):
    """the inputs do what td_case's docstring says: pairs on both sides of every decision, rows 2 .. 4 wholly beyond kappa"""
    theta = I.quantiles(c["x"].double(), c["taus"], [p.double() for p in c["ps"]], layout[1], A, C)[0]
    for disc in (torch.full((B,), GAMMA, dtype=torch.float64), c["discounts"].double()):
        T = Q.targets(c["next_quantiles"].double(), c["next_q"].double(), c["rewards"].double(), c["dones"], disc)
        u = T.unsqueeze(1) - theta[torch.arange(B), c["actions"].clamp(0, A - 1)].unsqueeze(2)
        if u.numel() >= 1000:                                                    # the small cases need not hold every kind of pair
            assert (u.abs() > KAPPA).any() and (u.abs() < KAPPA).any() and (u < 0).any() and (u > 0).any()
        assert (u[2] > KAPPA).all() and (u[3] < -KAPPA).all() and (u[4] < -KAPPA).all() and c["dones"][4] and not c["dones"][2] and not c["dones"][3]
        log(f"iqn td inputs {tag}: {(u.abs() > KAPPA).double().mean().item():.0%} of pairs beyond kappa, {(u < 0).double().mean().item():.0%} negative")
    assert c["taus"].min() == 0.0 and c["taus"].max() == 1.0 - 2.0 ** -24


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A, N, Np, C", SHAPES, ids=lambda v: str(v))
def test_td_step_against_fp64(B, F, A, N, Np, C, lname):
    layout = LAYOUTS[lname]
    c = td_case(B, F, A, N, Np, C, lname)
    if B > 4:
        check_inputs(c, layout, B, A, C, f"B{B} N{N} {lname}")
    for opt in (False, True):
        scal, dx, dw, ql = td_ref(B, F, A, N, Np, C, lname, opt)
        got, gen = run_td(c, layout, A, C, opt), run_generic(c, layout, A, C, opt)
        tag = f"B{B} F{F} A{A} N{N} N'{Np} C{C} {lname} {'disc+w' if opt else 'gamma'}"
        smax = scal.abs().max().item()
        worst_s = worst_g = worst_gen = 0.0
        for i, k in enumerate(("loss", "mean_q", "mean_target")):
            e = abs(got["scal"][i].item() - scal[i].item()) / max(abs(scal[i].item()), 1e-3 * smax, 1e-30)
            worst_s = max(worst_s, e)
            log(f"iqn td {tag} {k}: got {got['scal'][i].item():.6f} want {scal[i].item():.6f} rel err {e:.2e}")
            assert e <= 1e-4, (tag, k, e, got["scal"].tolist(), scal.tolist())
        gmax = max(g.abs().max().item() for g in [dx] + dw)
        for nme, g, gg, w in zip(["dx"] + [f"dw{i}" for i in range(len(dw))], [got["dx"]] + got["dw"], [gen["dx"]] + gen["dw"], [dx] + dw):
            e, eg = err(g, w, 1e-3 * gmax), err(gg, w, 1e-3 * gmax)
            worst_g, worst_gen = max(worst_g, e), max(worst_gen, eg)
            assert e <= 3e-4 and eg <= 3e-4, (tag, nme, e, eg)
        er = err(got["row_loss"], ql, 1e-3 * gmax)
        log(f"iqn td {tag}: worst scalar rel err {worst_s:.2e} (bound 1e-4), worst gradient {worst_g:.2e}, generic path {worst_gen:.2e}, "
            f"row_loss {er:.2e} (bound 3e-4)")
        assert er <= 3e-4, (tag, er)
        # without dfeatures, and again: the same bits
        nodx, again = run_td(c, layout, A, C, opt, want_dx=False), run_td(c, layout, A, C, opt)
        for other in (nodx, again):
            assert torch.equal(bits(other["scal"]), bits(got["scal"])) and torch.equal(bits(other["row_loss"]), bits(got["row_loss"]))
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(other["dw"], got["dw"]))
        assert nodx["dx"] is None and torch.equal(bits(again["dx"]), bits(got["dx"]))
    # every optional array null is discounts = gamma and weights = 1, bit for bit
    plain = run_td(c, layout, A, C, False)
    filled = run_td(c, layout, A, C, given=(torch.full((B,), GAMMA), torch.ones(B)))
    assert torch.equal(bits(plain["scal"]), bits(filled["scal"])) and torch.equal(bits(plain["row_loss"]), bits(filled["row_loss"]))
    assert torch.equal(bits(plain["dx"]), bits(filled["dx"])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(plain["dw"], filled["dw"]))


def test_td_step_at_another_kappa():
    """kappa = 0.25 and 3: the threshold is an argument, not a constant"""
    B, F, A, N, Np, C = SHAPES[3]
    c = td_case(B, F, A, N, Np, C, "mlp")
    for kappa in (0.25, 3.0):
        scal, dx, dw, ql = I.iqn_step(c["x"], c["taus"], c["ps"], (1, 1), A, C, c["next_quantiles"], c["next_q"], c["actions"], c["rewards"], c["dones"],
                                      GAMMA, kappa)
        got = run_td(c, LAYOUTS["mlp"], A, C, kappa=kappa)
        gmax = max(g.abs().max().item() for g in [dx] + dw)
        assert abs(got["scal"][0].item() - scal[0].item()) <= 1e-4 * scal[0].item() and err(got["row_loss"], ql, 1e-3 * gmax) <= 3e-4
        assert max(err(g, w, 1e-3 * gmax) for g, w in zip([got["dx"]] + got["dw"], [dx] + dw)) <= 3e-4


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A, N, Np, C", SHAPES, ids=lambda v: str(v))
def test_fwd_against_fp64(B, F, A, N, Np, C, lname):
    layout = LAYOUTS[lname]
    c = td_case(B, F, A, N, Np, C, lname)
    wt, wq = I.quantiles(c["x"].double(), c["taus"], [p.double() for p in c["ps"]], layout[1], A, C)
    (th, q), _ = run_fwd(c["x"], c["taus"], c["ps"], layout, A, C)
    (th2, q2), _ = run_fwd(c["x"], c["taus"], c["ps"], layout, A, C, save=1)
    (_, q3), _ = run_fwd(c["x"], c["taus"], c["ps"], layout, A, C, outs=(0, 1))
    (th4, _), _ = run_fwd(c["x"], c["taus"], c["ps"], layout, A, C, save=1, outs=(1, 0))
    (th5, _), _ = run_fwd(c["x"], c["taus"], c["ps"], layout, A, C, outs=(1, 0))
    et, eq = err(th, wt), err(q, wq)
    log(f"iqn fwd B{B} F{F} A{A} N{N} C{C} {lname}: quantiles {et:.2e} (bound 1e-5), q {eq:.2e} (bound 1e-4)")
    assert et <= 1e-5 and eq <= 1e-4
    assert all(torch.equal(bits(th), bits(t)) for t in (th2, th4, th5)) and torch.equal(bits(q), bits(q2)) and torch.equal(bits(q), bits(q3))


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
def test_a_row_does_not_depend_on_its_position_or_on_the_batch(lname):
    """rows 0 .. 4 of the B = 37 case alone (B = 5), and at the end of the batch (other tiles, other lanes): q, the quantile values and
    row_loss bitwise"""
    layout, (B, F, A, N, Np, C) = LAYOUTS[lname], SHAPES[4]
    c = td_case(B, F, A, N, Np, C, lname)
    perm = torch.cat([torch.arange(5, B), torch.arange(5)])
    full = run_td(c, layout, A, C, True)
    head = run_td(c, layout, A, C, True, rows=torch.arange(5))
    moved = run_td(c, layout, A, C, True, rows=perm)
    (tf, qf), _ = run_fwd(c["x"], c["taus"], c["ps"], layout, A, C)
    (t5, q5), _ = run_fwd(c["x"][:5], c["taus"][:5], c["ps"], layout, A, C)
    (tm, qm), _ = run_fwd(c["x"][perm], c["taus"][perm], c["ps"], layout, A, C)
    for af, a5, am in ((qf, q5, qm), (tf, t5, tm)):
        assert torch.equal(bits(af[:5]), bits(a5)) and torch.equal(bits(am[B - 5:]), bits(a5)) and torch.equal(bits(am[:B - 5]), bits(af[5:]))
    assert torch.equal(bits(full["row_loss"][:5]), bits(head["row_loss"])) and torch.equal(bits(moved["row_loss"][B - 5:]), bits(head["row_loss"]))
    assert torch.equal(bits(moved["row_loss"][:B - 5]), bits(full["row_loss"][5:]))


# ------------------------------------------------------------------------------------------------------------ 3. the draws
def gpu_taus(seed, row_offset, B, N):
    lib, L = _lib()
    out = nanlike(B, N)
    lib.check(L.ocrl_iqn_taus(seed, row_offset, B, N, lib.ptr(out), lib.stream()))
    torch.cuda.synchronize()
    return out.cpu()


def test_the_fractions_are_the_counter_rngs():
    t = gpu_taus(7, 0, 300, 17)
    k = t.double() * 2 ** 24
    assert (k == k.round()).all() and (t >= 0).all() and (t < 1).all()                        # every value is k / 2^24 in [0, 1)
    r0 = 123
    assert torch.equal(bits(gpu_taus(7, r0, 50, 17)), bits(t[r0:r0 + 50]))                    # a pure function of (seed, row_offset + b, s)
    assert torch.equal(bits(gpu_taus(7, 0, 300, 5)), bits(t[:, :5]))                          # ... whatever N is
    assert not torch.equal(gpu_taus(8, 0, 300, 17), t) and (gpu_taus(8, 0, 300, 17) != t).float().mean() > 0.99
    assert len(set(t[0].tolist())) == 17 and len(set(t[:, 0].tolist())) == 300               # another s, another row: another value
    # the mapping the header states: group 32 R + (s >> 1) of site 450, word s & 1, its top 24 bits
    for R_, s in ((0, 0), (0, 1), (0, 16), (5, 3), (299, 16), (r0, 7)):
        x, y = R._bits(7, SITE_IQN_TAU, 0, [32 * R_ + (s >> 1)])
        assert t[R_, s].item() == float((int(y[0]) if s & 1 else int(x[0])) >> 8) / 2 ** 24, (R_, s)
    big = gpu_taus(11, 1 << 40, 4, 64)                                                        # a row past 2^32: the key's high word
    x, y = R._bits(11, SITE_IQN_TAU, ((32 << 40) + 3 * 32 + 31) >> 32, [((32 << 40) + 3 * 32 + 31) & 0xFFFFFFFF])
    assert big[3, 63].item() == float(int(y[0]) >> 8) / 2 ** 24 and big[3, 62].item() == float(int(x[0]) >> 8) / 2 ** 24
    # 2^16 draws: the mean and 16 equal bins
    u = gpu_taus(3, 0, 1024, 64).double().flatten()
    counts = torch.bincount((u * 16).long(), minlength=16)
    log(f"iqn taus: mean {u.mean().item():.4f} of 2^16 draws; bins {counts.tolist()}")
    assert abs(u.mean().item() - 0.5) <= 0.01 and ((counts - 4096).abs() <= 0.05 * 4096).all()


# ------------------------------------------------------------------------------------------------------------ 4. acting
def run_act(x, ps, layout, A, N, C, seed, row_offset, epsilon, uniforms=None, taus=None, want_q=True):
    lib, L = _lib()
    B, F = x.shape
    d = lib.iqn_desc(B, F, A, N, C, *layout)
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    u = None if uniforms is None else torch.as_tensor(uniforms).cuda().contiguous()
    ts = None if taus is None else taus.cuda().contiguous()
    actions, q = torch.full((B,), -7, device="cuda", dtype=torch.int64), nanlike(B, A) if want_q else None
    lib.check(L.ocrl_iqn_act(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), seed, row_offset, epsilon, lib.ptr(u), lib.ptr(ts), lib.ptr(actions), lib.ptr(q),
                             lib.stream()))
    torch.cuda.synchronize()
    return actions.cpu().numpy(), None if q is None else q.cpu()


@pytest.mark.parametrize("A, N", [(4, 32), (5, 17), (3, 1), (6, 64)])
def test_act_follows_the_rule(A, N):
    B, F, C, layout = 512, 12, 64, LAYOUTS["mlp"]
    gen = torch.Generator().manual_seed(5 + N)
    x, ps = torch.randn(B, F, generator=gen), I.make_params(F, A, C, layout[0], 17)
    u = (torch.randint(0, 2 ** 24, (B, 2), generator=gen).float() / 2 ** 24).numpy()
    taus = gpu_taus(3, 0, B, N)
    actions, q = run_act(x, ps, layout, A, N, C, 3, 0, 0.3, u, taus)
    want, explore = R.act_rule(q.numpy(), u, 0.3)
    assert np.array_equal(actions, want) and 0.2 < explore.mean() < 0.4
    assert set(actions[explore].tolist()) == set(range(A))
    # the restatement fed the GPU's fractions: q to the forward's bound, and the greedy action wherever its margin is above that bound
    wt, wq = I.quantiles(x.double(), taus, [p.double() for p in ps], layout[1], A, C)
    assert err(q, wq) <= 1e-4
    top = wq.topk(2, dim=1).values if A > 1 else None
    clear = ~explore & ((top[:, 0] - top[:, 1]) > 1e-3 * wq.abs().max()).numpy()
    assert clear.sum() > B // 4 and np.array_equal(actions[clear], wq.argmax(dim=1).numpy()[clear])
    (_, qf), _ = run_fwd(x, taus, ps, layout, A, C)
    assert torch.equal(bits(q), bits(qf))                                  # ocrl_iqn_act's q is ocrl_iqn_fwd's bit for bit on the same fractions
    # epsilon 0 never explores, epsilon 1 always does; without q
    greedy, _ = run_act(x, ps, layout, A, N, C, 3, 0, 0.0, u, taus, want_q=False)
    rand, _ = run_act(x, ps, layout, A, N, C, 3, 0, 1.0, u, taus)
    assert np.array_equal(greedy, q.numpy().argmax(axis=1)) and np.array_equal(rand, R.act_rule(q.numpy(), u, 1.0)[0])
    # taus = NULL draws what ocrl_iqn_taus writes, and the coin what ocrl_dqn_act_uniforms writes; a row's result does not depend on the split
    lib, L = _lib()
    du = nanlike(B, 2)
    lib.check(L.ocrl_dqn_act_uniforms(11, 1000, B, lib.ptr(du), lib.stream()))
    du = du.cpu().numpy()
    drawn = gpu_taus(11, 1000, B, N)
    whole, qw = run_act(x, ps, layout, A, N, C, 11, 1000, 0.3)
    given, qg = run_act(x, ps, layout, A, N, C, 11, 1000, 0.3, du, drawn)
    assert np.array_equal(whole, given) and torch.equal(bits(qw), bits(qg)) and np.array_equal(whole, R.act_rule(qw.numpy(), du, 0.3)[0])
    parts = [run_act(x[a:b], ps, layout, A, N, C, 11, 1000 + a, 0.3)[0] for a, b in ((0, 5), (5, 37), (37, B))]
    assert np.array_equal(np.concatenate(parts), whole)


def test_act_takes_the_lower_index_of_a_tie():
    B, F, A, N, C, layout = 64, 8, 4, 32, 64, LAYOUTS["mlp"]
    gen = torch.Generator().manual_seed(6)
    x, ps = torch.randn(B, F, generator=gen), I.make_params(F, A, C, layout[0], 18)
    ps[-2][3], ps[-1][3] = ps[-2][1] + 0.0, ps[-1][1] + 8.0                  # actions 1 and 3 identical and lifted: q[1] == q[3] bitwise, the maximum
    ps[-1][1] += 8.0
    actions, q = run_act(x, ps, layout, A, N, C, 0, 0, 0.0)
    assert torch.equal(bits(q[:, 1]), bits(q[:, 3])) and (q.argmax(dim=1) == 1).sum() > B // 2
    assert np.array_equal(actions, q.numpy().argmax(axis=1)) and 3 not in actions.tolist()


# ------------------------------------------------------------------------------------------------------------ 5. the module
def test_the_module_is_attached_to_autograd():
    from ocrl_amd import sb3s
    torch.manual_seed(3)
    pol = sb3s.DQNPolicy(types.SimpleNamespace(shape=(12,)), types.SimpleNamespace(n=3), n_tau_samples=8, n_act_samples=6, n_cos=16, net_arch=(16,)).cuda()
    net = pol.q_net
    assert type(net) is sb3s.ImplicitQuantileQNetwork
    ps = [p.detach().cpu() for p in net._param_list()]
    x = torch.randn(9, 12, device="cuda", requires_grad=True)
    mid = ((torch.arange(6.0) + 0.5) / 6).expand(9, -1)
    q = pol.q_values(x)                                                      # at the midpoints (s + 0.5) / K
    wt, wq = I.quantiles(x.detach().cpu().double(), mid, [p.double() for p in ps], (1,), 3, 16)
    theta, qd = net.quantiles(x, mid.cuda())
    assert q.shape == (9, 3) and q.requires_grad and not theta.requires_grad and not qd.requires_grad
    assert err(q, wq) <= 1e-4 and err(theta, wt) <= 1e-5 and err(qd, wq) <= 1e-4
    with torch.no_grad():
        assert torch.equal(bits(pol.q_values(x)), bits(qd))                 # nothing asks for a gradient: the kernel's own q
    (q * torch.arange(1.0, 4.0, device="cuda")).sum().backward()
    xr = x.detach().cpu().double().requires_grad_(True)
    pr = [p.double().requires_grad_(True) for p in ps]
    (I.quantiles(xr, mid, pr, (1,), 3, 16)[1] * torch.arange(1.0, 4.0, dtype=torch.float64)).sum().backward()
    gmax = max(p.grad.abs().max().item() for p in pr + [xr])
    for g, w in zip([x.grad] + [p.grad for p in net._param_list()], [xr.grad] + [p.grad for p in pr]):
        assert err(g, w, 1e-3 * gmax) <= 3e-4
    # iqn_loss is the fused step: the C ABI call's results bit for bit, and the restatement's to the TD bound
    gen = torch.Generator().manual_seed(4)
    nxt = torch.randn(9, 12, generator=gen).cuda()
    taus, taus_p = gpu_taus(1, 0, 9, 8), gpu_taus(1, 9, 9, 5)
    next_quantiles, next_q = net.quantiles(nxt, taus_p.cuda())
    a, r, d = torch.randint(0, 3, (9,), generator=gen), torch.rand(9, generator=gen) * 3, torch.rand(9, generator=gen) < 0.3
    for p in pol.parameters():
        p.grad = None
    loss, m, row_loss = sb3s.iqn_loss(pol, x.detach(), taus.cuda(), next_quantiles, next_q, a, r, d, GAMMA, kappa=0.5)
    loss.backward()
    case = dict(x=x.detach().cpu(), taus=taus, ps=ps, next_quantiles=next_quantiles.cpu(), next_q=next_q.cpu(), actions=a, rewards=r, dones=d.to(torch.uint8))
    abi = run_td(case, ((16,), (1,)), 3, 16, kappa=0.5)
    assert torch.equal(bits(loss), bits(abi["scal"][0])) and torch.equal(bits(row_loss), bits(abi["row_loss"]))
    assert all(torch.equal(bits(p.grad), bits(g)) for p, g in zip(net._param_list(), abi["dw"]))
    want = I.iqn_step(case["x"], taus, ps, (1,), 3, 16, case["next_quantiles"], case["next_q"], a, r, case["dones"], GAMMA, 0.5)
    assert set(m) == set(sb3s.dqn.DQN_SCALARS) and abs(loss.item() - want[0][0].item()) <= 1e-4 * want[0][0].item() and err(row_loss, want[3]) <= 3e-4
    gmax = max(g.abs().max().item() for g in want[2])
    for p, w in zip(net._param_list(), want[2]):
        assert err(p.grad, w, 1e-3 * gmax) <= 3e-4
    # deterministic acting takes the midpoints; exploring acting needs the policy's stream and draws from it
    actions, qa, _ = pol.act(x.detach(), row_offset=0, deterministic=True)
    assert torch.equal(actions, qa.argmax(dim=1)) and torch.equal(bits(qa), bits(qd))
    with pytest.raises(RuntimeError, match="set_sampling"):
        pol.act(x.detach(), row_offset=0)
    pol.set_sampling(21)
    _, qs, _ = pol.act(x.detach(), row_offset=40, epsilon=0.0)
    assert torch.equal(bits(qs), bits(net.quantiles(x, gpu_taus(21, 40, 9, 6).cuda())[1]))
    with pytest.raises(TypeError, match="not an ImplicitQuantileQNetwork"):
        sb3s.iqn_loss(sb3s.DQNPolicy(types.SimpleNamespace(shape=(12,)), types.SimpleNamespace(n=3)).cuda(), x.detach(), taus.cuda(), next_quantiles, next_q,
                      a, r, d, GAMMA)


# ------------------------------------------------------------------------------------------------------------ 6. DQN, 7. the loop
LOOP = ["sb3.algo_kwargs.buffer_size=64", "sb3.algo_kwargs.learning_starts=16", "sb3.algo_kwargs.train_freq=4", "sb3.algo_kwargs.target_update_interval=8",
        "sb3.algo_kwargs.batch_size=8", "+sb3.algo_kwargs.log_interval=1", "sb3.algo_kwargs.learning_rate=1e-3", "env.max_steps=6"]
UPDATES = 3
VARIANTS = {"plain": ["sb3.algo_kwargs.double_q=False", "sb3.algo_kwargs.n_step=1", "sb3.algo_kwargs.prioritized_replay=False", "sb3.algo_kwargs.noisy=False"],
            "extended": ["sb3.algo_kwargs.noisy=False"],                      # double Q + 3-step returns + prioritized replay
            "noisy": []}                                                      # ... and noisy layers: iqn.yaml as it stands


def build_loop(sb3="iqn", *over):
    import train_sb3
    from ocrl_amd.utils.config import compose
    c = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0",
                                   "env.rew_type=dense"] + LOOP + list(over))
    return train_sb3.build(c)[2]


def head_layers(policy):
    """(in, out) of the chain's Linears, the output layer included: the noisy ones (the embedding is plain)"""
    return [(m.in_features, m.out_features) for m in policy.q_net.q_net if isinstance(m, torch.nn.Linear)]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_three_updates_against_the_restatement(variant):
    """DQN(n_tau_samples=8, n_tau_prime_samples=5) on four Target environments, plain, then with double Q + n-step + prioritized replay,
    then with noisy layers too: three train_step() calls against the restatement fed the batches and the fractions the run drew; the
    priorities written back are the rows' quantile losses"""
    from ocrl_amd import sb3s
    from ocrl_amd.sb3s.iqn import TRAIN_SEED_SALT, draw_taus
    from ocrl_amd.sb3s.noisy import draw_factors
    N, Np, BS = 8, 5, 8
    model = build_loop("iqn", "sb3.algo_kwargs.n_tau_prime_samples=5", *VARIANTS[variant])
    noisy, per, n_step = variant == "noisy", variant != "plain", 1 if variant == "plain" else 3
    assert type(model.policy.q_net) is sb3s.ImplicitQuantileQNetwork and type(model.target.q_net) is sb3s.ImplicitQuantileQNetwork
    assert (model.n_tau_samples, model.n_tau_prime_samples, model.n_act_samples, model.n_cos, model.huber_kappa, model.n_atoms, model.n_quantiles,
            model.dueling, model.double_q, model.n_step, model.prioritized_replay, model.noisy) == (N, Np, 32, 64, 1.0, 1, 0, False, per, n_step, per, noisy)
    for _ in range(8):
        model.collect_step()
    buf = model.replay_buffer
    assert buf.n_slots == 16 and buf.pos == 8 and torch.equal(model.flat_target, model.flat_p) and model.policy._sample_rows == 32
    assert model.noise_draws == (8 if noisy else 0)
    ps0 = [p.detach().cpu().clone() for p in model.policy.parameters() if p.requires_grad]
    n_plain = sum(1 for _ in model.policy.features_extractor._pooling.parameters())
    acts = model.policy.q_net._layout()[1]
    layers = head_layers(model.policy)
    F = model.policy.features_dim
    assert layers[0][0] == F and layers[-1][1] == 4 and len(ps0) == n_plain + (4 if noisy else 2) * len(layers) + 2 and len(acts) == len(layers) - 1
    assert tuple(ps0[-2].shape) == (F, 64) and tuple(ps0[-1].shape) == (F,)                   # the embedding is the last module of the head
    lr = model.learning_rate
    NE = 16 * 4
    batches, taus, leaves, facs = [], [], [], []
    for u in range(UPDATES):
        if per:
            idx, w = buf.sample_prioritized(BS, model.n_updates, model.beta())               # what train_step is about to draw: a pure function
        else:
            idx, w = buf.sample_indices(BS, model.n_updates, n_step), None
        b = buf.gather(idx, n_step, model.gamma) if n_step > 1 else buf.gather(idx)
        batches.append(tuple(None if t is None else t.cpu() for t in (model._obs(b.observations), model._obs(b.next_observations), b.actions, b.rewards,
                                                                      b.dones, b.discounts, w)))
        seed = model.seed + TRAIN_SEED_SALT                                                  # the fractions, as the GPU writes them
        taus.append(tuple(draw_taus(seed, (3 * model.n_updates + k) * BS, BS, n, model.device).cpu() for k, n in ((0, N), (1, Np), (2, Np))))
        if noisy:                                                                            # the step's two draws, as the GPU writes them
            facs.append((draw_factors(layers, model.seed, model.noise_draws, model.device)[1].cpu(),
                         draw_factors(layers, model.seed + 1, model.noise_draws + 1, model.device)[1].cpu()))
        model.train_step()
        if per:
            assert torch.equal(model.last_weights, w)
            leaves.append((idx.cpu().numpy(), X.parse_store(buf.priorities.cpu().numpy(), NE)[0]))
    assert model.n_updates == UPDATES and all(torch.equal(t.cpu(), p0) for t, p0 in zip(model.target.parameters(), ps0))      # the target stood still
    assert model.noise_draws == (8 + 2 * UPDATES if noisy else 0) and model.policy._sample_rows == 32                          # no acting row was spent
    assert not torch.equal(taus[0][1], taus[0][2]) and not torch.equal(taus[0][0], taus[1][0])

    def split(ps, fac=None):
        chain = list(ps[:-2]) if fac is None else Q.noisy_chain(list(ps[:-2]), n_plain, layers, fac)
        return chain[:n_plain], list(ps[-2:]) + chain[n_plain:]

    def ref(dtype):
        cur, m, v = [p.to(dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0]
        out = []
        for step, (batch, ts) in enumerate(zip(batches, taus), 1):
            fo, ft = facs[step - 1] if noisy else (None, None)
            cur, m, v, scal, ql = I.train_step(cur, ps0, m, v, step, batch, ts, acts, 4, 64, model.gamma, model.huber_kappa, model.double_q, lr,
                                               model.max_grad_norm, lambda ps, f=fo: split(ps, f), lambda ps, f=ft: split(ps, f), dtype)
            out.append((scal, ql))
        return cur, out
    p64, out64 = ref(torch.float64)
    p32, _ = ref(torch.float32)
    dev = max(((a.double() - p0.double()) - (w - p0.double())).abs().max().item() for a, w, p0 in zip(p32, p64, ps0)) / lr
    bound = 4 * dev
    got = [p.detach().cpu() for p in model.policy.parameters() if p.requires_grad]
    worst = max(((g.double() - p0.double()) - (w - p0.double())).abs().max().item() for g, w, p0 in zip(got, p64, ps0)) / lr
    log(f"iqn train_step {variant}: worst dp/lr deviation {worst:.2e}; the fp32 restatement's {dev:.2e} (bound 4 x that: {bound:.2e}, {worst / bound:.2f} of it)")
    assert all((g != p0).any() for g, p0 in zip(got, ps0)) and worst <= bound
    # the priorities written back are the rows' quantile losses: the fixed point of (ql + eps)^alpha, to row_loss's bound (3e-4) and a unit
    # of the rounding.  A transition drawn twice has two rows with fractions of their own: its priority is the larger of their losses
    for (idx, lv), (_, ql) in zip(leaves, out64):
        ql = np.array([ql.numpy()[idx == i].max() for i in idx])
        want = X.quantise64(ql, model.prioritized_replay_alpha, model.prioritized_replay_eps)
        assert (np.abs(lv[idx] - want) <= 1 + 3e-4 * want).all(), (lv[idx], want)
    st = model.train_stats()
    for i, k in enumerate(("loss", "mean_q", "mean_target")):
        want = sum(s[i].item() for s, _ in out64) / UPDATES
        assert abs(st[k] - want) <= 1e-4 * max(abs(want), 1e-3 * max(s.abs().max().item() for s, _ in out64)), (k, st[k], want)


def run_loop(total=96):
    model = build_loop()
    losses = []
    model.learn(total, callback=lambda loc: losses.append(loc["train"]["loss"]))
    return model, losses


def test_the_loop_is_reproducible_and_checkpoints_round_trip(tmp_path):
    """train_sb3.build with sb3=iqn collects and trains with finite results, twice the same; save / load round trip"""
    model, losses = run_loop()
    assert model.n_updates == 5 and model.num_timesteps == 96 and math.isnan(losses[0]) and all(math.isfinite(l) for l in losses[1:])
    assert torch.isfinite(model.flat_p).all() and all(math.isfinite(v) for v in model.train_stats().values())
    twin, losses2 = run_loop()
    assert torch.equal(twin.flat_p, model.flat_p) and torch.equal(twin.flat_v, model.flat_v) and torch.equal(twin.flat_target, model.flat_target)
    assert torch.equal(twin.replay_buffer.priorities, model.replay_buffer.priorities) and losses2[1:] == losses[1:]
    path = str(tmp_path / "iqn.pt")
    obs = model._last_obs.clone()
    before = model.predict(obs, deterministic=True)[0]
    assert np.array_equal(model.predict(obs, deterministic=True)[0], before)                  # the midpoints: evaluation spends no draw
    model.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert {k: ck["hyper"][k] for k in ("n_tau_samples", "n_tau_prime_samples", "n_act_samples", "n_cos", "huber_kappa", "n_atoms", "n_quantiles", "dueling",
                                        "noisy")} == dict(n_tau_samples=8, n_tau_prime_samples=8, n_act_samples=32, n_cos=64, huber_kappa=1.0, n_atoms=1,
                                                          n_quantiles=0, dueling=False, noisy=True)
    F = model.policy.features_dim
    assert ck["policy"]["q_net.tau_embedding.weight"].shape == (F, 64) and ck["policy"]["q_net.tau_embedding.bias"].shape == (F,)
    assert ck["policy"]["q_net.q_net.4.weight"].shape == (4, 64) and "q_net.q_net.4.weight_sigma" in ck["policy"]
    other = build_loop("iqn", "seed=5")
    assert not torch.equal(other.flat_p, model.flat_p)
    assert other.load(path) is other
    for k in ("flat_p", "flat_target", "flat_m", "flat_v"):
        assert torch.equal(getattr(other, k), getattr(model, k)), k
    assert np.array_equal(other.predict(obs, deterministic=True)[0], before) and other.n_updates == 5 and other.n_tau_samples == 8
    # another head has another layout: refused by name, and left as it was
    for name, arg in (("rainbow", "n_tau_samples"), ("qrdqn", "n_quantiles")):
        cat = build_loop(name)
        keep = cat.flat_p.clone()
        with pytest.raises(ValueError, match=f"the checkpoint was written with {arg}"):
            cat.load(path)
        assert torch.equal(cat.flat_p, keep)


def test_train_sb3_and_test_sb3_run_iqn_in_child_processes(tmp_path):
    """the two entry points with sb3=iqn, as a user starts them: metrics, checkpoints, and an evaluation of the saved agent"""
    base = ["ocr=gt", "pooling=mlp", "sb3=iqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "device=cuda:0", "num_envs=4", "env.max_steps=6", "env.rew_type=dense"]
    over = base + LOOP[:6] + ["max_steps=96", "eval.freq=48", "eval.n_episodes=4", f"run_dir={tmp_path / 'run'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_sb3.py")] + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert [l["step"] for l in lines] == list(range(16, 97, 16)) and [l["train/n_updates"] for l in lines] == [0, 1, 2, 3, 4, 5]
    assert lines[0]["train/loss"] is None                                 # no update yet: NaN is written as null
    for l in lines[1:]:
        for k in ("train/loss", "train/mean_q", "train/mean_target", "train/grad_norm", "train/exploration_rate"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
        assert l["train/loss"] >= 0.0
    assert [l["step"] for l in lines if "eval/mean_reward" in l] == [48, 96]
    agent = tmp_path / "run" / "checkpoints" / "model_latest.pth"
    assert agent.exists() and (tmp_path / "run" / "checkpoints" / "model_best.pth").exists()
    ck = torch.load(str(agent), map_location="cpu", weights_only=True)
    assert ck["algo"] == "DQN" and (ck["hyper"]["n_tau_samples"], ck["hyper"]["n_act_samples"], ck["hyper"]["n_cos"], ck["hyper"]["dueling"]) == (8, 32, 64, False)
    over = base + [f"agent_checkpoint.local_file={agent}", "n_eval_episodes=4", f"run_dir={tmp_path / 'test'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "test_sb3.py")] + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(l) for l in open(tmp_path / "test" / "eval.jsonl")]
    assert len(rows) == 1 and rows[0]["episodes"] == 4 and rows[0]["env"] == "TargetN4C4S3S1Env" and math.isfinite(rows[0]["mean_reward"])
    log(f"test_sb3 sb3=iqn: {rows[0]}")


def test_no_tau_samples_is_the_scalar_head_and_never_takes_the_new_step():
    from ocrl_amd import sb3s
    model = build_loop("iqn", "sb3.algo_kwargs.n_tau_samples=0")
    plain = build_loop("rainbow", "sb3.algo_kwargs.n_atoms=1", "sb3.algo_kwargs.dueling=False")
    assert type(model.policy.q_net) is sb3s.QNetwork and type(model.target.q_net) is sb3s.QNetwork and model.n_tau_samples == 0

    def never(*a):
        raise AssertionError("the implicit quantile step ran with n_tau_samples = 0")
    model._train_step_iqn = never
    model.learn(48)
    plain.learn(48)
    assert model.n_updates == 2 and torch.equal(model.flat_p, plain.flat_p) and torch.equal(model.flat_v, plain.flat_v)
    # and with sampled fractions the step is the new one
    iqn = build_loop()
    taken = []
    step = iqn._train_step_iqn
    iqn._train_step_iqn = lambda *a: (taken.append(1), step(*a))[1]
    iqn._train_step_qr = iqn._train_step_c51 = iqn._train_step_dqn = never
    iqn.learn(48)
    assert iqn.n_updates == 2 == len(taken) and math.isfinite(iqn.train_stats()["loss"])
