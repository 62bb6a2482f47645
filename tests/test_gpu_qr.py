"""GPU checks of DQN's quantile head: the entry points of include/ocrl_hip_qr.h through the C ABI, ``DQN._train_step_qr``, checkpoints and
the entry points, against the fp64 restatement of tests/qr_ref.py.

Bounds.  The TD step carries those tests/test_gpu_c51.py::test_td_step_against_fp64 applies to the same tile arithmetic: scalars 1e-4
relative with a floor of 1e-3 of the largest scalar, every gradient and row_loss 3e-4 of its tensor's maximum with a floor of 1e-3 of the
largest gradient.  They are dominated by the shared chain and fold: the quantile loss alone is sums of at most 64 x 64 products of fp32
numbers, and it and its gradient are continuous at u = 0 and |u| = kappa, so a pair that lands on the other side of a decision in fp32
moves the result by no more than the rounding that put it there.  The generic path (ocrl_qr_fwd with save, torch autograd on its quantile
values, ocrl_qr_bwd) meets the same bound.  The forward's quantile values are a Linear chain's outputs: within 1e-5 of the largest
(test_qnet_fwd_against_fp64's bound); q, a mean of them, 1e-4.  The integer rules (actions) are exact.  ``train_step()`` is graded on
dp / lr, elementwise, against the fp64 restatement fed the batches the run drew; the bound is the one of
test_gpu_c51.py::test_three_updates_against_the_restatement: 4 x the largest deviation of the fp32 torch restatement from the fp64 one on
the very inputs of the test, measured by the test itself on the CPU.  With ``noisy`` both restatements are fed the factors the GPU drew
(tests/test_gpu_noisy.py checks those on their own)."""
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
from tests import qr_ref as Q
from tests import replay_ext_ref as X
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
SHAPES = [(1, 4, 1, 1), (5, 8, 2, 5), (16, 8, 3, 50), (17, 12, 3, 50), (37, 128, 4, 51), (33, 12, 4, 64), (20, 12, 64, 4), (1040, 8, 4, 11)]
LAYOUTS = {"none": ((), ()), "mlp": ((64, 64), (1, 1)), "tanh": ((4,), (2,))}
GAMMA, KAPPA = 0.9, 1.0


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


# ------------------------------------------------------------------------------------------------------------ 1. the TD step, 2. the forward
@functools.lru_cache(maxsize=None)
def td_case(B, F, A, N, lname, dueling):
    """the inputs of a case on the CPU, built once: every third row done with next_quantiles = NaN and next_q = inf there, two actions
    outside [0, A), rewards 6 / -6 on rows 2 .. 4 (every u above kappa, below -kappa; not done, not done, done), and per-row discounts and
    weights"""
    dims, _ = LAYOUTS[lname]
    gen = torch.Generator().manual_seed(211 + B + N)
    ps = Q.make_params(F, A, N, dims, dueling, 79)
    x = torch.randn(B, F, generator=gen)
    next_quantiles = torch.randn(B, A, N, generator=gen) * 2
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
    return dict(x=x, ps=ps, next_quantiles=next_quantiles, next_q=next_q, actions=actions, rewards=rewards, dones=dones, discounts=discounts,
                weights=weights)


def options(case, opt):
    return (case["discounts"], case["weights"]) if opt else (None, None)


@functools.lru_cache(maxsize=None)
def td_ref(B, F, A, N, lname, dueling, opt):
    c = td_case(B, F, A, N, lname, dueling)
    disc, wts = options(c, opt)
    return Q.qr_step(c["x"], c["ps"], LAYOUTS[lname][1], A, N, dueling, c["next_quantiles"], c["next_q"], c["actions"], c["rewards"], c["dones"], GAMMA,
                     KAPPA, disc, wts)


def run_td(c, layout, A, N, dueling, opt=False, want_dx=True, rows=None, kappa=KAPPA):
    lib, L = _lib()
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    x = sel(c["x"])
    B, F = x.shape
    d = lib.qr_desc(B, F, A, N, *layout, dueling)
    n = L.ocrl_qr_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = x.cuda(), [p.cuda() for p in c["ps"]]
    disc, wts = options(c, opt)
    t = [sel(c["next_quantiles"]).cuda().contiguous(), sel(c["next_q"]).cuda().contiguous(), sel(c["actions"]).cuda().long(), sel(c["rewards"]).cuda(),
         sel(c["dones"]).cuda(), None if disc is None else sel(disc).cuda(), None if wts is None else sel(wts).cuda()]
    scal, row_loss, dw = nanlike(3), nanlike(B), [nanlike(*p.shape) for p in c["ps"]]
    dx, ws = nanlike(B, F) if want_dx else None, nanlike(n)
    lib.check(L.ocrl_qr_td_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), *[lib.ptr(v) for v in t], GAMMA, kappa, lib.ptr(scal), lib.ptr(row_loss),
                                   lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(scal=scal, row_loss=row_loss, dw=dw, dx=dx)


def run_fwd(x, ps, layout, A, N, dueling, save=0, outs=(1, 1)):
    lib, L = _lib()
    B, F = x.shape
    d = lib.qr_desc(B, F, A, N, *layout, dueling)
    n = L.ocrl_qr_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd, ws = x.cuda(), [p.cuda() for p in ps], nanlike(n)
    th, q = (nanlike(B, A, N) if outs[0] else None), (nanlike(B, A) if outs[1] else None)
    lib.check(L.ocrl_qr_fwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(th), lib.ptr(q), save, lib.ptr(ws) if save else None, n if save else 0,
                            lib.stream()))
    torch.cuda.synchronize()
    return (th, q), (d, xs, pd, ws, n)


def run_generic(c, layout, A, N, dueling, opt):
    """the same gradients without the fused step: ocrl_qr_fwd with save, dquantiles formed by torch autograd (fp32, on the CPU) from its
    quantile values, then ocrl_qr_bwd"""
    lib, L = _lib()
    (th, _), (d, xs, pd, ws, n) = run_fwd(c["x"], c["ps"], layout, A, N, dueling, save=1, outs=(1, 0))
    th = th.cpu().requires_grad_(True)
    disc, wts = options(c, opt)
    Q.qr_loss(th, c["next_quantiles"], c["next_q"], c["actions"], c["rewards"], c["dones"], GAMMA, KAPPA, disc, wts)[0].backward()
    dq = th.grad.cuda().contiguous()
    dw, dx = [nanlike(*p.shape) for p in c["ps"]], nanlike(*c["x"].shape)
    lib.check(L.ocrl_qr_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(dq), lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(dw=dw, dx=dx)


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A, N", SHAPES, ids=lambda v: str(v))
def test_td_step_against_fp64(B, F, A, N, lname, dueling):
    layout = LAYOUTS[lname]
    c = td_case(B, F, A, N, lname, dueling)
    if B > 4:                                                                                    # the inputs do what the docstring says
        theta = Q.quantiles(c["x"].double(), [p.double() for p in c["ps"]], layout[1], A, N, dueling)[0]
        for disc in (torch.full((B,), GAMMA, dtype=torch.float64), c["discounts"].double()):
            T = Q.targets(c["next_quantiles"].double(), c["next_q"].double(), c["rewards"].double(), c["dones"], disc)
            u, _ = Q.pair_terms(theta[torch.arange(B), c["actions"].clamp(0, A - 1)], T, KAPPA)
            assert (u.abs() > KAPPA).any() and (u.abs() < KAPPA).any() and (u < 0).any() and (u > 0).any()
            assert (u[2] > KAPPA).all() and (u[3] < -KAPPA).all() and (u[4] < -KAPPA).all() and c["dones"][4] and not c["dones"][2] and not c["dones"][3]
            log(f"qr td inputs B{B} N{N} {lname}: {(u.abs() > KAPPA).double().mean().item():.0%} of pairs beyond kappa, {(u < 0).double().mean().item():.0%} negative")
    for opt in (False, True):
        scal, dx, dw, ql = td_ref(B, F, A, N, lname, dueling, opt)
        got, gen = run_td(c, layout, A, N, dueling, opt), run_generic(c, layout, A, N, dueling, opt)
        tag = f"B{B} F{F} A{A} N{N} {lname} {'dueling' if dueling else 'plain'} {'disc+w' if opt else 'gamma'}"
        smax = scal.abs().max().item()
        worst_s = worst_g = worst_gen = 0.0
        for i, k in enumerate(("loss", "mean_q", "mean_target")):
            e = abs(got["scal"][i].item() - scal[i].item()) / max(abs(scal[i].item()), 1e-3 * smax, 1e-30)
            worst_s = max(worst_s, e)
            log(f"qr td {tag} {k}: got {got['scal'][i].item():.6f} want {scal[i].item():.6f} rel err {e:.2e}")
            assert e <= 1e-4, (tag, k, e, got["scal"].tolist(), scal.tolist())
        gmax = max(g.abs().max().item() for g in [dx] + dw)
        for nme, g, gg, w in zip(["dx"] + [f"dw{i}" for i in range(len(dw))], [got["dx"]] + got["dw"], [gen["dx"]] + gen["dw"], [dx] + dw):
            e, eg = err(g, w, 1e-3 * gmax), err(gg, w, 1e-3 * gmax)
            worst_g, worst_gen = max(worst_g, e), max(worst_gen, eg)
            assert e <= 3e-4 and eg <= 3e-4, (tag, nme, e, eg)
        er = err(got["row_loss"], ql, 1e-3 * gmax)
        log(f"qr td {tag}: worst scalar rel err {worst_s:.2e} (bound 1e-4), worst gradient {worst_g:.2e}, generic path {worst_gen:.2e}, "
            f"row_loss {er:.2e} (bound 3e-4)")
        assert er <= 3e-4, (tag, er)
        # without dfeatures, and again: the same bits
        nodx, again = run_td(c, layout, A, N, dueling, opt, want_dx=False), run_td(c, layout, A, N, dueling, opt)
        for other in (nodx, again):
            assert torch.equal(bits(other["scal"]), bits(got["scal"])) and torch.equal(bits(other["row_loss"]), bits(got["row_loss"]))
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(other["dw"], got["dw"]))
        assert nodx["dx"] is None and torch.equal(bits(again["dx"]), bits(got["dx"]))


def test_td_step_at_another_kappa():
    """kappa = 0.25 and 3: the threshold is an argument, not a constant"""
    B, F, A, N = SHAPES[3]
    c = td_case(B, F, A, N, "mlp", True)
    for kappa in (0.25, 3.0):
        scal, dx, dw, ql = Q.qr_step(c["x"], c["ps"], (1, 1), A, N, True, c["next_quantiles"], c["next_q"], c["actions"], c["rewards"], c["dones"], GAMMA, kappa)
        got = run_td(c, LAYOUTS["mlp"], A, N, True, kappa=kappa)
        gmax = max(g.abs().max().item() for g in [dx] + dw)
        assert abs(got["scal"][0].item() - scal[0].item()) <= 1e-4 * scal[0].item() and err(got["row_loss"], ql, 1e-3 * gmax) <= 3e-4
        assert max(err(g, w, 1e-3 * gmax) for g, w in zip([got["dx"]] + got["dw"], [dx] + dw)) <= 3e-4


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A, N", SHAPES, ids=lambda v: str(v))
def test_fwd_against_fp64(B, F, A, N, lname, dueling):
    layout = LAYOUTS[lname]
    c = td_case(B, F, A, N, lname, dueling)
    wt, wq = Q.quantiles(c["x"].double(), [p.double() for p in c["ps"]], layout[1], A, N, dueling)
    (th, q), _ = run_fwd(c["x"], c["ps"], layout, A, N, dueling)
    (th2, q2), _ = run_fwd(c["x"], c["ps"], layout, A, N, dueling, save=1)
    (_, q3), _ = run_fwd(c["x"], c["ps"], layout, A, N, dueling, outs=(0, 1))
    (th4, _), _ = run_fwd(c["x"], c["ps"], layout, A, N, dueling, save=1, outs=(1, 0))
    et, eq = err(th, wt), err(q, wq)
    log(f"qr fwd B{B} F{F} A{A} N{N} {lname} dueling={dueling}: quantiles {et:.2e} (bound 1e-5), q {eq:.2e} (bound 1e-4)")
    assert et <= 1e-5 and eq <= 1e-4
    assert torch.equal(bits(th), bits(th2)) and torch.equal(bits(th), bits(th4)) and torch.equal(bits(q), bits(q2)) and torch.equal(bits(q), bits(q3))


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
def test_a_row_does_not_depend_on_its_position_or_on_the_batch(lname, dueling):
    """rows 0 .. 4 of the B = 17 case alone (B = 5), and at the end of the batch (another tile, another lane): q, the quantile values and
    row_loss bitwise"""
    layout, (B, F, A, N) = LAYOUTS[lname], SHAPES[3]
    c = td_case(B, F, A, N, lname, dueling)
    perm = torch.cat([torch.arange(5, 17), torch.arange(5)])
    full = run_td(c, layout, A, N, dueling, True)
    head = run_td(c, layout, A, N, dueling, True, rows=torch.arange(5))
    moved = run_td(c, layout, A, N, dueling, True, rows=perm)
    (t17, q17), _ = run_fwd(c["x"], c["ps"], layout, A, N, dueling)
    (t5, q5), _ = run_fwd(c["x"][:5], c["ps"], layout, A, N, dueling)
    (tm, qm), _ = run_fwd(c["x"][perm], c["ps"], layout, A, N, dueling)
    for a17, a5, am in ((q17, q5, qm), (t17, t5, tm)):
        assert torch.equal(bits(a17[:5]), bits(a5)) and torch.equal(bits(am[12:]), bits(a5)) and torch.equal(bits(am[:12]), bits(a17[5:]))
    assert torch.equal(bits(full["row_loss"][:5]), bits(head["row_loss"])) and torch.equal(bits(moved["row_loss"][12:]), bits(head["row_loss"]))
    assert torch.equal(bits(moved["row_loss"][:12]), bits(full["row_loss"][5:]))


# ------------------------------------------------------------------------------------------------------------ 4. acting
def run_act(x, ps, layout, A, N, dueling, seed, row_offset, epsilon, uniforms=None, want_q=True):
    lib, L = _lib()
    B, F = x.shape
    d = lib.qr_desc(B, F, A, N, *layout, dueling)
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    u = None if uniforms is None else torch.as_tensor(uniforms).cuda().contiguous()
    actions, q = torch.full((B,), -7, device="cuda", dtype=torch.int64), nanlike(B, A) if want_q else None
    lib.check(L.ocrl_qr_act(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), seed, row_offset, epsilon, lib.ptr(u), lib.ptr(actions), lib.ptr(q), lib.stream()))
    torch.cuda.synchronize()
    return actions.cpu().numpy(), None if q is None else q.cpu()


@pytest.mark.parametrize("A", [4, 5])
def test_act_follows_the_rule(A):
    B, F, N, layout, dueling = 4096, 12, 50, LAYOUTS["mlp"], A == 5
    gen = torch.Generator().manual_seed(5)
    x, ps = torch.randn(B, F, generator=gen), Q.make_params(F, A, N, layout[0], dueling, 17)
    u = (torch.randint(0, 2 ** 24, (B, 2), generator=gen).float() / 2 ** 24).numpy()
    actions, q = run_act(x, ps, layout, A, N, dueling, 3, 0, 0.3, u)
    want, explore = R.act_rule(q.numpy(), u, 0.3)
    assert np.array_equal(actions, want) and 0.25 < explore.mean() < 0.35
    assert np.array_equal(actions[~explore], q.numpy().argmax(axis=1)[~explore]) and set(actions[explore].tolist()) == set(range(A))
    wt, wq = Q.quantiles(x.double(), [p.double() for p in ps], layout[1], A, N, dueling)
    assert err(q, wq) <= 1e-4
    (_, qf), _ = run_fwd(x, ps, layout, A, N, dueling)
    assert torch.equal(bits(q), bits(qf))                                  # ocrl_qr_act's q is ocrl_qr_fwd's bit for bit
    # epsilon 0 never explores, epsilon 1 always does; without q
    greedy, _ = run_act(x, ps, layout, A, N, dueling, 3, 0, 0.0, u, want_q=False)
    rand, _ = run_act(x, ps, layout, A, N, dueling, 3, 0, 1.0, u)
    assert np.array_equal(greedy, q.numpy().argmax(axis=1)) and np.array_equal(rand, R.act_rule(q.numpy(), u, 1.0)[0])
    assert np.array_equal(rand, (u[:, 1].astype(np.float64) * 2 ** 24).astype(np.int64) * A >> 24)
    # drawn uniforms: ocrl_dqn_act_uniforms keeps describing what is drawn, and a row's result does not depend on the split
    lib, L = _lib()
    du = nanlike(B, 2)
    lib.check(L.ocrl_dqn_act_uniforms(11, 1000, B, lib.ptr(du), lib.stream()))
    du = du.cpu().numpy()
    assert np.array_equal(du, R.act_uniforms(11, 1000, B))
    whole, _ = run_act(x, ps, layout, A, N, dueling, 11, 1000, 0.3)
    assert np.array_equal(whole, R.act_rule(q.numpy(), du, 0.3)[0])
    parts = [run_act(x[a:b], ps, layout, A, N, dueling, 11, 1000 + a, 0.3)[0] for a, b in ((0, 5), (5, 37), (37, B))]
    assert np.array_equal(np.concatenate(parts), whole)


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_act_takes_the_lower_index_of_a_tie(dueling):
    B, F, A, N, layout = 64, 8, 4, 50, LAYOUTS["mlp"]
    gen = torch.Generator().manual_seed(6)
    x, ps = torch.randn(B, F, generator=gen), Q.make_params(F, A, N, layout[0], dueling, 18)
    wa, ba = (ps[-4], ps[-3]) if dueling else (ps[-2], ps[-1])
    wa[3 * N:4 * N], ba[3 * N:4 * N] = wa[N:2 * N] + 0.0, ba[N:2 * N] + 0.0            # actions 1 and 3 identical: q[1] == q[3] bitwise
    ba[N:2 * N] += 8.0
    ba[3 * N:4 * N] += 8.0                                       # ... and lifted (dueling takes the mean off: a lift of 4): the maximum of the rows
    actions, q = run_act(x, ps, layout, A, N, dueling, 0, 0, 0.0)
    assert torch.equal(bits(q[:, 1]), bits(q[:, 3])) and (q.argmax(dim=1) == 1).sum() > B // 2
    assert np.array_equal(actions, q.numpy().argmax(axis=1)) and 3 not in actions.tolist()


# ------------------------------------------------------------------------------------------------------------ 5. the module
def test_the_module_is_attached_to_autograd():
    from ocrl_amd import sb3s
    torch.manual_seed(3)
    pol = sb3s.DQNPolicy(types.SimpleNamespace(shape=(12,)), types.SimpleNamespace(n=3), n_quantiles=11, dueling=True, net_arch=(16,)).cuda()
    net = pol.q_net
    assert type(net) is sb3s.QuantileQNetwork
    ps = [p.detach().cpu() for p in net._param_list()]
    x = torch.randn(9, 12, device="cuda", requires_grad=True)
    q = pol.q_values(x)
    wt, wq = Q.quantiles(x.detach().cpu().double(), [p.double() for p in ps], (1,), 3, 11, True)
    theta, qd = net.quantiles(x)
    assert q.shape == (9, 3) and q.requires_grad and not theta.requires_grad and not qd.requires_grad
    assert err(q, wq) <= 1e-4 and err(theta, wt) <= 1e-5 and err(qd, wq) <= 1e-4
    with torch.no_grad():
        assert torch.equal(bits(pol.q_values(x)), bits(qd))                 # nothing asks for a gradient: the kernel's own q
    (q * torch.arange(1.0, 4.0, device="cuda")).sum().backward()
    xr = x.detach().cpu().double().requires_grad_(True)
    pr = [p.double().requires_grad_(True) for p in ps]
    (Q.quantiles(xr, pr, (1,), 3, 11, True)[1] * torch.arange(1.0, 4.0, dtype=torch.float64)).sum().backward()
    gmax = max(p.grad.abs().max().item() for p in pr + [xr])
    for g, w in zip([x.grad] + [p.grad for p in net._param_list()], [xr.grad] + [p.grad for p in pr]):
        assert err(g, w, 1e-3 * gmax) <= 3e-4
    # qr_loss is the fused step: the C ABI call's results bit for bit, and the restatement's to the TD bound
    gen = torch.Generator().manual_seed(4)
    nxt = torch.randn(9, 12, generator=gen).cuda()
    next_quantiles, next_q = net.quantiles(nxt)
    a, r, d = torch.randint(0, 3, (9,), generator=gen), torch.rand(9, generator=gen) * 3, torch.rand(9, generator=gen) < 0.3
    for p in pol.parameters():
        p.grad = None
    loss, m, row_loss = sb3s.qr_loss(pol, x.detach(), next_quantiles, next_q, a, r, d, GAMMA, kappa=0.5)
    loss.backward()
    case = dict(x=x.detach().cpu(), ps=ps, next_quantiles=next_quantiles.cpu(), next_q=next_q.cpu(), actions=a, rewards=r, dones=d.to(torch.uint8))
    abi = run_td(case, ((16,), (1,)), 3, 11, True, kappa=0.5)
    assert torch.equal(bits(loss), bits(abi["scal"][0])) and torch.equal(bits(row_loss), bits(abi["row_loss"]))
    assert all(torch.equal(bits(p.grad), bits(g)) for p, g in zip(net._param_list(), abi["dw"]))
    want = Q.qr_step(case["x"], ps, (1,), 3, 11, True, case["next_quantiles"], case["next_q"], a, r, case["dones"], GAMMA, 0.5)
    assert set(m) == set(sb3s.dqn.DQN_SCALARS) and abs(loss.item() - want[0][0].item()) <= 1e-4 * want[0][0].item() and err(row_loss, want[3]) <= 3e-4
    assert all(abs(m[k].item() - want[0][i].item()) <= 1e-4 * max(abs(want[0][i].item()), 1e-3 * want[0].abs().max().item())
               for i, k in enumerate(sb3s.dqn.DQN_SCALARS))
    gmax = max(g.abs().max().item() for g in want[2])
    for p, w in zip(net._param_list(), want[2]):
        assert err(p.grad, w, 1e-3 * gmax) <= 3e-4
    actions, qa, _ = pol.act(x.detach(), row_offset=0, deterministic=True)
    assert torch.equal(actions, qa.argmax(dim=1)) and torch.equal(bits(qa), bits(qd))
    with pytest.raises(TypeError, match="not a QuantileQNetwork"):
        sb3s.qr_loss(sb3s.DQNPolicy(types.SimpleNamespace(shape=(12,)), types.SimpleNamespace(n=3)).cuda(), x.detach(), next_quantiles, next_q, a, r, d, GAMMA)


# ------------------------------------------------------------------------------------------------------------ 6. DQN, 7. the loop
LOOP = ["sb3.algo_kwargs.buffer_size=64", "sb3.algo_kwargs.learning_starts=16", "sb3.algo_kwargs.train_freq=4", "sb3.algo_kwargs.target_update_interval=8",
        "sb3.algo_kwargs.batch_size=8", "+sb3.algo_kwargs.log_interval=1", "sb3.algo_kwargs.learning_rate=1e-3", "env.max_steps=6"]
UPDATES = 3
NQ = 8


def build_loop(sb3="qrdqn", *over):
    import train_sb3
    from ocrl_amd.utils.config import compose
    c = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0",
                                   "env.rew_type=dense"] + LOOP + list(over))
    return train_sb3.build(c)[2]


def head_layers(policy):
    net = policy.q_net
    return [(m.in_features, m.out_features) for m in list(net.q_net) + [net.value_net] if isinstance(m, torch.nn.Linear)]


@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "noisy"])
def test_three_updates_against_the_restatement(noisy):
    """DQN(n_quantiles=8, double_q, n_step=3, prioritized_replay, dueling) on four Target environments: three train_step() calls against
    the restatement fed the batches the run drew; the priorities written back are the rows' quantile losses"""
    from ocrl_amd import sb3s
    from ocrl_amd.sb3s.noisy import draw_factors
    model = build_loop("qrdqn", f"sb3.algo_kwargs.n_quantiles={NQ}", f"sb3.algo_kwargs.noisy={noisy}")
    assert type(model.policy.q_net) is sb3s.QuantileQNetwork and type(model.target.q_net) is sb3s.QuantileQNetwork
    assert (model.n_quantiles, model.huber_kappa, model.n_atoms, model.dueling, model.double_q, model.n_step, model.prioritized_replay, model.noisy) == (
        NQ, 1.0, 1, True, True, 3, True, noisy)
    for _ in range(8):
        model.collect_step()
    buf = model.replay_buffer
    assert buf.n_slots == 16 and buf.pos == 8 and len(buf) == 6 * 4 and torch.equal(model.flat_target, model.flat_p)
    assert model.noise_draws == (8 if noisy else 0)
    ps0 = [p.detach().cpu().clone() for p in model.policy.parameters() if p.requires_grad]
    n_plain = sum(1 for _ in model.policy.features_extractor._pooling.parameters())
    acts = (1,) * (n_plain // 2) + model.policy.q_net._layout()[1]
    layers = head_layers(model.policy)
    assert layers[-2:] == [(64, 4 * NQ), (64, NQ)] and len(ps0) == n_plain + (4 if noisy else 2) * len(layers) and len(acts) == n_plain // 2 + len(layers) - 2
    lr = model.learning_rate
    NE = 16 * 4
    batches, leaves, facs = [], [], []
    for u in range(UPDATES):
        idx, w = buf.sample_prioritized(8, model.n_updates, model.beta())                # what train_step is about to draw: a pure function
        b = buf.gather(idx, 3, model.gamma)
        batches.append(tuple(t.cpu() for t in (model._obs(b.observations), model._obs(b.next_observations), b.actions, b.rewards, b.dones, b.discounts, w)))
        if noisy:                                                                        # the step's two draws, as the GPU writes them
            facs.append((draw_factors(layers, model.seed, model.noise_draws, model.device)[1].cpu(), draw_factors(layers, model.seed + 1, model.noise_draws + 1, model.device)[1].cpu()))
        model.train_step()
        assert torch.equal(model.last_weights, w)
        leaves.append((idx.cpu().numpy(), X.parse_store(buf.priorities.cpu().numpy(), NE)[0]))
    assert model.n_updates == UPDATES and all(torch.equal(t.cpu(), p0) for t, p0 in zip(model.target.parameters(), ps0))      # the target stood still
    assert model.noise_draws == (8 + 2 * UPDATES if noisy else 0)

    def ref(dtype):
        cur, m, v = [p.to(dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0]
        out = []
        for step, batch in enumerate(batches, 1):
            chains = {}
            if noisy:
                fo, ft = facs[step - 1]
                chains = dict(chain_cur=lambda ps, f=fo: Q.noisy_chain(ps, n_plain, layers, f), chain_tgt=lambda ps, f=ft: Q.noisy_chain(ps, n_plain, layers, f))
            cur, m, v, scal, ql = Q.train_step(cur, ps0, m, v, step, batch, acts, 4, NQ, True, model.gamma, model.huber_kappa, True, lr, model.max_grad_norm,
                                               dtype, **chains)
            out.append((scal, ql))
        return cur, out
    p64, out64 = ref(torch.float64)
    p32, _ = ref(torch.float32)
    dev = max(((a.double() - p0.double()) - (w - p0.double())).abs().max().item() for a, w, p0 in zip(p32, p64, ps0)) / lr
    bound = 4 * dev
    got = [p.detach().cpu() for p in model.policy.parameters() if p.requires_grad]
    worst = max(((g.double() - p0.double()) - (w - p0.double())).abs().max().item() for g, w, p0 in zip(got, p64, ps0)) / lr
    log(f"qr train_step noisy={noisy}: worst dp/lr deviation {worst:.2e}; the fp32 restatement's {dev:.2e} (bound 4 x that: {bound:.2e}, {worst / bound:.2f} of it)")
    assert all((g != p0).any() for g, p0 in zip(got, ps0)) and worst <= bound
    # the priorities written back are the rows' quantile losses: the fixed point of (ql + eps)^alpha, to row_loss's bound (3e-4) and a unit
    # of the rounding
    for (idx, lv), (_, ql) in zip(leaves, out64):
        want = X.quantise64(ql.numpy(), model.prioritized_replay_alpha, model.prioritized_replay_eps)
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
    model, losses = run_loop()
    assert model.n_updates == 5 and model.num_timesteps == 96 and math.isnan(losses[0]) and all(math.isfinite(l) for l in losses[1:])
    twin, losses2 = run_loop()
    assert torch.equal(twin.flat_p, model.flat_p) and torch.equal(twin.flat_v, model.flat_v) and torch.equal(twin.flat_target, model.flat_target)
    assert torch.equal(twin.replay_buffer.priorities, model.replay_buffer.priorities) and losses2[1:] == losses[1:]
    path = str(tmp_path / "qr.pt")
    obs = model._last_obs.clone()
    before = model.predict(obs, deterministic=True)[0]
    model.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert {k: ck["hyper"][k] for k in ("n_quantiles", "huber_kappa", "n_atoms", "dueling", "noisy")} == dict(n_quantiles=50, huber_kappa=1.0, n_atoms=1,
                                                                                                              dueling=True, noisy=True)
    assert "q_net.value_net.weight" in ck["policy"] and ck["policy"]["q_net.q_net.4.weight"].shape == (200, 64)
    other = build_loop("qrdqn", "seed=5")
    assert not torch.equal(other.flat_p, model.flat_p)
    assert other.load(path) is other
    for k in ("flat_p", "flat_target", "flat_m", "flat_v"):
        assert torch.equal(getattr(other, k), getattr(model, k)), k
    assert np.array_equal(other.predict(obs, deterministic=True)[0], before) and other.n_updates == 5 and other.huber_kappa == 1.0
    # another head has another layout: refused, and left as it was
    cat = build_loop("rainbow")
    keep = cat.flat_p.clone()
    with pytest.raises(ValueError, match="n_quantiles|Adam entries"):
        cat.load(path)
    assert torch.equal(cat.flat_p, keep)


def test_no_quantiles_is_the_scalar_head_and_never_takes_the_new_step():
    from ocrl_amd import sb3s
    model = build_loop("qrdqn", "sb3.algo_kwargs.n_quantiles=0", "sb3.algo_kwargs.dueling=False")
    plain = build_loop("rainbow", "sb3.algo_kwargs.n_atoms=1", "sb3.algo_kwargs.dueling=False")
    assert type(model.policy.q_net) is sb3s.QNetwork and type(model.target.q_net) is sb3s.QNetwork and model.n_quantiles == 0

    def never(*a):
        raise AssertionError("the quantile step ran with n_quantiles = 0")
    model._train_step_qr = never
    model.learn(48)
    plain.learn(48)
    assert model.n_updates == 2 and torch.equal(model.flat_p, plain.flat_p) and torch.equal(model.flat_v, plain.flat_v)
    # and with quantiles the step is the new one
    qr = build_loop()
    taken = []
    step = qr._train_step_qr
    qr._train_step_qr = lambda *a: (taken.append(1), step(*a))[1]
    qr._train_step_c51 = qr._train_step_dqn = never
    qr.learn(48)
    assert qr.n_updates == 2 == len(taken) and math.isfinite(qr.train_stats()["loss"])


def test_two_return_distributions_at_once_are_refused():
    with pytest.raises(ValueError, match="n_quantiles > 0 and n_atoms > 1"):
        build_loop("qrdqn", "sb3.algo_kwargs.n_atoms=51")


@pytest.mark.parametrize("option", ["sb3.algo_kwargs.n_step=1", "sb3.algo_kwargs.double_q=False", "sb3.algo_kwargs.prioritized_replay=False",
                                    "sb3.algo_kwargs.dueling=False", "sb3.algo_kwargs.noisy=False"])
def test_the_loop_with_one_extension_off(option):
    model = build_loop("qrdqn", option)
    model.learn(48)
    assert model.n_updates == 2 and math.isfinite(model.train_stats()["loss"]) and (model.last_weights is None) == option.endswith("replay=False")


# ------------------------------------------------------------------------------------------------------------ 8. the entry points
def test_train_sb3_and_test_sb3_run_qrdqn_in_child_processes(tmp_path):
    base = ["ocr=gt", "pooling=mlp", "sb3=qrdqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "device=cuda:0", "num_envs=4", "env.max_steps=6", "env.rew_type=dense"]
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
    evals = [l for l in lines if "eval/mean_reward" in l]
    assert [l["step"] for l in evals] == [48, 96]
    agent = tmp_path / "run" / "checkpoints" / "model_latest.pth"
    assert agent.exists() and (tmp_path / "run" / "checkpoints" / "model_best.pth").exists()
    ck = torch.load(str(agent), map_location="cpu", weights_only=True)
    assert ck["algo"] == "DQN" and ck["hyper"]["n_quantiles"] == 50 and ck["hyper"]["dueling"] is True and ck["hyper"]["n_atoms"] == 1
    over = base + [f"agent_checkpoint.local_file={agent}", "n_eval_episodes=4", f"run_dir={tmp_path / 'test'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "test_sb3.py")] + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(l) for l in open(tmp_path / "test" / "eval.jsonl")]
    assert len(rows) == 1 and rows[0]["episodes"] == 4 and rows[0]["env"] == "TargetN4C4S3S1Env" and math.isfinite(rows[0]["mean_reward"])
    log(f"test_sb3 sb3=qrdqn: {rows[0]}")
