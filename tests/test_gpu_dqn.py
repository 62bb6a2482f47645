"""GPU checks of DQN: the entry points of include/ocrl_hip_dqn.h through the C ABI, ``DQN.train_step()``, the loop, checkpoints and the
entry points, against the fp64 restatement of tests/dqn_ref.py.

Bounds.  The TD step carries those tests/test_gpu_a2c.py applies to the same quantities of ocrl_acnet_a2c_fwd_bwd: scalars 1e-4 with the
1e-3 floor, dw and dfeatures 3e-4 of the largest gradient with the 1e-3 floor (the Huber gradient is continuous at the threshold: no row
is excluded).  Q values: 1e-5 of the largest.  The integer rules (actions, sampled ids) and the batch read are exact.  ``train_step()`` is
graded on dp / lr, elementwise, against the fp64 restatement fed the same fp32 inputs; the bound is 4 x the largest deviation of the fp32
torch restatement from the fp64 one on the very inputs of the test, measured on a CPU and written at TRAIN_DEV below (the factor 4 is for
the different summation order of the norm and of the MFMA products)."""
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
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
# largest |dp_fp32 / lr - dp_fp64 / lr| of the restatement over every parameter after the two updates of
# test_train_step_against_the_restatement (measured on a CPU by train_deviation(): 1.43e-5 of updates that reach 2.0)
TRAIN_DEV = 1.5e-5
TRAIN_LR, TRAIN_NORM, TRAIN_GAMMA, TRAIN_UPDATES = 1e-3, 10.0, 0.99, 2


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def nanlike(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def err(got, want, floor=0.0):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert torch.isfinite(got).all(), "non-finite entries (an output the kernels did not write?)"
    return (got - want).abs().max().item() / max(want.abs().max().item(), floor, 1e-30)


# ------------------------------------------------------------------------------------------------------------ 1. the TD step, 2. the forward
SHAPES = [(1, 4, 1), (5, 8, 2), (16, 8, 3), (17, 12, 3), (37, 128, 4), (64, 12, 64), (1040, 8, 4)]
LAYOUTS = {"none": ((), ()), "mlp": ((64, 64), (1, 1)), "tanh": ((4,), (2,))}
GAMMA = 0.9


@functools.lru_cache(maxsize=None)
def td_case(B, F, A, lname):
    """(x, parameters, next_q, actions, rewards, dones) of a case on the CPU, built once: rewards scaled so that both Huber branches
    occur, every third row done with next_q = 1e30 there (and inf once), two actions outside [0, A)"""
    dims, _ = LAYOUTS[lname]
    gen = torch.Generator().manual_seed(91 + B)
    ps = R.make_params(F, A, dims, 71)
    x = torch.randn(B, F, generator=gen)
    next_q = torch.randn(B, A, generator=gen)
    actions = torch.randint(0, A, (B,), generator=gen)
    rewards = torch.randn(B, generator=gen) * 1.5
    dones = (torch.arange(B) % 3 == 1).to(torch.uint8)
    next_q[dones.bool()] = 1e30
    if B > 1:
        next_q[1, 0] = float("inf")
        actions[0], actions[-1] = -3, A + 5
    return x, ps, next_q, actions, rewards, dones


@functools.lru_cache(maxsize=None)
def td_ref(B, F, A, lname):
    x, ps, next_q, actions, rewards, dones = td_case(B, F, A, lname)
    return R.td_step(x, ps, LAYOUTS[lname][1], next_q, actions, rewards, dones, GAMMA)


def run_td(x, ps, layout, A, next_q, actions, rewards, dones, gamma, want_dx=True):
    lib, L = _lib()
    B, F = x.shape
    d = lib.qnet_desc(B, F, A, *layout)
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    t = [next_q.cuda(), actions.cuda().long(), rewards.cuda(), dones.cuda()]
    scal, dw, dx, ws = nanlike(3), [nanlike(*p.shape) for p in ps], nanlike(B, F) if want_dx else None, nanlike(n)
    lib.check(L.ocrl_dqn_td_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), *[lib.ptr(v) for v in t], gamma, lib.ptr(scal), lib.ptr(dx), lib.ptrs(dw),
                                    lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(scal=scal, dw=dw, dx=dx)


def run_fwd(x, ps, layout, A, save=0):
    lib, L = _lib()
    B, F = x.shape
    d = lib.qnet_desc(B, F, A, *layout)
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    xs, pd, q, ws = x.cuda(), [p.cuda() for p in ps], nanlike(B, A), nanlike(n)
    lib.check(L.ocrl_qnet_fwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(q), save, lib.ptr(ws) if save else None, n if save else 0, lib.stream()))
    torch.cuda.synchronize()
    return q, (d, xs, pd, ws, n)


def run_generic(x, ps, layout, A, next_q, actions, rewards, dones, gamma):
    """the same gradients without the fused step: ocrl_qnet_fwd with save, dQ formed by torch autograd from its q, then ocrl_qnet_bwd"""
    lib, L = _lib()
    q, (d, xs, pd, ws, n) = run_fwd(x, ps, layout, A, save=1)
    q = q.clone().requires_grad_(True)
    R.td_loss(q, next_q.cuda(), actions.cuda(), rewards.cuda(), dones.cuda(), gamma)[0].backward()
    dq = q.grad.contiguous()
    dw, dx = [nanlike(*p.shape) for p in ps], nanlike(*x.shape)
    lib.check(L.ocrl_qnet_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(dq), lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(dw=dw, dx=dx)


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A", SHAPES, ids=lambda v: str(v))
def test_td_step_against_fp64(B, F, A, lname):
    layout = LAYOUTS[lname]
    inp = td_case(B, F, A, lname)
    scal, dx, dw = td_ref(B, F, A, lname)
    got, gen = run_td(inp[0], inp[1], layout, A, *inp[2:], GAMMA), run_generic(inp[0], inp[1], layout, A, *inp[2:], GAMMA)
    tag = f"B{B} F{F} A{A} {lname}"
    deltas = R.q_forward(inp[0].double(), [p.double() for p in inp[1]], layout[1]).gather(1, inp[3].clamp(0, A - 1).reshape(-1, 1)).squeeze(1) \
        - R.td_target(inp[2].double(), inp[4].double(), inp[5], GAMMA)
    if B >= 16:
        assert (deltas.abs() < 1).any() and (deltas.abs() > 1).any(), tag                   # both Huber branches
    smax = scal.abs().max().item()
    worst_s = worst_g = worst_gen = 0.0
    for i, k in enumerate(("loss", "mean_q", "mean_target")):
        e = abs(got["scal"][i].item() - scal[i].item()) / max(abs(scal[i].item()), 1e-3 * smax, 1e-30)
        worst_s = max(worst_s, e)
        log(f"dqn td {tag} {k}: got {got['scal'][i].item():.6f} want {scal[i].item():.6f} rel err {e:.2e}")
        assert e <= 1e-4, (tag, k, e, got["scal"].tolist(), scal.tolist())
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    for nme, g, gg, w in zip(["dx"] + [f"dw{i}" for i in range(len(dw))], [got["dx"]] + got["dw"], [gen["dx"]] + gen["dw"], [dx] + dw):
        e, eg = err(g, w, 1e-3 * gmax), err(gg, w, 1e-3 * gmax)
        worst_g, worst_gen = max(worst_g, e), max(worst_gen, eg)
        assert e <= 3e-4 and eg <= 3e-4, (tag, nme, e, eg)
    log(f"dqn td {tag}: worst scalar rel err {worst_s:.2e} (bound 1e-4), worst gradient {worst_g:.2e}, generic path {worst_gen:.2e} (bound 3e-4)")
    # without dfeatures, and again: the same bits
    nodx, again = run_td(inp[0], inp[1], layout, A, *inp[2:], GAMMA, want_dx=False), run_td(inp[0], inp[1], layout, A, *inp[2:], GAMMA)
    assert nodx["dx"] is None and torch.equal(nodx["scal"], got["scal"]) and all(torch.equal(a, b) for a, b in zip(nodx["dw"], got["dw"]))
    assert torch.equal(again["scal"], got["scal"]) and torch.equal(again["dx"], got["dx"]) and all(torch.equal(a, b) for a, b in zip(again["dw"], got["dw"]))


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
def test_a_row_does_not_depend_on_its_position_or_on_the_batch(lname):
    """rows 0 .. 4 of the B = 17 case alone (B = 5), and at the end of the batch (another tile, another lane): q bitwise, B * dfeatures to
    1e-6 relative (1 / B is the one operation that differs)"""
    layout = LAYOUTS[lname]
    x, ps, next_q, actions, rewards, dones = td_case(17, 12, 3, lname)
    perm = torch.cat([torch.arange(5, 17), torch.arange(5)])
    full = run_td(x, ps, layout, 3, next_q, actions, rewards, dones, GAMMA)
    head = run_td(x[:5], ps, layout, 3, next_q[:5], actions[:5], rewards[:5], dones[:5], GAMMA)
    moved = run_td(x[perm], ps, layout, 3, next_q[perm], actions[perm], rewards[perm], dones[perm], GAMMA)
    q17, q5, qm = run_fwd(x, ps, layout, 3)[0], run_fwd(x[:5], ps, layout, 3)[0], run_fwd(x[perm], ps, layout, 3)[0]
    assert torch.equal(q17[:5], q5) and torch.equal(qm[12:], q5) and torch.equal(qm[:12], q17[5:])
    a, b, c = 17 * full["dx"][:5], 5 * head["dx"], 17 * moved["dx"][12:]
    scale = a.abs().max().item()
    assert scale > 0 and (a - b).abs().max().item() <= 1e-6 * scale and torch.equal(a, c)


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A", SHAPES, ids=lambda v: str(v))
def test_qnet_fwd_against_fp64(B, F, A, lname):
    layout = LAYOUTS[lname]
    x, ps = td_case(B, F, A, lname)[:2]
    want = R.q_forward(x.double(), [p.double() for p in ps], layout[1])
    q, _ = run_fwd(x, ps, layout, A)
    qs, _ = run_fwd(x, ps, layout, A, save=1)
    e = err(q, want)
    log(f"dqn qnet_fwd B{B} F{F} A{A} {lname}: rel err {e:.2e} (bound 1e-5)")
    assert e <= 1e-5 and torch.equal(q, qs)


# ------------------------------------------------------------------------------------------------------------ 3. acting
def run_act(x, ps, layout, A, seed, row_offset, epsilon, uniforms=None, want_q=True):
    lib, L = _lib()
    B, F = x.shape
    d = lib.qnet_desc(B, F, A, *layout)
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    u = None if uniforms is None else torch.as_tensor(uniforms).cuda().contiguous()
    actions, q = torch.full((B,), -7, device="cuda", dtype=torch.int64), nanlike(B, A) if want_q else None
    lib.check(L.ocrl_dqn_act(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), seed, row_offset, epsilon, lib.ptr(u), lib.ptr(actions), lib.ptr(q), lib.stream()))
    torch.cuda.synchronize()
    return actions.cpu().numpy(), None if q is None else q.cpu()


def drawn(seed, row_offset, n):
    lib, L = _lib()
    out = nanlike(n, 2)
    lib.check(L.ocrl_dqn_act_uniforms(seed, row_offset, n, lib.ptr(out), lib.stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize("A", [4, 5])
def test_act_follows_the_rule(A):
    B, F, layout = 4096, 12, LAYOUTS["mlp"]
    gen = torch.Generator().manual_seed(5)
    x, ps = torch.randn(B, F, generator=gen), R.make_params(F, A, layout[0], 17)
    u = (torch.randint(0, 2 ** 24, (B, 2), generator=gen).float() / 2 ** 24).numpy()
    actions, q = run_act(x, ps, layout, A, 3, 0, 0.3, u)
    want, explore = R.act_rule(q.numpy(), u, 0.3)
    assert np.array_equal(actions, want) and 0.25 < explore.mean() < 0.35
    assert np.array_equal(actions[~explore], q.numpy().argmax(axis=1)[~explore]) and set(actions[explore].tolist()) == set(range(A))
    assert err(q, R.q_forward(x.double(), [p.double() for p in ps], layout[1])) <= 1e-5
    assert torch.equal(q, run_fwd(x, ps, layout, A)[0].cpu())
    # epsilon 0 never explores, epsilon 1 always does; without q
    greedy, _ = run_act(x, ps, layout, A, 3, 0, 0.0, u, want_q=False)
    rand, _ = run_act(x, ps, layout, A, 3, 0, 1.0, u)
    assert np.array_equal(greedy, q.numpy().argmax(axis=1)) and np.array_equal(rand, R.act_rule(q.numpy(), u, 1.0)[0])
    assert np.array_equal(rand, (u[:, 1].astype(np.float64) * 2 ** 24).astype(np.int64) * A >> 24)
    # drawn uniforms: what _act_uniforms writes, what the restatement computes, and a row's result whatever the split
    du = drawn(11, 1000, B)
    assert np.array_equal(du, R.act_uniforms(11, 1000, B))
    whole, _ = run_act(x, ps, layout, A, 11, 1000, 0.3)
    assert np.array_equal(whole, R.act_rule(q.numpy(), du, 0.3)[0])
    parts = [run_act(x[a:b], ps, layout, A, 11, 1000 + a, 0.3)[0] for a, b in ((0, 5), (5, 37), (37, B))]
    assert np.array_equal(np.concatenate(parts), whole)
    high = drawn(11, (1 << 32) + 1000, 8)                              # past 2^32 the key's high word changes: another stream
    assert not np.array_equal(high, du[:8]) and (high >= 0).all() and (high < 1).all()


def test_act_takes_the_lower_index_of_a_tie():
    B, F, A, layout = 64, 8, 4, LAYOUTS["mlp"]
    gen = torch.Generator().manual_seed(6)
    x, ps = torch.randn(B, F, generator=gen), R.make_params(F, A, layout[0], 18)
    ps[-2][3], ps[-1][3] = ps[-2][1] + 0.0, ps[-1][1] + 0.0         # output rows 1 and 3 identical: Q[1] == Q[3] bitwise
    ps[-1][1] += 3.0
    ps[-1][3] += 3.0                                                 # ... and the maximum of most rows
    actions, q = run_act(x, ps, layout, A, 0, 0, 0.0)
    assert torch.equal(q[:, 1], q[:, 3]) and (q.argmax(dim=1) == 1).sum() > B // 2
    assert np.array_equal(actions, q.numpy().argmax(axis=1)) and 3 not in actions.tolist()


# ------------------------------------------------------------------------------------------------------------ 4. replay
@pytest.mark.parametrize("shape, dtype", [((3, 4, 4), torch.uint8), ((2, 5), torch.float32), ((3, 64, 64), torch.uint8)], ids=["S48", "S40", "S12288"])
def test_replay_gather_equals_torch_indexing(shape, dtype):
    from ocrl_amd.sb3s import ReplayBuffer
    N, E = 5, 3
    buf = ReplayBuffer(N * E, E, shape, "cuda", dtype, seed=4)
    assert buf.obs_bytes == {48: 48, 10: 40, 12288: 12288}[math.prod(shape)]
    gen = torch.Generator().manual_seed(8)
    obs = torch.randint(0, 256, (N, E, *shape), generator=gen)
    buf.observations.copy_(obs.to(dtype) if dtype == torch.uint8 else obs.float() / 7)
    buf.actions.copy_(torch.randint(0, 4, (N, E), generator=gen))
    buf.rewards.copy_(torch.randn(N, E, generator=gen))
    buf.dones.copy_(torch.randint(0, 2, (N, E), generator=gen))
    ids = torch.cat([torch.arange(N * E), torch.tensor([-4, N * E, N * E + 100, 7, 7])])          # every id, ids outside the range, a repeat
    got = buf.gather(ids.cuda())
    c = ids.clamp(0, N * E - 1).cuda()
    t, e = c // E, c % E
    assert torch.equal(got.observations, buf.observations[t, e]) and torch.equal(got.next_observations, buf.observations[(t + 1) % N, e])
    assert torch.equal(got.actions, buf.actions[t, e]) and torch.equal(got.rewards, buf.rewards[t, e]) and torch.equal(got.dones, buf.dones[t, e])
    assert got.observations.dtype == dtype and got.dones.dtype == torch.uint8 and got.observations.shape == (len(ids), *shape)
    assert torch.equal(got.next_observations[(N - 1) * E], buf.observations[0, 0])                   # slot N - 1's successor is slot 0


@pytest.mark.parametrize("pos, full, slots", [(3, 0, {0, 1, 2}), (2, 1, {0, 1, 3, 4}), (0, 1, {1, 2, 3, 4}), (4, 1, {0, 1, 2, 3}), (1, 0, {0})])
def test_replay_sample_follows_the_rule(pos, full, slots):
    lib, L = _lib()
    N, E, B = 5, 3, 4096
    idx = torch.full((B,), -1, device="cuda", dtype=torch.int64)
    lib.check(L.ocrl_replay_sample(21, 6, B, N, E, pos, full, lib.ptr(idx), lib.stream()))
    got = idx.cpu().numpy()
    assert np.array_equal(got, R.sample_rule(21, 6, B, N, E, pos, full))
    assert set((got // E).tolist()) == slots and set((got % E).tolist()) == {0, 1, 2}
    lib.check(L.ocrl_replay_sample(21, 6, 100, N, E, pos, full, lib.ptr(idx), lib.stream()))         # a pure function of (seed, update, row)
    assert np.array_equal(idx.cpu().numpy()[:100], got[:100])
    lib.check(L.ocrl_replay_sample(21, (1 << 32) + 6, 100, N, E, pos, full, lib.ptr(idx), lib.stream()))
    assert np.array_equal(idx.cpu().numpy()[:100], R.sample_rule(21, (1 << 32) + 6, 100, N, E, pos, full))


# ------------------------------------------------------------------------------------------------------------ 5. train_step()
TE, TN, TROWS, TB = 4, 6, 5, 8           # environments, slots, state rows [TROWS, 5], batch


def _gt_config():
    from ocrl_amd.utils.config import compose
    return compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", f"num_envs={TE}", "device=cuda:0",
                                      "pooling.dims=[32,16]"])


def train_inputs():
    """the transitions test 5 fills the buffer with, on the CPU: TN - 1 steps of TE environments of state rows"""
    gen = torch.Generator().manual_seed(41)
    frames = torch.rand(TN, TE, TROWS, 5, generator=gen)
    actions = torch.randint(0, 4, (TN - 1, TE), generator=gen)
    rewards = torch.randn(TN - 1, TE, generator=gen) * 2
    dones = torch.rand(TN - 1, TE, generator=gen) < 0.3
    return frames, actions, rewards, dones


def chain_params(policy):
    """the policy's trainable parameters as one chain of Linear layers (the pooling MLP, then the Q head) on the CPU"""
    return [p.detach().cpu().clone() for p in policy.parameters() if p.requires_grad]


def chain_acts(policy):
    n_pool = sum(1 for _ in policy.features_extractor._pooling.parameters()) // 2
    return (1,) * n_pool + policy.q_net._layout()[1]


def ref_train(ps, acts, batches, dtype):
    """TRAIN_UPDATES updates of the restatement on the given batches, the target network held at the initial parameters"""
    target = [p.to(dtype) for p in ps]
    cur = [p.to(dtype) for p in ps]
    m, v = [torch.zeros_like(p) for p in cur], [torch.zeros_like(p) for p in cur]
    scal = []
    for step, (obs, nxt, a, r, d) in enumerate(batches, 1):
        next_q = R.q_forward(nxt.flatten(1).to(dtype), target, acts)
        s, _, grads = R.td_step(obs.flatten(1), cur, acts, next_q, a, r, d, TRAIN_GAMMA, dtype)
        cur, m, v, _ = R.adam_update(cur, grads, m, v, step, TRAIN_LR, TRAIN_NORM)
        scal.append(s)
    return cur, scal


def ref_batches(seed):
    frames, actions, rewards, dones = train_inputs()
    out = []
    for u in range(TRAIN_UPDATES):
        idx = torch.as_tensor(R.sample_rule(seed, u, TB, TN, TE, TN - 1, 0))
        t, e = idx // TE, idx % TE
        out.append((frames[t, e], frames[t + 1, e], actions[t, e], rewards[t, e], dones[t, e]))
    return out


def train_deviation(ps, acts, seed):
    """what TRAIN_DEV records: max |dp_fp32 - dp_fp64| / lr of the restatement on the test's inputs (CPU)"""
    b = ref_batches(seed)
    p32, p64 = ref_train(ps, acts, b, torch.float32)[0], ref_train(ps, acts, b, torch.float64)[0]
    return max(((a.double() - p0.double()) - (w - p0.double())).abs().max().item() for a, w, p0 in zip(p32, p64, ps)) / TRAIN_LR


def make_dqn(seed=13, **over):
    from ocrl_amd import sb3s
    c = _gt_config()
    env = types.SimpleNamespace(num_envs=TE, observation_space=types.SimpleNamespace(shape=(TROWS, 5)), action_space=types.SimpleNamespace(n=4))
    kw = dict(learning_rate=TRAIN_LR, buffer_size=TN * TE, batch_size=TB, gamma=TRAIN_GAMMA, max_grad_norm=TRAIN_NORM, seed=seed, device="cuda:0",
              policy_kwargs=dict(config=c, features_extractor_class=sb3s.OCRExtractor, features_extractor_kwargs=dict(config=c), net_arch=(16,)))
    kw.update(over)
    dqn = sb3s.DQN(sb3s.DQNPolicy, env, **kw)
    frames, actions, rewards, dones = train_inputs()
    dqn.replay_buffer = sb3s.ReplayBuffer(TN * TE, TE, (TROWS, 5), dqn.device, torch.float32, seed)
    for t in range(TN - 1):
        dqn.replay_buffer.add(frames[t], frames[t + 1], actions[t], rewards[t], dones[t])
    return dqn


def test_train_step_against_the_restatement():
    dqn = make_dqn()
    assert all(p.data_ptr() >= dqn.flat_p.data_ptr() and p.data_ptr() < dqn.flat_p.data_ptr() + 4 * dqn.flat_p.numel() for p in dqn.policy.parameters())
    assert all(p.data_ptr() >= dqn.flat_target.data_ptr() and p.data_ptr() < dqn.flat_target.data_ptr() + 4 * dqn.flat_p.numel()
               for p in dqn.target.parameters())
    assert torch.equal(dqn.flat_target, dqn.flat_p) and dqn.replay_buffer.pos == TN - 1 and not dqn.replay_buffer.full
    ps, acts = chain_params(dqn.policy), chain_acts(dqn.policy)
    assert [tuple(p.shape) for p in ps] == [(32, 25), (32,), (16, 32), (16,), (16, 16), (16,), (4, 16), (4,)] and acts == (1, 1, 1)
    # the baseline: a copy of the same module stepped by torch autograd (the head's generic forward / backward), smooth_l1_loss,
    # clip_grad_norm_ and torch.optim.Adam, on the batches train_step samples
    import copy
    base = copy.deepcopy(dqn.target)
    for p in base.parameters():
        p.data = p.data.clone()
        p.requires_grad_(True)
    opt = torch.optim.Adam(base.parameters(), lr=TRAIN_LR, eps=1e-8)
    batches = ref_batches(dqn.seed)
    for u in range(TRAIN_UPDATES):
        got = dqn.replay_buffer.sample(TB, u)
        for g, w in zip(got, batches[u]):
            assert torch.equal(g.cpu(), w.to(g.dtype)), u                      # the batch is the restated rule's, bit for bit
        with torch.no_grad():
            next_q = dqn.target.q_values(got.next_observations)
        y = R.td_target(next_q, got.rewards, got.dones, TRAIN_GAMMA)
        q = base.q_values(got.observations).gather(1, got.actions.reshape(-1, 1)).squeeze(1)
        opt.zero_grad()
        torch.nn.functional.smooth_l1_loss(q, y).backward()
        torch.nn.utils.clip_grad_norm_(base.parameters(), TRAIN_NORM)
        opt.step()
        dqn.train_step()
    assert dqn.n_updates == TRAIN_UPDATES and dqn.adam_step == TRAIN_UPDATES and torch.equal(dqn.flat_target.cpu(), torch.cat([p.reshape(-1) for p in ps]))
    want_p, want_s = ref_train(ps, acts, batches, torch.float64)
    bound = 4 * TRAIN_DEV
    worst = worst_b = 0.0
    for i, (g, b, w, p0) in enumerate(zip(chain_params(dqn.policy), chain_params(base), want_p, ps)):
        worst = max(worst, ((g.double() - p0.double()) - (w - p0.double())).abs().max().item() / TRAIN_LR)
        worst_b = max(worst_b, ((b.double() - p0.double()) - (w - p0.double())).abs().max().item() / TRAIN_LR)
        assert (g != p0).any(), i
    log(f"dqn train_step: worst dp/lr deviation {worst:.2e}, torch-autograd baseline {worst_b:.2e} (bound {bound:.2e}, {worst / bound:.2f} of it)")
    assert worst <= bound and worst_b <= bound
    st = dqn.train_stats()
    assert set(st) == {"loss", "mean_q", "mean_target", "grad_norm", "n_updates", "exploration_rate"} and st["n_updates"] == TRAIN_UPDATES
    for i, k in enumerate(("loss", "mean_q", "mean_target")):
        want = sum(s[i].item() for s in want_s) / TRAIN_UPDATES
        assert abs(st[k] - want) <= 1e-4 * max(abs(want), 1e-3 * max(abs(s).max().item() for s in want_s)), (k, st[k], want)
    assert 0 < st["grad_norm"] < 100


# ------------------------------------------------------------------------------------------------------------ 6. the loop
LOOP = ["sb3.algo_kwargs.buffer_size=32", "sb3.algo_kwargs.learning_starts=16", "sb3.algo_kwargs.train_freq=4", "sb3.algo_kwargs.target_update_interval=8",
        "sb3.algo_kwargs.batch_size=8", "+sb3.algo_kwargs.log_interval=1", "sb3.algo_kwargs.learning_rate=1e-3", "env.max_steps=6"]


def build_loop(*over):
    import train_sb3
    from ocrl_amd.utils.config import compose
    c = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0"] + LOOP + list(over))
    env, eval_env, model = train_sb3.build(c)
    return env, model


def run_loop(total=96):
    from ocrl_amd.sb3s.dqn import exploration_schedule
    env, model = build_loop()
    assert env.render_mode == "state" and model.replay_buffer is None and model.n_steps == 4 and model.batch_size == 8
    rows = []

    def cb(loc):
        assert set(loc) == {"self", "iteration", "num_timesteps", "train", "ep_rew_mean", "ep_len_mean"}
        want = exploration_schedule((loc["num_timesteps"] - 4) / total, 1.0, 0.05, 0.1)             # set before the iteration's last step
        assert loc["train"]["exploration_rate"] == model.exploration_rate == want
        rows.append((loc["num_timesteps"], loc["train"]["n_updates"], model.n_target_updates, loc["train"]["loss"], torch.equal(model.flat_target, model.flat_p)))
    model.learn(total, callback=cb)
    return model, rows


def test_the_loop_counts_its_steps_and_is_reproducible(tmp_path):
    model, rows = run_loop()
    calls, updates, targets = R.loop_counts(96, 4, 4, 1, 16, 8)
    assert (model.n_calls, model.n_updates, model.n_target_updates) == (calls, updates, targets) == (24, 5, 12) and model.num_timesteps == 96
    assert [r[0] for r in rows] == list(range(16, 97, 16)) and [r[1] for r in rows] == [0, 1, 2, 3, 4, 5]
    assert math.isnan(rows[0][3]) and all(math.isfinite(r[3]) for r in rows[1:])                     # NaN before the first update
    assert rows[0][4] and not any(r[4] for r in rows[1:])                # every iteration ends: target update (4th call), then a gradient step
    buf = model.replay_buffer
    assert buf.n_slots == 8 and buf.full and buf.pos == 0 and buf.observations.shape == (8, 4, 5, 5) and len(model._episodes) >= 8
    model.update_target()
    assert torch.equal(model.flat_target, model.flat_p)
    model.train_step()
    assert not torch.equal(model.flat_target, model.flat_p)
    twin, rows2 = run_loop()
    twin.update_target()
    twin.train_step()
    assert torch.equal(twin.flat_p, model.flat_p) and torch.equal(twin.flat_target, model.flat_target) and torch.equal(twin.flat_v, model.flat_v)
    assert torch.equal(twin.replay_buffer.observations, buf.observations) and torch.equal(twin.replay_buffer.actions, buf.actions)
    assert [r[:3] for r in rows2] == [r[:3] for r in rows] and [r[3] for r in rows2[1:]] == [r[3] for r in rows[1:]]
    assert list(twin._episodes) == list(model._episodes) and list(twin._successes) == list(model._successes)


class HostView:
    """the same environment without ``on_device``: the algorithm then takes its host path through ``step``"""

    def __init__(self, env):
        self.env, self.num_envs, self.observation_space, self.action_space = env, env.num_envs, env.observation_space, env.action_space

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        return self.env.step(actions)


def test_the_host_path_fills_the_buffer_of_the_device_path():
    (env_d, dev), (env_h, hst) = build_loop("env.rew_type=dense"), build_loop("env.rew_type=dense")
    hst.env = HostView(env_h)
    assert getattr(dev.env, "on_device", False) and not getattr(hst.env, "on_device", False)
    dev.learn(48)
    hst.learn(48)
    a, b = dev.replay_buffer, hst.replay_buffer
    assert (a.pos, a.full) == (b.pos, b.full) == (4, True) and dev.n_updates == hst.n_updates == 2
    for k in ("observations", "actions", "rewards", "dones"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.rewards.abs().max() > 0 and a.dones.any() and torch.equal(dev.flat_p, hst.flat_p) and torch.equal(dev.flat_target, hst.flat_target)
    assert list(dev._episodes) == list(hst._episodes) and len(dev._episodes) >= 4


def test_checkpoints_round_trip_and_name_their_algorithm(tmp_path):
    from ocrl_amd.sb3s import PPO
    path = str(tmp_path / "dqn.pt")
    env_a, a = build_loop()
    a.learn(48)
    obs = a._last_obs.clone()
    before = a.predict(obs, deterministic=True)[0]                  # before the save: predict takes rows of the sampling stream
    a.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["algo"] == "DQN" and set(ck["optimizer"]) == {"m", "v", "step", "sampling_rows"} and ck["optimizer"]["step"] == a.n_updates == 2
    assert ck["hyper"]["n_calls"] == 12 and ck["hyper"]["n_updates"] == 2 and ck["hyper"]["num_timesteps"] == 48 and "replay" not in ck
    assert set(ck["policy"]) == set(ck["target"]) and any(k.startswith("q_net.q_net.") for k in ck["policy"])
    # a fresh instance whose buffer the same steps refill: loading changes nothing it had not reached itself, and both go on alike
    env_b, b = build_loop()
    b.learn(48)
    assert b.load(path) is b
    for k in ("flat_p", "flat_target", "flat_m", "flat_v"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert (b.n_calls, b.n_updates, b.adam_step, b.policy._sample_rows, b.exploration_rate) == (a.n_calls, a.n_updates, a.adam_step, a.policy._sample_rows,
                                                                                                 a.exploration_rate)
    a.learn(96)
    b.learn(96)
    assert a.n_updates == b.n_updates == 5 and torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_target, b.flat_target)
    # another initialisation takes the saved state whole, and predicts as the saved agent did
    env_c, c = build_loop("seed=5")
    assert not torch.equal(c.flat_p, torch.load(path, map_location="cuda:0", weights_only=True)["optimizer"]["m"]) and c.n_updates == 0
    c.load(path)
    assert all(torch.equal(v.cpu(), c.policy.state_dict()[k].cpu()) for k, v in ck["policy"].items())
    assert all(torch.equal(v.cpu(), c.target.state_dict()[k].cpu()) for k, v in ck["target"].items())
    assert all(p.data_ptr() >= c.flat_p.data_ptr() and p.data_ptr() < c.flat_p.data_ptr() + 4 * c.flat_p.numel() for p in c.policy.parameters())
    assert np.array_equal(c.predict(obs, deterministic=True)[0], before) and c.n_updates == 2 and c.seed == a.seed
    # each algorithm loads its own files only, and says which
    with pytest.raises(ValueError, match="was written by DQN, not by PPO"):
        PPO(_ac_policy(), types.SimpleNamespace(num_envs=4, observation_space=types.SimpleNamespace(shape=(12,)), action_space=types.SimpleNamespace(n=4)),
            n_steps=5, batch_size=10).load(path)
    ppo_path = str(tmp_path / "ppo.pt")
    torch.save({"algo": "PPO"}, ppo_path)
    before_p = c.flat_p.clone()
    with pytest.raises(ValueError, match="was written by PPO, not by DQN"):
        c.load(ppo_path)
    assert torch.equal(c.flat_p, before_p)


def _ac_policy():
    from ocrl_amd.sb3s import CustomActorCriticPolicy
    from ocrl_amd.utils.config import compose
    return CustomActorCriticPolicy(types.SimpleNamespace(shape=(12,)), types.SimpleNamespace(n=4),
                                   config=types.SimpleNamespace(sb3_acnet=compose(os.path.join(CFG, "sb3_acnet"), "mlp")))


def test_one_iteration_behind_a_frozen_slate_extractor(tmp_path):
    """64x64 frames through a pre-trained (here: freshly initialised and saved), frozen SLATE encoder: shapes only.  The two policies
    share the encoder's wrapper; a trainable one is refused."""
    import train_sb3
    from ocrl_amd import ocrs
    from ocrl_amd.utils.config import compose
    base = ["ocr=slate", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0", "sb3.algo_kwargs.buffer_size=32",
            "sb3.algo_kwargs.learning_starts=0", "sb3.algo_kwargs.batch_size=8"]
    c = compose(CFG, "train_sb3", base)
    with pytest.raises(NotImplementedError, match="stepping it from DQN is not built"):
        train_sb3.build(c)
    src = ocrs.SLATE(c.ocr, c.env)
    src.to("cuda:0")
    ckpt = str(tmp_path / "slate.pth")
    torch.save(src.save(), ckpt)
    c = compose(CFG, "train_sb3", base + [f"pooling.ocr_checkpoint.local_file={ckpt}"])
    env, _, model = train_sb3.build(c)
    assert model.target.features_extractor._ocr is model.policy.features_extractor._ocr
    assert model.target.features_extractor._pooling is not model.policy.features_extractor._pooling
    model.learn(16)
    buf = model.replay_buffer
    assert buf.observations.shape == (8, 4, 3, 64, 64) and buf.observations.dtype == torch.uint8 and buf.obs_bytes == 12288 and buf.pos == 4
    assert (model.n_calls, model.n_updates) == (4, 1) and model.flat_p.numel() == model.flat_target.numel()
    batch = buf.sample(8, 0)
    assert batch.observations.shape == (8, 3, 64, 64) and batch.next_observations.dtype == torch.uint8
    feats = model.policy.extract_features(model._obs(batch.observations))
    actions, q, _ = model.policy.act(feats, row_offset=0, deterministic=True)
    assert feats.shape == (8, 128) and q.shape == (8, 4) and actions.shape == (8,) and actions.dtype == torch.int64
    assert math.isfinite(model.train_stats()["loss"])


# ------------------------------------------------------------------------------------------------------------ 7. the entry points
def test_train_sb3_and_test_sb3_run_dqn_in_child_processes(tmp_path):
    base = ["ocr=gt", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "device=cuda:0", "num_envs=4", "env.max_steps=6", "env.rew_type=dense"]
    over = base + LOOP[:6] + ["max_steps=96", "eval.freq=48", "eval.n_episodes=4", f"run_dir={tmp_path / 'run'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_sb3.py")] + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert [l["step"] for l in lines] == list(range(16, 97, 16)) and [l["train/n_updates"] for l in lines] == [0, 1, 2, 3, 4, 5]
    assert lines[0]["train/loss"] is None                                 # no update yet: NaN is written as null
    for l in lines[1:]:
        for k in ("train/loss", "train/mean_q", "train/grad_norm", "train/exploration_rate"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
    evals = [l for l in lines if "eval/mean_reward" in l]
    assert [l["step"] for l in evals] == [48, 96]
    for l in evals:
        for k in ("eval/success_rate", "eval/mean_reward", "eval/mean_ep_length"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
    agent = tmp_path / "run" / "checkpoints" / "model_latest.pth"
    assert agent.exists() and (tmp_path / "run" / "checkpoints" / "model_best.pth").exists()
    assert torch.load(str(agent), map_location="cpu", weights_only=True)["algo"] == "DQN"
    over = base + [f"agent_checkpoint.local_file={agent}", "n_eval_episodes=4", f"run_dir={tmp_path / 'test'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "test_sb3.py")] + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(l) for l in open(tmp_path / "test" / "eval.jsonl")]
    assert len(rows) == 1 and rows[0]["episodes"] == 4 and rows[0]["env"] == "TargetN4C4S3S1Env" and math.isfinite(rows[0]["mean_reward"])
    log(f"test_sb3 sb3=dqn: {rows[0]}")
