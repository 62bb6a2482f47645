"""What DQN's replay extensions promise without a GPU: the fourth header (include/ocrl_hip_replay.h) parses, binds and is exported while the
three older tables stay as they were; every rejection its entry points make before a launch; the hand-worked examples of
tests/replay_ext_ref.py through its restatements; the dqn_per config; and the ValueErrors of DQN's new arguments."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import replay_ext_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
FUNCTIONS = {"ocrl_replay_sample_nstep": 10, "ocrl_replay_gather_nstep": 18, "ocrl_dqn_td_fwd_bwd_ext": 18, "ocrl_per_bytes": 1, "ocrl_per_init": 3,
             "ocrl_per_set_range": 6, "ocrl_per_update": 8, "ocrl_per_sample": 10}
DQN_FUNCTIONS = {"ocrl_qnet_desc_size", "ocrl_qnet_ws_floats", "ocrl_qnet_fwd", "ocrl_qnet_bwd", "ocrl_dqn_act", "ocrl_dqn_act_uniforms",
                 "ocrl_dqn_td_fwd_bwd", "ocrl_replay_gather", "ocrl_replay_sample"}
NEW_KWARGS = dict(double_q=False, n_step=1, prioritized_replay=False, prioritized_replay_alpha=0.6, prioritized_replay_beta0=0.4,
                  prioritized_replay_beta_final=1.0, prioritized_replay_eps=1e-6)


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_replay.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {} and abi.structs == {}
    assert set(_lib.ABI_REPLAY.functions) == set(FUNCTIONS)
    L = _lib.lib()
    for name, n in FUNCTIONS.items():
        assert len(getattr(L, name).argtypes) == n, name
    assert L.ocrl_per_bytes.restype is ctypes.c_size_t and L.ocrl_per_update.argtypes[5] is ctypes.c_float
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_REPLAY_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text                                        # self-contained
    # the three older tables are what they were
    assert len(_lib.ABI.functions) == 146 and _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    assert set(_lib.ABI_DQN.functions) == DQN_FUNCTIONS and set(_lib.ABI_ROLLOUT.functions) == {"ocrl_task_scenes_rollout_batch"}
    assert not set(FUNCTIONS) & (set(_lib.ABI.functions) | DQN_FUNCTIONS | set(_lib.ABI_ROLLOUT.functions))
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    for part in ("replay_ext.hip", "replay_ext_unit.o", "replay_ext.h", "ocrl_hip_replay.h"):
        assert part in makefile, part


def test_store_size_follows_the_documented_layout():
    L = _lib.lib()
    for NE in (1, 2, 21, 64, 65, 4096, 4097, 100000, 262145, 2 ** 31 - 1):
        assert L.ocrl_per_bytes(NE) == X.store_bytes(NE), NE
    assert X.level_sizes(100000) == [1563, 25, 1] and X.store_bytes(100000) == 400000 + 8 + 8 * 1589
    assert L.ocrl_per_bytes(0) == 0 and "1 <= NE < 2^31" in last_error() and L.ocrl_per_bytes(2 ** 31) == 0


# ---- rejections before any launch
def test_arguments_are_checked_before_any_launch():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)
    d = _lib.qnet_desc(5, 8, 4, [8, 8], [1, 1])
    r = ctypes.byref(d)
    w = (ctypes.c_void_p * 6)(*[FAKE] * 6)
    hole = (ctypes.c_void_p * 6)(FAKE, FAKE, None, FAKE, FAKE, FAKE)
    bad = _lib.qnet_desc(5, 8, 65, [8], [1])
    sample = lambda **kw: (lambda a: L.ocrl_replay_sample_nstep(0, 0, a["B"], a["N"], a["E"], a["pos"], a["full"], a["n"], a["idx"], None))(
        dict(dict(B=4, N=7, E=3, pos=3, full=0, n=2, idx=p), **kw))
    gather = lambda **kw: (lambda a: L.ocrl_replay_gather_nstep(a["obs"], p, p, p, a["N"], 3, a["S"], a["n"], 0.9, a["idx"], 4, p, p, p, p, p, a["disc"], None))(
        dict(dict(obs=p, N=7, S=48, n=2, idx=p, disc=p), **kw))
    td = lambda dd=r, nq=p, ww=w, dw=w, ws=1 << 40: L.ocrl_dqn_td_fwd_bwd_ext(dd, p, ww, nq, None, p, p, p, None, None, 0.99, p, None, None, dw, p, ws, None)
    for call, msg in ((lambda: sample(idx=None), "ocrl_replay_sample_nstep: null argument"),
                      (lambda: sample(n=0), "1 <= n <= 16"),
                      (lambda: sample(n=17, N=40, pos=20), "1 <= n <= 16"),
                      (lambda: sample(n=7, full=1), "n < slots"),
                      (lambda: sample(n=9, full=1), "n < slots"),
                      (lambda: sample(n=4), "pos >= n while the ring is not full"),
                      (lambda: sample(pos=7, full=1), "0 <= pos < slots"),
                      (lambda: sample(N=1), "slots >= 2"),
                      (lambda: gather(idx=None), "ocrl_replay_gather_nstep: null argument"),
                      (lambda: gather(disc=None), "ocrl_replay_gather_nstep: null argument"),
                      (lambda: gather(n=0), "1 <= n <= 16"),
                      (lambda: gather(n=17, N=40), "1 <= n <= 16"),
                      (lambda: gather(n=7), "n < slots"),
                      (lambda: gather(S=46), "multiple of 4"),
                      (lambda: gather(obs=ctypes.c_void_p(FAKE + 4)), "16-byte aligned"),
                      (lambda: td(dd=None), "ocrl_dqn_td_fwd_bwd_ext: null descriptor"),
                      (lambda: td(dd=ctypes.byref(bad)), "1 <= n_actions <= 64"),
                      (lambda: td(nq=None), "ocrl_dqn_td_fwd_bwd_ext: null argument"),
                      (lambda: td(dw=hole), "parameter pointer 2 of 6 is null"),
                      (lambda: td(ws=8), "workspace too small"),
                      (lambda: L.ocrl_per_init(None, 21, None), "ocrl_per_init: null argument"),
                      (lambda: L.ocrl_per_init(p, 0, None), "1 <= NE < 2^31"),
                      (lambda: L.ocrl_per_init(ctypes.c_void_p(FAKE + 4), 21, None), "8-byte aligned"),
                      (lambda: L.ocrl_per_set_range(p, 0, 0, 1, 0, None), "1 <= NE < 2^31"),
                      (lambda: L.ocrl_per_set_range(p, 21, 20, 2, 0, None), "inside [0, NE)"),
                      (lambda: L.ocrl_per_set_range(p, 21, -1, 2, 0, None), "inside [0, NE)"),
                      (lambda: L.ocrl_per_set_range(p, 21, 0, 0, 0, None), "inside [0, NE)"),
                      (lambda: L.ocrl_per_set_range(p, 21, 0, 4, 2, None), "mode 0"),
                      (lambda: L.ocrl_per_update(p, 21, None, p, 4, 0.6, 1e-6, None), "ocrl_per_update: null argument"),
                      (lambda: L.ocrl_per_update(p, 0, p, p, 4, 0.6, 1e-6, None), "1 <= NE < 2^31"),
                      (lambda: L.ocrl_per_update(p, 21, p, p, 0, 0.6, 1e-6, None), "batch >= 1"),
                      (lambda: L.ocrl_per_update(p, 21, p, p, 4, 1.5, 1e-6, None), "0 <= alpha <= 1"),
                      (lambda: L.ocrl_per_sample(p, 21, 0, 0, 4, 0.4, None, None, p, None), "ocrl_per_sample: null argument"),
                      (lambda: L.ocrl_per_sample(p, 0, 0, 0, 4, 0.4, None, p, p, None), "1 <= NE < 2^31"),
                      (lambda: L.ocrl_per_sample(p, 21, 0, 0, 4, -0.1, None, p, p, None), "0 <= beta <= 1")):
        assert call() != 0 and msg in last_error(), (msg, last_error())


# ---- the hand-worked examples of tests/replay_ext_ref.py
def test_three_step_return_that_stops_on_a_done():
    N, E = 5, 2
    rewards, dones = np.zeros((N, E), dtype=np.float32), np.zeros((N, E), dtype=np.uint8)
    rewards[[3, 4, 0], 1] = (1.0, 2.0, 4.0)               # the window of slot 3 wraps: slots 3, 4, 0
    dones[4, 1] = 1
    R, g, stop, m = X.nstep_walk(rewards, dones, N, E, 3, 0.5, [3 * E + 1, 4 * E + 1, 0 * E + 1, 3 * E + 0])
    assert R.tolist() == [2.0, 2.0, 4.0, 0.0] and g.tolist() == [0.25, 0.5, 0.125, 0.125] and stop.tolist() == [1, 1, 0, 0] and m.tolist() == [2, 1, 3, 3]
    assert R.dtype == np.float32 and g.dtype == np.float32
    # float32 in the written order: 0.1f * 0.99f is rounded before it is added
    rewards[:, 0] = np.float32(0.1)
    R, g, _, _ = X.nstep_walk(rewards, dones, N, E, 3, 0.99, [0])
    f = np.float32
    g1 = f(f(1) * f(0.99))
    g2 = f(g1 * f(0.99))
    assert R[0] == f(f(f(f(0) + f(0.1)) + f(g1 * f(0.1))) + f(g2 * f(0.1))) and g[0] == f(g2 * f(0.99))
    # n = 1 is the plain read
    R, g, stop, m = X.nstep_walk(rewards, dones, N, E, 1, 0.5, np.arange(N * E))
    assert np.array_equal(R, rewards.reshape(-1)) and np.array_equal(stop, dones.reshape(-1)) and set(g.tolist()) == {0.5} and set(m.tolist()) == {1}


def test_nstep_sampling_rule_keeps_to_the_whole_windows():
    for N, pos, full, n in ((7, 3, 0, 2), (7, 6, 0, 5), (7, 0, 1, 3), (7, 3, 1, 5), (7, 6, 1, 1), (7, 3, 0, 1)):
        idx = X.sample_nstep_rule(3, 9, 4096, N, 3, pos, full, n)
        assert set((idx // 3).tolist()) == X.valid_slots(N, pos, full, n) and set((idx % 3).tolist()) == {0, 1, 2}, (N, pos, full, n)
        if n == 1:
            assert np.array_equal(idx, X.sample_rule(3, 9, 4096, N, 3, pos, full))
    assert X.valid_slots(7, 3, 1, 5) == {4, 5} and X.valid_slots(7, 6, 0, 5) == {0, 1} and X.valid_slots(7, 3, 0, 2) == {0, 1}


def test_a_draw_on_a_prefix_boundary_goes_to_the_next_nonzero_leaf():
    leaves = [3, 0, 2, 5]
    assert X.search(leaves, [0, 2, 3, 4, 5, 9, 10, 2 ** 60]).tolist() == [0, 0, 2, 2, 3, 3, 3, 3]          # past the total: clamped to total - 1
    assert X.search([0, 0, 7, 0], [0, 6]).tolist() == [2, 2] and X.level_sums(leaves) == [[10]]
    big = [1] * 130
    assert X.level_sums(big) == [[64, 64, 2], [130]] and X.level_sizes(130) == [3, 1] and X.level_sizes(4097) == [65, 2, 1]
    # the draw: (w64 * total) >> 64 lies in [0, total) and is a pure function of (seed, update, row)
    t = X.draw_targets(5, 2, 4096, 10)
    assert set(t) == set(range(10)) and X.draw_targets(5, 2, 64, 10) == t[:64] and X.draw_targets(5, 3, 64, 10) != t[:64]


def test_the_fixed_point_of_a_priority():
    q = X.quantise([0.0, 1.0, 1e4, float("inf"), float("nan"), 0.5, -2.0], 1.0, 0.0)
    assert q.tolist() == [1, 65536, 1 << 24, 1 << 24, 1 << 24, 32768, 131072]
    assert X.quantise([0.0, 1.0, 1e4, float("inf")], 0.0, 1e-6).tolist() == [65536] * 4                   # alpha = 0: every priority is 1
    assert X.quantise([0.0], 1.0, 1e-6).tolist() == [1] and X.quantise([255.99], 1.0, 0.0).tolist() == [int(np.floor(np.float32(255.99) * 65536 + 0.5))]
    a = np.abs(np.random.default_rng(0).normal(size=200)).astype(np.float32) * 3
    q32, q64 = X.quantise(a, 0.6, 1e-6), X.quantise64(a, 0.6, 1e-6)
    assert (np.abs(q32 - q64) <= 1 + q64 * 2.0 ** -20).all() and (np.abs(X.quantise(a, 1.0, 1e-6) - X.quantise64(a, 1.0, 1e-6)) <= 1).all()
    w = X.weights_rule([65536, 131072, 65536 * 4], 0.5)
    assert w.dtype == np.float32 and w[0] == 1.0 and abs(w[1] - 0.5 ** 0.5) < 1e-7 and abs(w[2] - 0.5) < 1e-7
    assert X.weights_rule([7, 9, 1 << 24], 0.0).tolist() == [1.0, 1.0, 1.0] and X.weights_rule([3, 6], 1.0).tolist() == [1.0, 0.5]


def test_the_extended_td_rule_on_a_worked_batch():
    """three rows, gamma 0.5: the online maximum differs from the target's (row 0), a tie takes the lowest index (row 1), a done row ignores
    its infinite next_q (row 2)"""
    q = torch.tensor([[0.0, 1.5], [2.0, 0.0], [7.0, 4.0]], dtype=torch.float64)
    next_q = torch.tensor([[1.0, 2.0], [3.0, 5.0], [float("inf"), 1e30]], dtype=torch.float64)
    online = torch.tensor([[9.0, 0.0], [4.0, 4.0], [0.0, 1.0]], dtype=torch.float64)
    actions, rewards, dones = torch.tensor([1, 0, 0]), torch.tensor([0.0, 1.0, 5.0], dtype=torch.float64), torch.tensor([0, 0, 1], dtype=torch.uint8)
    loss, mq, my, ad = X.td_loss_ext(q, next_q, actions, rewards, dones, 0.5, next_q_online=online)
    assert ad.tolist() == [1.0, 0.5, 2.0] and my.item() == pytest.approx((0.5 + 2.5 + 5.0) / 3)        # y = 0.5 * 1, 1 + 0.5 * 3, 5
    assert loss.item() == pytest.approx((0.5 + 0.125 + 1.5) / 3)
    plain = X.td_loss_ext(q, next_q, actions, rewards, dones, 0.5)
    assert plain[3].tolist() == [0.5, 1.5, 2.0]                                                        # y = 0.5 * 2, 1 + 0.5 * 5, 5
    disc = torch.tensor([0.25, 1.0, 0.5], dtype=torch.float64)
    wts = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)
    loss, _, my, ad = X.td_loss_ext(q, next_q, actions, rewards, dones, 0.5, discounts=disc, weights=wts)
    assert ad.tolist() == [1.0, 4.0, 2.0] and loss.item() == pytest.approx((0.5 + 0.5 * 3.5 + 0.25 * 1.5) / 3)


# ---- config and the algorithm's arguments
def test_dqn_per_config_composes_and_its_kwargs_are_dqns():
    from ocrl_amd import sb3s
    base, per = compose(os.path.join(CFG, "sb3"), "dqn").to_dict(), compose(os.path.join(CFG, "sb3"), "dqn_per").to_dict()
    assert per["name"] == "DQN"
    extra = dict(NEW_KWARGS, double_q=True, n_step=3, prioritized_replay=True)
    assert per["algo_kwargs"] == dict(base["algo_kwargs"], **extra)
    params = inspect.signature(sb3s.DQN.__init__).parameters
    assert set(per["algo_kwargs"]) <= set(params) and {k: params[k].default for k in NEW_KWARGS} == NEW_KWARGS
    assert set(NEW_KWARGS) <= set(sb3s.DQN.HYPER)
    full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=dqn_per", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
    assert full.sb3.to_dict() == per
    comment = open(os.path.join(CFG, "sb3", "dqn_per.yaml")).read()
    assert "4 bytes per transition" in comment and str(4 * 100000) in comment
    rp = inspect.signature(sb3s.ReplayBuffer.__init__).parameters
    assert rp["prioritized"].default is False and rp["n_step"].default == 1
    lp = inspect.signature(sb3s.dqn_loss).parameters
    assert [lp[k].default for k in ("next_q_online", "discounts", "weights", "return_abs_td")] == [None, None, None, False]


@pytest.mark.parametrize("kw, name", [(dict(n_step=0), "n_step"), (dict(n_step=17), "n_step"), (dict(n_step=4, buffer_size=8), "n_step"),
                                      (dict(prioritized_replay_alpha=1.5), "prioritized_replay_alpha"), (dict(prioritized_replay_alpha=-0.1), "prioritized_replay_alpha"),
                                      (dict(prioritized_replay_beta0=1.2), "prioritized_replay_beta0"),
                                      (dict(prioritized_replay_beta_final=-1), "prioritized_replay_beta_final")])
def test_bad_values_name_their_argument(kw, name):
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env = types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=4))
    with pytest.raises(ValueError, match=name):
        DQN(DQNPolicy, env, **kw)                            # buffer_size 8 of 2 environments: 4 slots, so n_step = 4 does not fit


def test_replay_buffer_counts_whole_windows_on_the_cpu():
    from ocrl_amd.sb3s import ReplayBuffer
    N, E = 5, 3
    buf = ReplayBuffer(N * E, E, (4,), device="cpu", n_step=3)
    step = lambda k: buf.add(torch.full((E, 4), float(k)), torch.full((E, 4), float(k + 1)), torch.zeros(E), torch.zeros(E), torch.zeros(E))
    counts = []
    for k in range(7):
        step(k)
        counts.append(len(buf))
    assert counts == [0, 0, 3, 6, 6, 6, 6]                 # pos 1, 2 hold no window of 3; pos 3, 4 hold 1, 2 slots; full: N - 3 slots
    with pytest.raises(ValueError, match="n_step"):
        ReplayBuffer(N * E, E, (4,), device="cpu", n_step=5)
    with pytest.raises(RuntimeError, match="lives on the GPU"):
        ReplayBuffer(N * E, E, (4,), device="cpu", prioritized=True)
