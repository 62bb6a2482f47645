"""What DQN promises without a GPU: the second header (include/ocrl_hip_dqn.h) parses, binds and matches the compiler's layout while the
first table stays as it was; every rejection the new entry points make before a launch; the replay ring's storage and position arithmetic
on the CPU; the exploration schedule and the loop's counters; the dqn config, train_sb3.build's choices and DQN's refusals; and the
restatement of tests/dqn_ref.py against its hand-worked Huber example."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import dqn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
FUNCTIONS = {"ocrl_qnet_desc_size": 0, "ocrl_qnet_ws_floats": 1, "ocrl_qnet_fwd": 8, "ocrl_qnet_bwd": 9, "ocrl_dqn_act": 10, "ocrl_dqn_act_uniforms": 5,
             "ocrl_dqn_td_fwd_bwd": 14, "ocrl_replay_gather": 15, "ocrl_replay_sample": 9}


def header():
    return open(os.path.join(ROOT, "include", "ocrl_hip_dqn.h")).read()


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    abi = _abi.read(header())
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {}
    assert list(abi.structs) == ["ocrl_qnet_desc"] and abi.structs["ocrl_qnet_desc"].__name__ == "QnetDesc"
    assert set(_lib.ABI_DQN.functions) == set(FUNCTIONS) and _lib.QnetDesc is _lib.ABI_DQN.structs["ocrl_qnet_desc"]
    assert len(_lib.ABI.functions) == 146 and not set(_lib.ABI.functions) & set(FUNCTIONS)      # the first table is ocrl_hip.h's alone
    L = _lib.lib()
    for name, n in FUNCTIONS.items():
        assert len(getattr(L, name).argtypes) == n, name
    assert L.ocrl_qnet_desc_size.restype is ctypes.c_size_t and L.ocrl_qnet_ws_floats.restype is ctypes.c_size_t
    assert L.ocrl_qnet_desc_size() == ctypes.sizeof(_lib.QnetDesc) == 80
    assert L.ocrl_dqn_act.argtypes[0] is ctypes.POINTER(_lib.QnetDesc) and L.ocrl_dqn_act.argtypes[5] is ctypes.c_float
    # the dialect the reader takes and csrc's switch scan relies on: an #ifndef guard, no OCRL_ array length, self-contained
    text = header()
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_DQN_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip.h"' not in text and not re.search(r"\[\s*OCRL_", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_struct_layout_matches_the_compiler(tmp_path):
    """sizeof and every field's offsetof and size from a C program compiled with the Makefile's compiler, against the ctypes class"""
    cls, c = _lib.QnetDesc, "ocrl_qnet_desc"
    names = [n for n, _ in cls._fields_]
    assert names == ["B", "F", "A", "n", "dims", "acts"]
    lines = [f'    printf("{c} %zu\\n", sizeof({c}));']
    lines += [f'    printf("{c}.{n} %zu %zu\\n", offsetof({c}, {n}), sizeof((({c}*)0)->{n}));' for n in names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ocrl_hip_dqn.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    cc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)$", makefile, re.M).group(1)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    want = [f"{c} {ctypes.sizeof(cls)}"] + [f"{c}.{n} {getattr(cls, n).offset} {getattr(cls, n).size}" for n in names]
    assert out[:-1] == want and out[-1] == ""
    for part in ("dqn.hip", "dqn_unit.o", "dqn.h", "ocrl_hip_dqn.h"):
        assert part in makefile, part
    assert re.search(r"^(?:\S+ )*dqn\.o(?: \S+)*: qhead_tile\.h$", makefile, re.M) and "qhead_tile.h" in re.search(r"^HDRS = (.*)$", makefile, re.M).group(1).split()


# ---- rejections before any launch
def _entries(d):
    """every entry point that takes a descriptor, on pointers that are never read"""
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)
    w = (ctypes.c_void_p * 18)(*[FAKE] * 18)
    r = ctypes.byref(d)
    return {"ocrl_qnet_fwd": lambda: L.ocrl_qnet_fwd(r, p, w, p, 0, None, 0, None),
            "ocrl_qnet_bwd": lambda: L.ocrl_qnet_bwd(r, p, w, p, p, w, p, 1 << 40, None),
            "ocrl_dqn_act": lambda: L.ocrl_dqn_act(r, p, w, 0, 0, 0.1, None, p, None, None),
            "ocrl_dqn_td_fwd_bwd": lambda: L.ocrl_dqn_td_fwd_bwd(r, p, w, p, p, p, p, 0.99, p, None, w, p, 1 << 40, None)}


@pytest.mark.parametrize("kw, reason", [(dict(A=65), "1 <= n_actions <= 64"), (dict(A=0), "1 <= n_actions <= 64"), (dict(dims=[6]), "multiples of 4"),
                                        (dict(dims=[260]), "multiples of 4"), (dict(n=9), "at most 8 hidden layers"), (dict(B=0), "batch >= 1"),
                                        (dict(F=0), "feature_dim >= 1"), (dict(acts=[3]), "activation 0")])
def test_descriptors_outside_the_limits_are_rejected(kw, reason):
    kw = dict(dict(B=5, F=8, A=4, dims=[8], acts=[1], n=1), **kw)
    d = _lib.qnet_desc(kw["B"], kw["F"], kw["A"], kw["dims"], kw["acts"])
    d.n = kw["n"]
    assert _lib.lib().ocrl_qnet_ws_floats(ctypes.byref(d)) == 0 and reason in last_error() and "ocrl_qnet_ws_floats" in last_error()
    for name, call in _entries(d).items():
        assert call() != 0 and reason in last_error() and last_error().startswith(name), name


def test_null_pointers_and_replay_shapes_are_rejected():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)
    d = _lib.qnet_desc(5, 8, 4, [8, 8], [1, 1])
    assert L.ocrl_qnet_ws_floats(ctypes.byref(d)) > 0
    assert L.ocrl_qnet_ws_floats(None) == 0 and "null descriptor" in last_error()
    w = (ctypes.c_void_p * 6)(*[FAKE] * 6)
    hole = (ctypes.c_void_p * 6)(FAKE, FAKE, None, FAKE, FAKE, FAKE)
    r = ctypes.byref(d)
    for call, msg in ((lambda: L.ocrl_qnet_fwd(r, None, w, p, 0, None, 0, None), "ocrl_qnet_fwd: null argument"),
                      (lambda: L.ocrl_qnet_fwd(r, p, hole, p, 0, None, 0, None), "parameter pointer 2 of 6 is null"),
                      (lambda: L.ocrl_qnet_fwd(r, p, w, p, 1, p, 8, None), "workspace too small"),
                      (lambda: L.ocrl_qnet_bwd(r, p, w, None, p, w, p, 1 << 40, None), "ocrl_qnet_bwd: null argument"),
                      (lambda: L.ocrl_dqn_act(r, p, w, 0, 0, 0.1, None, None, None, None), "ocrl_dqn_act: null argument"),
                      (lambda: L.ocrl_dqn_act_uniforms(0, 0, 4, None, None), "ocrl_dqn_act_uniforms"),
                      (lambda: L.ocrl_dqn_act_uniforms(0, 0, 0, p, None), "n < 1"),
                      (lambda: L.ocrl_dqn_td_fwd_bwd(r, p, w, p, p, p, None, 0.99, p, None, w, p, 1 << 40, None), "ocrl_dqn_td_fwd_bwd: null argument"),
                      (lambda: L.ocrl_dqn_td_fwd_bwd(r, p, w, p, p, p, p, 0.99, p, None, hole, p, 1 << 40, None), "parameter pointer 2 of 6 is null"),
                      (lambda: L.ocrl_dqn_td_fwd_bwd(r, p, w, p, p, p, p, 0.99, p, None, w, p, 8, None), "workspace too small"),
                      (lambda: L.ocrl_replay_gather(p, p, p, p, 5, 3, 48, None, 4, p, p, p, p, p, None), "ocrl_replay_gather: null argument"),
                      (lambda: L.ocrl_replay_gather(p, p, p, p, 1, 3, 48, p, 4, p, p, p, p, p, None), "slots >= 2"),
                      (lambda: L.ocrl_replay_gather(p, p, p, p, 5, 3, 46, p, 4, p, p, p, p, p, None), "multiple of 4"),
                      (lambda: L.ocrl_replay_gather(ctypes.c_void_p(FAKE + 4), p, p, p, 5, 3, 48, p, 4, p, p, p, p, p, None), "16-byte aligned"),
                      (lambda: L.ocrl_replay_sample(0, 0, 4, 1, 3, 0, 1, p, None), "slots >= 2"),
                      (lambda: L.ocrl_replay_sample(0, 0, 4, 5, 3, 0, 0, p, None), "pos >= 1 while the ring is not full"),
                      (lambda: L.ocrl_replay_sample(0, 0, 4, 5, 3, 5, 1, p, None), "0 <= pos < slots"),
                      (lambda: L.ocrl_replay_sample(0, 0, 4, 5, 3, 2, 1, None, None), "ocrl_replay_sample: null argument")):
        assert call() != 0 and msg in last_error(), msg


# ---- the replay ring on the CPU
def test_replay_buffer_slots_wrap_and_successors():
    from ocrl_amd.sb3s import ReplayBuffer
    N, E = 5, 3
    buf = ReplayBuffer(N * E + 2, E, (2, 5), device="cpu", obs_dtype=torch.float32)
    assert buf.n_slots == N and buf.obs_bytes == 40 and ReplayBuffer(1, 4, (4,), device="cpu").n_slots == 2
    buf.observations.fill_(-1.0)                    # torch.empty storage: give the unwritten slots a value to compare against
    frame = lambda k: torch.full((E, 2, 5), float(k)) + torch.arange(E, dtype=torch.float32).reshape(E, 1, 1) / 10
    step = lambda k: buf.add(frame(k), frame(k + 1), torch.full((E,), k), torch.full((E,), k / 2), torch.tensor([k % 2 == 1, False, True]))
    slot_frames = lambda: [int(buf.observations[t, 0, 0, 0]) for t in range(N)]
    for k in range(3):
        step(k)
    assert (buf.pos, buf.full, len(buf)) == (3, False, 9) and slot_frames() == [0, 1, 2, 3, -1]
    assert torch.equal(buf.observations[3], frame(3)) and torch.equal(buf.observations[2], frame(2))     # the successor slot holds next_obs
    assert buf.actions[:3, 0].tolist() == [0, 1, 2] and buf.rewards[:3, 1].tolist() == [0.0, 0.5, 1.0]
    assert buf.dones[:3].tolist() == [[0, 0, 1], [1, 0, 1], [0, 0, 1]] and buf.dones.dtype == torch.uint8
    for k in range(3, 5):
        step(k)
    assert (buf.pos, buf.full, len(buf)) == (0, True, 12) and slot_frames() == [5, 1, 2, 3, 4]       # step 4's next_obs went to slot 0
    for k in range(5, 7):
        step(k)
    assert (buf.pos, buf.full) == (2, True) and slot_frames() == [5, 6, 7, 3, 4]
    assert buf.actions[:, 0].tolist() == [5, 6, 2, 3, 4] and torch.equal(buf.observations[1], frame(6))
    # every slot but pos is a transition: slot t's successor (t + 1) % N holds frame k + 1 of its own step k
    for t in (3, 4, 0, 1):
        k = int(buf.actions[t, 0])
        assert torch.equal(buf.observations[t], frame(k)) and torch.equal(buf.observations[(t + 1) % N], frame(k + 1))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        buf.sample(4, 0)
    with pytest.raises(ValueError, match="not a multiple of 4"):
        ReplayBuffer(8, 2, (3, 1, 1), device="cpu", obs_dtype=torch.uint8)


# ---- schedule and counters
def test_exploration_schedule_and_loop_counts():
    from ocrl_amd.sb3s.dqn import exploration_schedule
    loop_counts = R.loop_counts
    eps = lambda f: exploration_schedule(f, 1.0, 0.05, 0.1)
    assert eps(0.0) == 1.0 and eps(0.05) == pytest.approx(0.525) and eps(0.1) == pytest.approx(0.05) and eps(0.5) == 0.05 and eps(1.0) == 0.05
    # E = 4, train_freq = 4: an iteration is 16 timesteps; updates start after the second one (32 > 16); a target update every 8 // 4 = 2 calls
    assert loop_counts(64, 4, 4, 1, 16, 8) == (16, 3, 8)
    assert loop_counts(96, 4, 4, 1, 16, 8) == (24, 5, 12) and loop_counts(96, 4, 4, 2, 0, 10_000) == (24, 12, 0)
    assert loop_counts(20, 4, 4, 1, 0, 2) == (8, 2, 8)           # the last iteration is whole; an interval below E updates every call


# ---- config and entry points
def test_dqn_config_composes_and_build_chooses_per_algorithm():
    import train_sb3
    from ocrl_amd import sb3s
    c = compose(os.path.join(CFG, "sb3"), "dqn")
    assert c.to_dict() == {"name": "DQN", "algo_kwargs": dict(
        learning_rate=1e-4, buffer_size=100000, learning_starts=50000, batch_size=32, tau=1.0, gamma=0.99, train_freq=4, gradient_steps=1,
        target_update_interval=10000, exploration_fraction=0.1, exploration_initial_eps=1.0, exploration_final_eps=0.05, max_grad_norm=10)}
    full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
    assert full.sb3.to_dict() == c.to_dict()
    assert train_sb3.ALGOS == {"PPO": sb3s.PPO, "A2C": sb3s.A2C, "DQN": sb3s.DQN} and train_sb3.POLICIES == {"DQN": sb3s.DQNPolicy}
    assert {"DQN", "DQNPolicy", "QNetwork", "dqn_loss", "ReplayBuffer"} <= set(sb3s.__all__)
    assert sb3s.on_policy.ALGOS == ("PPO", "A2C") and not issubclass(sb3s.DQN, sb3s.on_policy.OnPolicyAlgorithm)
    sac = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "sb3.name=SAC"])
    with pytest.raises(NotImplementedError, match="SAC is not built") as e:
        train_sb3.build(sac)
    assert all(a in str(e.value) for a in ("PPO", "A2C", "DQN"))
    comment = open(os.path.join(CFG, "sb3", "dqn.yaml")).read()
    assert str(3 * 64 * 64 + 8 + 4 + 1) in comment and str(3 * 128 * 128 + 8 + 4 + 1) in comment      # bytes per transition


def test_dqn_refuses_what_it_does_not_build():
    from ocrl_amd.sb3s import DQN, DQNPolicy, QNetwork
    env = lambda space: types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=space)
    with pytest.raises(NotImplementedError, match="schedule"):
        DQN(DQNPolicy, env(types.SimpleNamespace(n=4)), learning_rate=lambda progress: 1e-4 * progress)
    with pytest.raises(ValueError, match="gradient_steps >= 1"):
        DQN(DQNPolicy, env(types.SimpleNamespace(n=4)), gradient_steps=-1)
    with pytest.raises(NotImplementedError, match="Discrete action spaces only"):
        DQN(DQNPolicy, env(types.SimpleNamespace(shape=(3,), low=-1.0, high=1.0)))
    head = QNetwork(12, 4, (64, 64), "relu")
    assert list(head.state_dict()) == [f"q_net.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias")]
    assert [tuple(v.shape) for v in head.state_dict().values()] == [(64, 12), (64,), (64, 64), (64,), (4, 64), (4,)]
    assert list(QNetwork(12, 4, (), "tanh").state_dict()) == ["q_net.0.weight", "q_net.0.bias"] and head._layout() == ((64, 64), (1, 1))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        head(torch.zeros(2, 12))


# ---- the restatement
def test_hand_worked_huber_example_holds_through_the_restatement():
    """delta = 0.5, -3, 1 (the docstring of tests/dqn_ref.py): one row bootstraps, one is done with a non-finite next_q, one sits on the
    threshold"""
    q = torch.tensor([[0.0, 1.5], [2.0, 0.0], [7.0, 4.0]], dtype=torch.float64, requires_grad=True)
    next_q = torch.tensor([[1.0, 2.0], [float("inf"), 1e30], [-1.0, 4.0]], dtype=torch.float64)
    actions, rewards, dones = torch.tensor([1, 0, 5]), torch.tensor([0.0, 5.0, 1.0], dtype=torch.float64), torch.tensor([0, 1, 0], dtype=torch.uint8)
    y = R.td_target(next_q, rewards, dones, 0.5)
    assert y.tolist() == [1.0, 5.0, 3.0]                               # the done row's infinity is selected away; action 5 clamps to 1
    loss, mq, my = R.td_loss(q, next_q, actions, rewards, dones, 0.5)
    assert loss.item() == pytest.approx((0.125 + 2.5 + 0.5) / 3, abs=1e-15) and mq.item() == pytest.approx(7.5 / 3) and my.item() == 3.0
    loss.backward()
    assert torch.allclose(q.grad, torch.tensor([[0.0, 0.5], [-1.0, 0.0], [0.0, 1.0]], dtype=torch.float64) / 3, atol=1e-15)


def test_integer_rules_of_the_restatement():
    u = R.act_uniforms(7, 100, 4096)
    assert u.shape == (4096, 2) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert np.array_equal(R.act_uniforms(7, 1100, 8), u[1000:1008]) and abs(u.mean() - 0.5) < 0.02          # a pure function of (seed, row)
    q = np.array([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 2.0, 5.0]])
    un = np.array([[0.5, 0.9], [0.29999, 0.75], [0.0, 0.999999]], dtype=np.float32)
    a, ex = R.act_rule(q, un, 0.3)
    assert a.tolist() == [1, 3, 3] and ex.tolist() == [False, True, True]                                 # lowest argmax; floor(0.75 * 4)
    assert R.act_rule(q, un, 0.0)[0].tolist() == [1, 0, 3] and R.act_rule(q, un, 1.0)[1].all()
    for full, pos, slots in ((0, 3, {0, 1, 2}), (1, 2, {0, 1, 3, 4})):
        idx = R.sample_rule(3, 9, 4096, 5, 3, pos, full)
        assert set((idx // 3).tolist()) == slots and set((idx % 3).tolist()) == {0, 1, 2}
        assert np.array_equal(R.sample_rule(3, 9, 64, 5, 3, pos, full), idx[:64]) and not np.array_equal(R.sample_rule(3, 10, 64, 5, 3, pos, full), idx[:64])
