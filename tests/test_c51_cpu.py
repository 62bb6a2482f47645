"""What DQN's categorical head promises without a GPU: the fifth header (include/ocrl_hip_c51.h) parses, binds and is exported while the
four older tables stay as they were; every rejection its entry points make before a launch; the hand-worked batch of tests/c51_ref.py and
the identities of the projection (gather form = scatter form, mass 1, the mean of the target) in fp64; the dqn_c51 config; and the
ValueErrors of DQN's new arguments."""
import ctypes
import inspect
import math
import os
import re
import types

import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import c51_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
FUNCTIONS = {"ocrl_c51_desc_size": 0, "ocrl_c51_ws_floats": 1, "ocrl_c51_fwd": 12, "ocrl_c51_bwd": 9, "ocrl_c51_act": 12, "ocrl_c51_td_fwd_bwd": 20}
DQN_FUNCTIONS = {"ocrl_qnet_desc_size", "ocrl_qnet_ws_floats", "ocrl_qnet_fwd", "ocrl_qnet_bwd", "ocrl_dqn_act", "ocrl_dqn_act_uniforms",
                 "ocrl_dqn_td_fwd_bwd", "ocrl_replay_gather", "ocrl_replay_sample"}
REPLAY_FUNCTIONS = {"ocrl_replay_sample_nstep", "ocrl_replay_gather_nstep", "ocrl_dqn_td_fwd_bwd_ext", "ocrl_per_bytes", "ocrl_per_init",
                    "ocrl_per_set_range", "ocrl_per_update", "ocrl_per_sample"}
NEW_KWARGS = dict(n_atoms=1, v_min=0.0, v_max=2.0, dueling=False)


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_c51.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {} and set(abi.structs) == {"ocrl_c51_desc"}
    assert [f[0] for f in abi.structs["ocrl_c51_desc"]._fields_] == ["B", "F", "A", "Z", "n", "dueling", "dims", "acts"]
    assert all(t in (ctypes.c_int, ctypes.c_int * 8) for _, t in abi.structs["ocrl_c51_desc"]._fields_)         # int fields only
    assert set(_lib.ABI_C51.functions) == set(FUNCTIONS)
    L = _lib.lib()
    for name, n in FUNCTIONS.items():
        assert len(getattr(L, name).argtypes) == n, name
    assert L.ocrl_c51_ws_floats.restype is ctypes.c_size_t and L.ocrl_c51_fwd.argtypes[3] is ctypes.c_float and L.ocrl_c51_td_fwd_bwd.argtypes[12] is ctypes.c_float
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_C51_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                      # self-contained
    # the four older tables are what they were
    assert len(_lib.ABI.functions) == 146 and _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    assert set(_lib.ABI_DQN.functions) == DQN_FUNCTIONS and set(_lib.ABI_ROLLOUT.functions) == {"ocrl_task_scenes_rollout_batch"}
    assert set(_lib.ABI_REPLAY.functions) == REPLAY_FUNCTIONS
    assert not set(FUNCTIONS) & (set(_lib.ABI.functions) | DQN_FUNCTIONS | REPLAY_FUNCTIONS | set(_lib.ABI_ROLLOUT.functions))
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    for part in ("c51.hip", "c51_unit.o", "c51.h", "ocrl_hip_c51.h"):
        assert part in makefile, part
    assert re.search(r"^acnet\.o .*\bc51\.o\b.*: acnet_tile\.h$", makefile, re.M) and re.search(r"^acnet\.o .*\bc51_unit\.o\b.*: acnet\.h$", makefile, re.M)
    assert re.search(r"^(?:\S+ )*c51\.o(?: \S+)*: qhead_tile\.h$", makefile, re.M) and "qhead_tile.h" in re.search(r"^HDRS = (.*)$", makefile, re.M).group(1).split()


def test_descriptor_size_is_the_ctypes_struct():
    assert _lib.lib().ocrl_c51_desc_size() == ctypes.sizeof(_lib.C51Desc) == 22 * 4
    d = _lib.c51_desc(5, 8, 4, 51, [64, 32], [1, 2], dueling=True)
    assert (d.B, d.F, d.A, d.Z, d.n, d.dueling, list(d.dims)[:3], list(d.acts)[:3]) == (5, 8, 4, 51, 2, 1, [64, 32, 0], [1, 2, 0])
    with pytest.raises(ValueError, match="at most 8 hidden layers"):
        _lib.c51_desc(5, 8, 4, 51, [4] * 9, [1] * 9)


# ---- rejections before any launch
def test_arguments_are_checked_before_any_launch():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)
    desc = lambda A=4, Z=51, dueling=True, dims=(8, 8), B=5, F=8: _lib.c51_desc(B, F, A, Z, list(dims), [1] * len(dims), dueling)
    good = desc()
    w = (ctypes.c_void_p * 8)(*[FAKE] * 8)
    hole = (ctypes.c_void_p * 8)(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE)
    big = 1 << 40

    def fwd(d=good, ww=w, vmin=0.0, vmax=2.0, outs=(p, p, p), save=0, ws=None, n=0):
        return L.ocrl_c51_fwd(ctypes.byref(d) if d is not None else None, p, ww, vmin, vmax, *outs, save, ws, n, None)

    def bwd(d=good, ww=w, dw=w, dl=p, n=big):
        return L.ocrl_c51_bwd(ctypes.byref(d), p, ww, dl, None, dw, p, n, None)

    def act(d=good, ww=w, vmin=0.0, vmax=2.0, actions=p):
        return L.ocrl_c51_act(ctypes.byref(d), p, ww, vmin, vmax, 0, 0, 0.1, None, actions, None, None)

    def td(d=good, ww=w, dw=w, vmin=0.0, vmax=2.0, np_=p, n=big):
        return L.ocrl_c51_td_fwd_bwd(ctypes.byref(d), p, ww, vmin, vmax, np_, p, p, p, p, None, None, 0.99, p, None, None, dw, p, n, None)

    limits = ((desc(A=65, Z=2), "1 <= n_actions <= 64"), (desc(Z=1), "2 <= n_atoms <= 64"), (desc(Z=65, A=2), "2 <= n_atoms <= 64"),
              (desc(A=5, Z=52), "n_actions * n_atoms <= 256"), (desc(A=0), "1 <= n_actions <= 64"), (desc(dims=(6,)), "multiples of 4"),
              (desc(dims=(260,)), "multiples of 4"), (desc(B=0), "batch >= 1"), (desc(F=0), "feature_dim >= 1"))
    assert limits[3][0].A * limits[3][0].Z == 260
    for bad, msg in limits:
        for call in (fwd, bwd, act, td):
            assert call(d=bad) != 0 and msg in last_error(), (msg, last_error())
        assert L.ocrl_c51_ws_floats(ctypes.byref(bad)) == 0 and msg in last_error()
    nine = desc()
    nine.n = 9
    for call, msg in ((lambda: fwd(d=None), "ocrl_c51_fwd: null descriptor"),
                      (lambda: fwd(d=nine), "at most 8 hidden layers"),
                      (lambda: fwd(vmin=2.0, vmax=2.0), "v_min < v_max"),
                      (lambda: fwd(vmin=3.0, vmax=2.0), "v_min < v_max"),
                      (lambda: act(vmin=0.0, vmax=float("inf")), "v_min < v_max, both finite"),
                      (lambda: td(vmin=float("nan")), "v_min < v_max, both finite"),
                      (lambda: td(vmin=1.0, vmax=1.0), "ocrl_c51_td_fwd_bwd: v_min < v_max"),
                      (lambda: fwd(outs=(None, None, None)), "logits, probs and q are all null"),
                      (lambda: fwd(ww=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: fwd(ww=None), "ocrl_c51_fwd: null argument"),
                      (lambda: fwd(save=1, ws=p, n=8), "workspace too small"),
                      (lambda: fwd(save=1, ws=None, n=big), "workspace too small"),
                      (lambda: bwd(dw=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: bwd(dl=None), "ocrl_c51_bwd: null argument"),
                      (lambda: bwd(n=8), "workspace too small"),
                      (lambda: act(ww=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: act(actions=None), "ocrl_c51_act: null argument"),
                      (lambda: td(np_=None), "ocrl_c51_td_fwd_bwd: null argument"),
                      (lambda: td(dw=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: td(n=8), "workspace too small")):
        assert call() != 0 and msg in last_error(), (msg, last_error())
    # without dueling the list is two pointers shorter: the hole at 6 is past its end
    plain = desc(dueling=False)
    six = (ctypes.c_void_p * 6)(FAKE, FAKE, FAKE, None, FAKE, FAKE)
    assert fwd(d=plain, ww=six) != 0 and "parameter pointer 3 of 6 is null" in last_error()
    # the workspace: saved layer outputs, S slabs of every parameter's gradient, S rows of 8 scalars, each block a multiple of 64 floats
    up = lambda n: (n + 63) & ~63
    d = desc(B=37)                                                         # 3 tiles, 3 slabs
    n_par = 8 * 8 + 8 + 8 * 8 + 8 + 204 * 8 + 204 + 51 * 8 + 51
    assert L.ocrl_c51_ws_floats(ctypes.byref(d)) == 2 * up(37 * 8) + up(3 * n_par) + up(3 * 8)


# ---- the projection
def test_the_hand_worked_batch():
    W = C.WORKED
    f = lambda v: torch.tensor(v, dtype=torch.float64)
    dones = torch.tensor(W["dones"], dtype=torch.uint8)
    disc = torch.full((3,), W["gamma"], dtype=torch.float64)
    args = (f(W["next_probs"]), f(W["rewards"]), dones, disc, W["v_min"], W["v_max"], W["Z"])
    assert C.support(0.0, 2.0, 5).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    assert C.project_gather(*args).tolist() == W["m"]                       # row 0: done, its NaN next_probs never read
    assert C.project_scatter(*args).tolist() == W["m"]
    # the two rows the loss is worked for: ce = -log p[a, 2] and -log p[a, 4]
    lg = torch.zeros(2, 2, 5, dtype=torch.float64)
    lg[0, 1] = f([0.0, 0.0, 1.0, 0.0, 0.0])
    next_probs = f([W["next_probs"][0]] * 2 + [W["next_probs"][1]] * 2).reshape(2, 2, 5)
    next_q = f([[float("inf"), 0.0], [1.0, 1.0]])
    loss, mq, mt, ce = C.c51_loss(lg, next_probs, next_q, torch.tensor([1, 7]), f(W["rewards"][:2]), dones[:2], W["gamma"], 0.0, 2.0)
    e = torch.tensor(1.0, dtype=torch.float64).exp()
    assert ce.tolist() == pytest.approx([-(e / (4 + e)).log().item(), math.log(5.0)], abs=1e-15)
    assert loss.item() == pytest.approx(ce.mean().item()) and mt.item() == pytest.approx((1.0 + 2.0) / 2)
    assert mq.item() == pytest.approx((((0 + 0.5 + 1.5 + 2) + e * 1.0) / (4 + e)).item() / 2 + 0.5)            # row 1: action 7 clamps to 1, uniform: q = 1


@pytest.mark.parametrize("Z", [2, 5, 51, 64])
def test_gather_form_equals_scatter_form(Z):
    B, v_min, v_max = 64, -0.5, 2.0
    gen = torch.Generator().manual_seed(300 + Z)
    z = C.support(v_min, v_max, Z)
    next_p = torch.softmax(torch.randn(B, Z, generator=gen, dtype=torch.float64) * 2, dim=-1)
    rewards = torch.randn(B, generator=gen, dtype=torch.float64) * 1.2
    disc = torch.rand(B, generator=gen, dtype=torch.float64)
    dones = (torch.arange(B) % 3 == 1).to(torch.uint8)
    rewards[0], rewards[1], dones[0], dones[1] = z[Z // 2], z[Z - 1], 1, 1                      # on an atom (done rows)
    rewards[2], disc[2], dones[2] = z[1] - z[0], 1.0, 0                                          # every target on an atom: a shift by one
    rewards[3], rewards[4], dones[4] = v_min - 3.0, v_max + 3.0, 1                                # below v_min, above v_max
    rewards[5], dones[5] = v_min - 3.0, 1
    g, s = C.project_gather(next_p, rewards, dones, disc, v_min, v_max, Z), C.project_scatter(next_p, rewards, dones, disc, v_min, v_max, Z)
    assert (g - s).abs().max().item() <= 1e-12 and (g.sum(-1) - 1).abs().max().item() <= 1e-12 and (g >= 0).all()
    assert g[0].argmax().item() == Z // 2 and g[0].max().item() == pytest.approx(1.0, abs=1e-12) and g[4, -1].item() == 1.0 and g[5, 0].item() == 1.0
    shifted = torch.cat([torch.zeros(1, dtype=torch.float64), next_p[2, :-2], next_p[2, -2:].sum().reshape(1)])       # the top atom takes two
    assert (g[2] - shifted).abs().max().item() <= 1e-12
    # where nothing is clamped the projection keeps the mean: sum m z = r + g sum p z (0 for the bootstrap of a done row)
    boot = torch.where(dones.bool(), torch.zeros(1, dtype=torch.float64), disc * (next_p * z).sum(-1))
    lo = rewards + torch.where(dones.bool(), torch.zeros(1, dtype=torch.float64), disc * v_min)
    hi = rewards + torch.where(dones.bool(), torch.zeros(1, dtype=torch.float64), disc * v_max)
    free = (torch.minimum(lo, hi) >= v_min) & (torch.maximum(lo, hi) <= v_max)
    assert free.sum() >= 4 and (~free).sum() >= 4
    assert ((g * z).sum(-1) - (rewards + boot))[free].abs().max().item() <= 1e-12


def test_the_dueling_rule_and_its_backward():
    gen = torch.Generator().manual_seed(9)
    adv = torch.randn(3, 4, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    v = torch.randn(3, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    lg = C.dueling_rule(adv, v)
    assert torch.allclose(lg.mean(dim=1), v) and lg.shape == (3, 4, 5)
    dl = torch.randn(3, 4, 5, generator=gen, dtype=torch.float64)
    da, dv = torch.autograd.grad(lg, [adv, v], dl)
    assert torch.allclose(dv, dl.sum(dim=1)) and torch.allclose(da, dl - dl.sum(dim=1, keepdim=True) / 4)        # the header's backward


# ---- config and the algorithm's arguments
def test_dqn_c51_config_composes_and_its_kwargs_are_dqns():
    from ocrl_amd import sb3s
    per, c51 = compose(os.path.join(CFG, "sb3"), "dqn_per").to_dict(), compose(os.path.join(CFG, "sb3"), "dqn_c51").to_dict()
    assert c51["name"] == "DQN"
    assert c51["algo_kwargs"] == dict(per["algo_kwargs"], n_atoms=51, v_min=0.0, v_max=2.0, dueling=True)
    params = inspect.signature(sb3s.DQN.__init__).parameters
    assert set(c51["algo_kwargs"]) <= set(params) and {k: params[k].default for k in NEW_KWARGS} == NEW_KWARGS
    assert set(NEW_KWARGS) <= set(sb3s.DQN.HYPER)
    pp = inspect.signature(sb3s.DQNPolicy.__init__).parameters
    assert {k: pp[k].default for k in NEW_KWARGS} == NEW_KWARGS
    full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=dqn_c51", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
    assert full.sb3.to_dict() == c51
    comment = open(os.path.join(CFG, "sb3", "dqn_c51.yaml")).read()
    assert "[0, 1]" in comment and "0.01 x max_steps = 1" in comment
    assert compose(os.path.join(CFG, "env"), "target-N4C4S3S1").max_steps == 100
    assert {"CategoricalQNetwork", "c51_loss"} <= set(sb3s.__all__)
    lp = inspect.signature(sb3s.c51_loss).parameters
    assert list(lp) == ["policy", "features", "next_probs", "next_q", "actions", "rewards", "dones", "gamma", "discounts", "weights"]
    import train_sb3
    assert set(train_sb3.ALGOS) == {"PPO", "A2C", "DQN"}


def _env(n=4):
    return types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=n))


@pytest.mark.parametrize("kw, n, name", [(dict(n_atoms=0), 4, "n_atoms"), (dict(n_atoms=-3), 4, "n_atoms"), (dict(n_atoms=65), 4, "n_atoms"),
                                         (dict(n_atoms=52), 5, r"n_actions \* n_atoms"), (dict(n_atoms=51, v_min=2.0, v_max=2.0), 4, "v_min < v_max"),
                                         (dict(n_atoms=51, v_min=1.0, v_max=0.0), 4, "v_min < v_max"), (dict(dueling=True), 4, "dueling")])
def test_bad_values_name_their_argument(kw, n, name):
    from ocrl_amd.sb3s import DQN, DQNPolicy
    with pytest.raises(ValueError, match=name):
        DQN(DQNPolicy, _env(n), **kw)


def test_the_head_follows_the_arguments():
    from ocrl_amd.sb3s import DQN, DQNPolicy, CategoricalQNetwork, QNetwork
    env = _env()
    plain = DQNPolicy(env.observation_space, env.action_space)
    assert type(plain.q_net) is QNetwork and (plain.n_atoms, plain.dueling) == (1, False)
    cat = DQNPolicy(env.observation_space, env.action_space, n_atoms=11, v_min=-1.0, v_max=1.0, dueling=True, net_arch=(8,))
    net = cat.q_net
    assert type(net) is CategoricalQNetwork and (net.n_actions, net.n_atoms, net.dueling, net.v_min, net.v_max) == (4, 11, True, -1.0, 1.0)
    assert list(cat.state_dict()) == ["q_net.q_net.0.weight", "q_net.q_net.0.bias", "q_net.q_net.2.weight", "q_net.q_net.2.bias",
                                      "q_net.value_net.weight", "q_net.value_net.bias"]
    assert [tuple(p.shape) for p in net._param_list()] == [(8, 4), (8,), (44, 8), (44,), (11, 8), (11,)]
    assert torch.allclose(net.atoms, torch.linspace(-1, 1, 11))
    with pytest.raises(ValueError, match="dueling"):
        DQNPolicy(env.observation_space, env.action_space, dueling=True)
    # a policy instance whose head disagrees with the arguments
    for kw in (dict(), dict(n_atoms=11, v_min=-1.0, v_max=1.0), dict(n_atoms=51, dueling=True), dict(n_atoms=11, dueling=True)):
        with pytest.raises(ValueError, match="n_atoms|v_min"):
            DQN(cat, env, device="cpu", **kw)
    with pytest.raises(ValueError, match="n_atoms"):
        DQN(plain, env, device="cpu", n_atoms=51)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.distribution(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.logits(torch.zeros(2, 4))
