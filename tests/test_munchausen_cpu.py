"""What DQN's Munchausen targets promise without a GPU: the header (include/ocrl_hip_munchausen.h) parses, binds and is exported; the
Makefile lists the new parts; every rejection the entry point makes before a launch; the hand-worked rows of tests/munchausen_ref.py; the
mdqn and miqn configs; the ValueErrors of DQN's new arguments; and checkpoints with and without the new keys."""
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
from tests import munchausen_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
NEW_KWARGS = dict(munchausen=False, munchausen_alpha=0.9, munchausen_tau=0.03, munchausen_clip=-1.0)
ON = dict(munchausen=True, munchausen_alpha=0.9, munchausen_tau=0.03, munchausen_clip=-1.0)
ALPHA, CLIP = 0.9, -1.0
f64 = torch.float64


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    path = os.path.join(ROOT, "include", "ocrl_hip_munchausen.h")
    text = open(path).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == {"ocrl_munchausen_targets": 16} and abi.consts == {} and abi.structs == {}
    assert set(_lib.ABI_MUNCHAUSEN.functions) == {"ocrl_munchausen_targets"} and os.path.samefile(_lib.MUNCHAUSEN_HEADER_PATH, path)
    L = _lib.lib()
    at = L.ocrl_munchausen_targets.argtypes
    assert len(at) == 16 and at[3] is ctypes.c_int and at[7] is ctypes.c_int and at[8] is ctypes.c_int
    assert at[9] is ctypes.c_float and at[10] is ctypes.c_float and at[11] is ctypes.c_float                      # alpha, tau, clip_lo
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_MUNCHAUSEN_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                      # self-contained
    assert _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    older = set()
    for abi_old in (_lib.ABI, _lib.ABI_DQN, _lib.ABI_ROLLOUT, _lib.ABI_REPLAY, _lib.ABI_C51, _lib.ABI_NOISY, _lib.ABI_CLASSIFIER, _lib.ABI_IODINE,
                    _lib.ABI_QR, _lib.ABI_IQN, _lib.ABI_SLATE_KERNELS, _lib.ABI_VIT_KERNELS):
        older |= set(abi_old.functions)
    assert "ocrl_munchausen_targets" not in older


def test_the_makefile_lists_the_new_parts():
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    srcs, objs, hdrs = (re.search(rf"^{k} = (.*)$", makefile, re.M).group(1).split() for k in ("SRCS", "OBJS", "HDRS"))
    assert "munchausen.hip" in srcs and "munchausen_unit.o" in objs and "munchausen.h" in hdrs and "../../include/ocrl_hip_munchausen.h" in hdrs
    line = re.search(r"^([^#\n]*): munchausen\.h", makefile, re.M).group(1).split()
    assert {"munchausen.o", "munchausen_unit.o"} <= set(line)
    for f in ("munchausen.hip", "munchausen.h", "munchausen_unit.cpp"):
        assert os.path.exists(os.path.join(ROOT, "ocrl_amd", "csrc", f)), f


# ---- rejections before the launch
def test_arguments_are_checked_before_the_launch():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)

    def call(B=5, A=4, Np=8, alpha=0.9, tau=0.03, clip=-1.0, quant=p, nm=p, cur=p, nxt=p, actions=p, rewards=p, dones=p, ro=p, nv=p):
        return L.ocrl_munchausen_targets(cur, nxt, quant, Np, actions, rewards, dones, B, A, alpha, tau, clip, ro, nv, nm, None)

    nan, inf = float("nan"), float("inf")
    for kw, msg in ((dict(B=0), "batch >= 1"), (dict(B=-3), "batch >= 1"), (dict(A=0), "1 <= n_actions <= 64"), (dict(A=65), "1 <= n_actions <= 64"),
                    (dict(Np=65), "n_target_samples"), (dict(Np=-1), "n_target_samples"), (dict(Np=0), "n_target_samples"),        # 0 with both given
                    (dict(Np=8, quant=None, nm=None), "n_target_samples"), (dict(Np=8, quant=None), "n_target_samples"),
                    (dict(Np=8, nm=None), "n_target_samples"), (dict(Np=0, quant=None), "n_target_samples"), (dict(Np=0, nm=None), "n_target_samples"),
                    (dict(alpha=-0.1), "alpha in [0, 1]"), (dict(alpha=1.5), "alpha in [0, 1]"), (dict(alpha=nan), "alpha in [0, 1]"),
                    (dict(tau=0.0), "tau finite and > 0"), (dict(tau=-1.0), "tau finite and > 0"), (dict(tau=inf), "tau finite and > 0"),
                    (dict(tau=nan), "tau finite and > 0"), (dict(clip=0.5), "clip_lo finite and <= 0"), (dict(clip=-inf), "clip_lo finite and <= 0"),
                    (dict(clip=nan), "clip_lo finite and <= 0"), (dict(cur=None), "null argument"), (dict(nxt=None), "null argument"),
                    (dict(actions=None), "null argument"), (dict(rewards=None), "null argument"), (dict(dones=None), "null argument"),
                    (dict(ro=None), "null argument"), (dict(nv=None), "null argument")):
        assert call(**kw) != 0 and "ocrl_munchausen_targets: " in last_error() and msg in last_error(), (kw, msg, last_error())


# ---- the restatement against rows worked on paper (tests/munchausen_ref.py's docstring)
@pytest.mark.parametrize("dtype", [torch.float32, f64])
@pytest.mark.parametrize("tau", [0.03, 1.0])
def test_one_action_changes_nothing(dtype, tau):
    gen = torch.Generator().manual_seed(1)
    cur, nxt, quant = (torch.randn(*s, generator=gen).to(dtype) * 2 for s in ((6, 1), (6, 1), (6, 1, 5)))
    r, d = torch.randn(6, generator=gen).to(dtype), torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.uint8)
    ro, nv, nm = M.targets(cur, nxt, torch.tensor([0, 0, 3, -2, 0, 0]), r, d, ALPHA, tau, CLIP, quant)
    keep = ~d.bool()
    assert torch.equal(ro, r) and torch.equal(nv[keep], nxt[keep]) and torch.equal(nm[keep], quant[keep])
    assert (nv[~keep] == 0).all() and (nm[~keep] == 0).all() and ro.dtype == nv.dtype == nm.dtype == dtype


@pytest.mark.parametrize("tau", [0.03, 1.0])
def test_an_all_equal_row_is_the_uniform_policy(tau):
    A = 4
    cur, nxt = torch.full((1, A), 1.5, dtype=f64), torch.full((1, A), -0.75, dtype=f64)
    quant = torch.arange(A * 3, dtype=f64).reshape(1, A, 3)
    logpi, pi, c = M.policy(cur, tau)
    assert torch.allclose(pi, torch.full((1, A), 0.25, dtype=f64), atol=1e-15) and torch.allclose(c, torch.full((1, A), -tau * math.log(A), dtype=f64), atol=1e-15)
    ro, nv, nm = M.targets(cur, nxt, torch.tensor([2]), torch.tensor([0.5], dtype=f64), torch.zeros(1, dtype=torch.uint8), ALPHA, tau, CLIP, quant)
    bonus = ALPHA * max(CLIP, -tau * math.log(A))
    assert abs(ro.item() - (0.5 + bonus)) < 1e-15
    assert torch.allclose(nv, torch.full((1, A), -0.75 + tau * math.log(A), dtype=f64), atol=1e-14)
    assert torch.allclose(nm, (quant.mean(1, keepdim=True) + tau * math.log(A)).expand(1, A, 3), atol=1e-13)


@pytest.mark.parametrize("dtype", [torch.float32, f64])
@pytest.mark.parametrize("tau", [0.03, 1.0])
def test_an_action_far_below_the_maximum_takes_the_whole_clip(dtype, tau):
    cur = torch.tensor([[0.25, 0.25 - 1001 * tau, 0.0]], dtype=dtype)
    nxt = torch.tensor([[1.0, 1.0 - 2000 * tau, 0.5]], dtype=dtype)                       # exp underflows: pi = 0, logpi finite, the term 0
    quant = torch.tensor([[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]], dtype=dtype)
    ro, nv, nm = M.targets(cur, nxt, torch.tensor([1]), torch.tensor([2.0], dtype=dtype), torch.zeros(1, dtype=torch.uint8), ALPHA, tau, CLIP, quant)
    assert ro.item() == torch.tensor(2.0, dtype=dtype).add(torch.tensor(ALPHA * CLIP, dtype=dtype)).item()
    logpi, pi, _ = M.policy(nxt, tau)
    assert pi[0, 1].item() == 0.0 and math.isfinite(logpi[0, 1].item()) and torch.isfinite(nv).all() and torch.isfinite(nm).all()
    assert (nv == nv[:, :1]).all() and (nm == nm[:, :1]).all()                            # broadcast over the actions
    # with alpha = 0 the reward comes back as it is
    assert torch.equal(M.targets(cur, nxt, torch.tensor([1]), torch.tensor([2.0], dtype=dtype), torch.zeros(1, dtype=torch.uint8), 0.0, tau, CLIP)[0],
                       torch.tensor([2.0], dtype=dtype))


def test_a_finished_row_never_reads_its_next_inputs():
    cur = torch.tensor([[0.0, 0.5], [0.5, 0.25]], dtype=f64)
    nxt = torch.tensor([[float("inf"), float("nan")], [0.1, 0.2]], dtype=f64)
    quant = torch.full((2, 2, 3), float("nan"), dtype=f64)
    quant[1] = 1.0
    ro, nv, nm = M.targets(cur, nxt, torch.tensor([0, 1]), torch.tensor([1.0, -1.0], dtype=f64), torch.tensor([1, 0], dtype=torch.uint8), ALPHA, 1.0, CLIP,
                           quant)
    assert torch.isfinite(ro).all() and torch.isfinite(nv).all() and torch.isfinite(nm).all()
    assert (nv[0] == 0).all() and (nm[0] == 0).all() and (nv[1] != 0).all()
    assert abs(ro[0].item() - (1.0 + ALPHA * (-0.5 - math.log(1 + math.exp(-0.5))))) < 1e-15        # the bonus of a finished row is still added
    none = M.targets(cur, nxt, torch.tensor([0, 1]), torch.tensor([1.0, -1.0], dtype=f64), torch.tensor([1, 0], dtype=torch.uint8), ALPHA, 1.0, CLIP)
    assert none[2] is None and torch.equal(none[0], ro) and torch.equal(none[1], nv)


def test_the_soft_value_is_tau_logsumexp():
    """sum_a pi_a (q_a - tau log pi_a) = tau log sum_a exp(q_a / tau): the identity the broadcast rests on"""
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(9, 5, generator=gen, dtype=f64) * 2
    for tau in (0.03, 1.0):
        _, nv, _ = M.targets(q, q, torch.zeros(9, dtype=torch.int64), torch.zeros(9, dtype=f64), torch.zeros(9, dtype=torch.uint8), ALPHA, tau, CLIP)
        assert torch.allclose(nv[:, 0], tau * torch.logsumexp(q / tau, dim=1), atol=1e-13)


# ---- configs and the algorithm's arguments
def test_the_configs_compose_and_their_kwargs_are_dqns():
    from ocrl_amd import sb3s
    sb3 = lambda name: compose(os.path.join(CFG, "sb3"), name).to_dict()
    dqn, iqn, mdqn, miqn = sb3("dqn"), sb3("iqn"), sb3("mdqn"), sb3("miqn")
    assert mdqn["name"] == miqn["name"] == "DQN"
    assert mdqn["algo_kwargs"] == dict(dqn["algo_kwargs"], **ON)
    assert miqn["algo_kwargs"] == dict(iqn["algo_kwargs"], double_q=False, **ON)
    params = inspect.signature(sb3s.DQN.__init__).parameters
    for cfg in (mdqn, miqn):
        assert set(cfg["algo_kwargs"]) <= set(params)
    assert {k: params[k].default for k in NEW_KWARGS} == NEW_KWARGS and set(NEW_KWARGS) <= set(sb3s.DQN.HYPER)
    for name in ("mdqn", "miqn"):
        text = open(os.path.join(CFG, "sb3", name + ".yaml")).read()
        assert text.startswith("# ") and "include/ocrl_hip_munchausen.h" in text
        full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={name}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
        assert full.sb3.to_dict() == sb3(name)
    assert "munchausen_targets" in sb3s.__all__
    mp = inspect.signature(sb3s.munchausen_targets).parameters
    assert list(mp) == ["cur_q", "next_q", "actions", "rewards", "dones", "alpha", "tau", "clip_lo", "next_quantiles"] and mp["next_quantiles"].default is None
    import train_sb3
    assert set(train_sb3.ALGOS) == {"PPO", "A2C", "DQN"} and "sb3=mdqn" in train_sb3.__doc__ and "sb3=miqn" in train_sb3.__doc__


def _env(n=4):
    return types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=n))


@pytest.mark.parametrize("kw, name", [(dict(munchausen=True, n_atoms=51), "munchausen.*n_atoms"), (dict(munchausen=True, double_q=True), "munchausen.*double_q"),
                                      (dict(munchausen=True, n_tau_samples=8, double_q=True), "munchausen.*double_q"),
                                      (dict(munchausen=True, munchausen_alpha=-0.1), "munchausen_alpha"), (dict(munchausen=True, munchausen_alpha=1.5), "munchausen_alpha"),
                                      (dict(munchausen=True, munchausen_tau=0.0), "munchausen_tau"), (dict(munchausen=True, munchausen_tau=float("inf")), "munchausen_tau"),
                                      (dict(munchausen=True, munchausen_tau=float("nan")), "munchausen_tau"),
                                      (dict(munchausen=True, munchausen_clip=0.5), "munchausen_clip"), (dict(munchausen=True, munchausen_clip=float("-inf")), "munchausen_clip"),
                                      (dict(munchausen_tau=-1.0), "munchausen_tau")])
def test_refusals_name_their_arguments(kw, name):
    from ocrl_amd.sb3s import DQN, DQNPolicy
    with pytest.raises(ValueError, match=name):
        DQN(DQNPolicy, _env(), device="cpu", **kw)


def test_the_three_heads_build_on_the_cpu_and_the_function_refuses_cpu_tensors():
    from ocrl_amd import sb3s
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env = _env()
    for head, cls in ((dict(), sb3s.QNetwork), (dict(n_quantiles=8, dueling=True), sb3s.QuantileQNetwork), (dict(n_tau_samples=8, n_cos=16), sb3s.ImplicitQuantileQNetwork)):
        model = DQN(DQNPolicy, env, device="cpu", munchausen=True, munchausen_alpha=0.5, munchausen_tau=0.1, munchausen_clip=-2.0, n_step=3,
                    prioritized_replay=True, noisy=True, policy_kwargs=dict(net_arch=(8,)), **head)
        assert type(model.policy.q_net) is cls and type(model.target.q_net) is cls
        assert (model.munchausen, model.munchausen_alpha, model.munchausen_tau, model.munchausen_clip) == (True, 0.5, 0.1, -2.0)
    assert DQN(DQNPolicy, env, device="cpu").munchausen is False
    z = torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        sb3s.munchausen_targets(z, z, torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(2, dtype=torch.uint8), 0.9, 0.03, -1.0)


def test_checkpoints_carry_the_four_values(tmp_path):
    """save writes them; a mismatch is refused by the key's name; what an earlier version wrote has none of them and loads as
    munchausen=False"""
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env, arch = _env(), dict(policy_kwargs=dict(net_arch=(8,)))
    model = DQN(DQNPolicy, env, device="cpu", munchausen=True, **arch)
    path = str(tmp_path / "m.pt")
    model.save(path)
    ck = torch.load(path, weights_only=True)
    assert {k: ck["hyper"][k] for k in ON} == ON
    twin = DQN(DQNPolicy, env, device="cpu", seed=4, munchausen=True, **arch)
    assert twin.load(path) is twin and torch.equal(twin.flat_p, model.flat_p) and twin.munchausen is True
    for kw, key in ((dict(), "munchausen"), (dict(munchausen=True, munchausen_alpha=0.5), "munchausen_alpha"), (dict(munchausen=True, munchausen_tau=0.1), "munchausen_tau"),
                    (dict(munchausen=True, munchausen_clip=-2.0), "munchausen_clip")):
        other = DQN(DQNPolicy, env, device="cpu", seed=3, **arch, **kw)
        keep = other.flat_p.clone()
        with pytest.raises(ValueError, match=f"the checkpoint was written with {key} = "):
            other.load(path)
        assert torch.equal(other.flat_p, keep)
    for k in ON:
        del ck["hyper"][k]
    old = str(tmp_path / "old.pt")
    torch.save(ck, old)
    plain = DQN(DQNPolicy, env, device="cpu", seed=3, **arch)
    assert plain.load(old) is plain and {k: getattr(plain, k) for k in NEW_KWARGS} == NEW_KWARGS and torch.equal(plain.flat_p, model.flat_p)
    with pytest.raises(ValueError, match="the checkpoint was written with munchausen = False, this instance has munchausen = True"):
        DQN(DQNPolicy, env, device="cpu", munchausen=True, **arch).load(old)
