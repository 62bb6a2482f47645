"""What DQN's implicit quantile head promises without a GPU: the header (include/ocrl_hip_iqn.h) parses, binds and is exported; the
Makefile lists the new parts; every rejection its entry points make before a launch; the hand-worked values of tests/iqn_ref.py and its
agreement with tests/qr_ref.py at the midpoint fractions; the iqn config; and the ValueErrors of DQN's new arguments."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import iqn_ref as I
from tests import qr_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
FUNCTIONS = {"ocrl_iqn_desc_size": 0, "ocrl_iqn_ws_floats": 1, "ocrl_iqn_taus": 6, "ocrl_iqn_fwd": 10, "ocrl_iqn_bwd": 10, "ocrl_iqn_act": 11,
             "ocrl_iqn_td_fwd_bwd": 21}
NEW_KWARGS = dict(n_tau_samples=0, n_tau_prime_samples=0, n_act_samples=32, n_cos=64)
f64 = torch.float64


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_iqn.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {} and set(abi.structs) == {"ocrl_iqn_desc"}
    assert [f[0] for f in abi.structs["ocrl_iqn_desc"]._fields_] == ["B", "F", "A", "N", "C", "n", "dims", "acts"]
    assert all(t in (ctypes.c_int, ctypes.c_int * 8) for _, t in abi.structs["ocrl_iqn_desc"]._fields_)         # int fields only
    assert set(_lib.ABI_IQN.functions) == set(FUNCTIONS) and os.path.samefile(_lib.IQN_HEADER_PATH, os.path.join(ROOT, "include", "ocrl_hip_iqn.h"))
    L = _lib.lib()
    for name, n in FUNCTIONS.items():
        assert len(getattr(L, name).argtypes) == n, name
    td = L.ocrl_iqn_td_fwd_bwd.argtypes
    assert L.ocrl_iqn_ws_floats.restype is ctypes.c_size_t and td[5] is ctypes.c_int and td[12] is ctypes.c_float and td[13] is ctypes.c_float
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_IQN_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                      # self-contained
    assert _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    older = set()
    for abi_old in (_lib.ABI, _lib.ABI_DQN, _lib.ABI_ROLLOUT, _lib.ABI_REPLAY, _lib.ABI_C51, _lib.ABI_NOISY, _lib.ABI_CLASSIFIER, _lib.ABI_IODINE,
                    _lib.ABI_QR, _lib.ABI_SLATE_KERNELS, _lib.ABI_VIT_KERNELS):
        older |= set(abi_old.functions)
    assert not set(FUNCTIONS) & older


def test_the_makefile_lists_the_new_parts():
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    srcs, objs, hdrs = (re.search(rf"^{k} = (.*)$", makefile, re.M).group(1).split() for k in ("SRCS", "OBJS", "HDRS"))
    assert "iqn.hip" in srcs and "iqn_unit.o" in objs and "iqn.h" in hdrs and "../../include/ocrl_hip_iqn.h" in hdrs
    assert "qhead_tile.h" in hdrs
    for dep, objects in (("acnet.h", ("iqn.o", "iqn_unit.o")), ("acnet_tile.h", ("iqn.o",)), ("acnet_host.h", ("iqn_unit.o",)),
                         ("qhead_tile.h", ("iqn.o",))):
        line = re.search(rf"^([^#\n]*): {re.escape(dep)}$", makefile, re.M).group(1).split()
        assert set(objects) <= set(line), (dep, line)
    for f in ("iqn.hip", "iqn.h", "iqn_unit.cpp"):
        assert os.path.exists(os.path.join(ROOT, "ocrl_amd", "csrc", f)), f


def test_descriptor_size_is_the_ctypes_struct():
    assert _lib.lib().ocrl_iqn_desc_size() == ctypes.sizeof(_lib.IqnDesc) == 22 * 4 == 88
    d = _lib.iqn_desc(5, 8, 4, 16, 64, [64, 32], [1, 2])
    assert (d.B, d.F, d.A, d.N, d.C, d.n, list(d.dims)[:3], list(d.acts)[:3]) == (5, 8, 4, 16, 64, 2, [64, 32, 0], [1, 2, 0])
    with pytest.raises(ValueError, match="at most 8 hidden layers"):
        _lib.iqn_desc(5, 8, 4, 16, 64, [4] * 9, [1] * 9)


# ---- rejections before any launch
def test_arguments_are_checked_before_any_launch():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)
    desc = lambda A=4, N=8, C=16, dims=(8, 8), B=5, F=8: _lib.iqn_desc(B, F, A, N, C, list(dims), [1] * len(dims))
    good = desc()
    w = (ctypes.c_void_p * 8)(*[FAKE] * 8)                                     # 2 (n + 2) pointers
    hole = (ctypes.c_void_p * 8)(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE)
    big = 1 << 40

    def fwd(d=good, ww=w, outs=(p, p), save=0, ws=None, n=0, taus=p):
        return L.ocrl_iqn_fwd(ctypes.byref(d) if d is not None else None, p, taus, ww, *outs, save, ws, n, None)

    def bwd(d=good, ww=w, dw=w, dq=p, n=big, taus=p):
        return L.ocrl_iqn_bwd(ctypes.byref(d), p, taus, ww, dq, None, dw, p, n, None)

    def act(d=good, ww=w, actions=p):
        return L.ocrl_iqn_act(ctypes.byref(d), p, ww, 0, 0, 0.1, None, None, actions, None, None)

    def td(d=good, ww=w, dw=w, kappa=1.0, nq=p, n=big, Np=8, taus=p):
        return L.ocrl_iqn_td_fwd_bwd(ctypes.byref(d), p, taus, ww, nq, Np, p, p, p, p, None, None, 0.99, kappa, p, None, None, dw, p, n, None)

    limits = ((desc(B=0), "batch >= 1"), (desc(F=0), "feature_dim is a multiple of 4 in 4 .. 256"), (desc(F=6), "feature_dim is a multiple of 4 in 4 .. 256"),
              (desc(F=260), "feature_dim is a multiple of 4 in 4 .. 256"), (desc(A=0), "1 <= n_actions <= 64"), (desc(A=65), "1 <= n_actions <= 64"),
              (desc(N=0), "1 <= n_samples <= 64"), (desc(N=65), "1 <= n_samples <= 64"), (desc(C=0), "n_cos is a multiple of 4 in 4 .. 64"),
              (desc(C=6), "n_cos is a multiple of 4 in 4 .. 64"), (desc(C=68), "n_cos is a multiple of 4 in 4 .. 64"),
              (desc(dims=(6,)), "multiples of 4"), (desc(dims=(260,)), "multiples of 4"), (desc(B=1 << 20, N=8), "expanded rows"))
    for bad, msg in limits:
        for call in (fwd, bwd, act, td):
            assert call(d=bad) != 0 and msg in last_error(), (msg, last_error())
        assert L.ocrl_iqn_ws_floats(ctypes.byref(bad)) == 0 and msg in last_error()
    nine = desc()
    nine.n = 9
    for call, msg in ((lambda: fwd(d=None), "ocrl_iqn_fwd: null descriptor"),
                      (lambda: fwd(d=nine), "at most 8 hidden layers"),
                      (lambda: td(Np=0), "ocrl_iqn_td_fwd_bwd: 1 <= n_target_samples <= 64"),
                      (lambda: td(Np=65), "1 <= n_target_samples <= 64"),
                      (lambda: td(kappa=0.0), "ocrl_iqn_td_fwd_bwd: kappa finite and > 0"),
                      (lambda: td(kappa=float("inf")), "kappa finite and > 0"),
                      (lambda: td(kappa=-1.0), "kappa finite and > 0"),
                      (lambda: td(kappa=float("nan")), "kappa finite and > 0"),
                      (lambda: fwd(outs=(None, None)), "quantiles and q are both null"),
                      (lambda: fwd(ww=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: fwd(ww=None), "ocrl_iqn_fwd: null argument"),
                      (lambda: fwd(taus=None), "ocrl_iqn_fwd: null argument"),
                      (lambda: fwd(save=1, ws=p, n=8), "workspace too small"),
                      (lambda: fwd(save=1, ws=None, n=big), "workspace too small"),
                      (lambda: fwd(outs=(None, p), ws=None, n=0), "workspace too small"),          # q alone: theta goes to the workspace
                      (lambda: bwd(dw=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: bwd(dq=None), "ocrl_iqn_bwd: null argument"),
                      (lambda: bwd(taus=None), "ocrl_iqn_bwd: null argument"),
                      (lambda: bwd(n=8), "workspace too small"),
                      (lambda: act(ww=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: act(actions=None), "ocrl_iqn_act: null argument"),
                      (lambda: td(nq=None), "ocrl_iqn_td_fwd_bwd: null argument"),
                      (lambda: td(taus=None), "ocrl_iqn_td_fwd_bwd: null argument"),
                      (lambda: td(dw=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: td(n=8), "workspace too small"),
                      (lambda: L.ocrl_iqn_taus(0, 0, 0, 8, p, None), "ocrl_iqn_taus: batch >= 1"),
                      (lambda: L.ocrl_iqn_taus(0, 0, 4, 0, p, None), "ocrl_iqn_taus: 1 <= n_samples <= 64"),
                      (lambda: L.ocrl_iqn_taus(0, 0, 4, 65, p, None), "1 <= n_samples <= 64"),
                      (lambda: L.ocrl_iqn_taus(0, 0, 4, 8, None, None), "ocrl_iqn_taus: null argument")):
        assert call() != 0 and msg in last_error(), (msg, last_error())
    # an empty chain has four pointers: the hole at 3 is the output Linear's bias
    none = desc(dims=())
    four = (ctypes.c_void_p * 4)(FAKE, FAKE, FAKE, None)
    assert fwd(d=none, ww=four) != 0 and "parameter pointer 3 of 4 is null" in last_error()
    # the workspace: E = B * N expanded rows.  phi and the chain's saved layer outputs, S slabs of every parameter's gradient, S rows of 8
    # scalars, then theta [E, A], the partial losses [E], theta of the action taken [E] and dz * phi [E, F]; each block a multiple of 64
    up = lambda n: (n + 63) & ~63
    d = desc()                                                              # E = 40: 3 tiles, 3 slabs
    n_par = 8 * 16 + 8 + 8 * 8 + 8 + 8 * 8 + 8 + 4 * 8 + 4
    assert L.ocrl_iqn_ws_floats(ctypes.byref(d)) == 3 * up(40 * 8) + up(3 * n_par) + up(3 * 8) + up(40 * 4) + 2 * up(40) + up(40 * 8)
    d = desc(B=130, N=8, dims=())                                           # E = 1040: 65 tiles, 64 slabs
    n_par = 8 * 16 + 8 + 4 * 8 + 4
    assert L.ocrl_iqn_ws_floats(ctypes.byref(d)) == up(1040 * 8) + up(64 * n_par) + up(64 * 8) + up(1040 * 4) + 2 * up(1040) + up(1040 * 8)
    for lim in (desc(N=1, A=1, C=4, F=4), desc(N=64, A=64, C=64, F=256, dims=(256,) * 8)):                                  # the limits themselves
        assert L.ocrl_iqn_ws_floats(ctypes.byref(lim)) > 0


# ---- the restatement against values worked on paper (tests/iqn_ref.py's docstring)
def test_cosines_worked_on_paper():
    c = I.cos_features(torch.tensor([0.5, 0.0, 1.0 / 3.0]), 8)
    assert torch.allclose(c[0], torch.tensor([1.0, 0.0, -1.0, 0.0, 1.0, 0.0, -1.0, 0.0], dtype=f64), atol=1e-15)
    assert c[1].tolist() == [1.0] * 8
    assert abs(c[2, 1].item() - 0.5) < 1e-7 and c.dtype == f64              # 1 / 3 is the fp32 1 / 3: 0.5 to its rounding
    # the product is formed in fp32: k * tau of the largest k and fraction is the fp32 rounding of the exact product
    tau = torch.tensor([1.0 - 2.0 ** -24])
    prod = (tau * torch.arange(64, dtype=torch.float32))[63].double()
    assert I.cos_features(tau, 64)[0, 63].item() == torch.cos(torch.pi * prod).item() and prod.item() != 63 * (1.0 - 2.0 ** -24)


def test_one_fraction_worked_on_paper():
    """B = A = N = N' = 1, tau = 0.25, theta = 0.25, kappa 1, gamma 1, reward 0: T = 0.75 -> 0.25 * 0.125 = 0.03125; T = -2.75 -> 0.75 * 2.5
    = 1.875; the gradients -(0.25 * 0.5) and -(0.75 * -1)"""
    for T, want, grad in ((0.75, 0.03125, -0.125), (-2.75, 1.875, 0.75)):
        theta = torch.tensor([[[0.25]]], dtype=f64, requires_grad=True)
        loss, mq, mt, ql = I.iqn_loss(theta, torch.tensor([[0.25]]), torch.tensor([[[T]]], dtype=f64), torch.zeros(1, 1, dtype=f64), torch.tensor([0]),
                                      torch.zeros(1, dtype=f64), torch.tensor([0], dtype=torch.uint8), 1.0)
        assert ql.tolist() == [want] and loss.item() == want and mq.item() == 0.25 and mt.item() == T
        assert torch.autograd.grad(loss, theta)[0].item() == grad


def test_at_the_midpoints_the_loss_is_the_quantile_heads():
    """taus = (i + 0.5) / N and N' = N: loss, gradient and row_loss equal qr_ref.qr_loss's exactly in fp64"""
    B, A, N = 7, 3, 5
    gen = torch.Generator().manual_seed(3)
    theta = torch.randn(B, A, N, generator=gen, dtype=f64)
    nxt, nq = torch.randn(B, A, N, generator=gen, dtype=f64) * 2, torch.randn(B, A, generator=gen, dtype=f64)
    a, r = torch.randint(-1, A + 1, (B,), generator=gen), torch.randn(B, generator=gen, dtype=f64) * 2
    d = (torch.arange(B) % 3 == 1).to(torch.uint8)
    nxt[d.bool()], nq[d.bool()] = float("nan"), float("inf")
    disc, w = torch.rand(B, generator=gen, dtype=f64), torch.rand(B, generator=gen, dtype=f64) + 0.1
    taus = Q.taus(N).unsqueeze(0).expand(B, -1)
    for kw in (dict(), dict(discounts=disc, weights=w), dict(kappa=0.3)):
        t1, t2 = theta.clone().requires_grad_(True), theta.clone().requires_grad_(True)
        mine, theirs = I.iqn_loss(t1, taus, nxt, nq, a, r, d, 0.9, **kw), Q.qr_loss(t2, nxt, nq, a, r, d, 0.9, **kw)
        assert all(torch.equal(x, y) for x, y in zip(mine, theirs))
        assert torch.equal(torch.autograd.grad(mine[0], t1)[0], torch.autograd.grad(theirs[0], t2)[0])


def test_the_head_of_the_restatement():
    ps = I.make_params(8, 3, 16, (12,), 4, f64)
    assert [tuple(p.shape) for p in ps] == [(8, 16), (8,), (12, 8), (12,), (3, 12), (3,)]
    gen = torch.Generator().manual_seed(1)
    x, taus = torch.randn(4, 8, generator=gen, dtype=f64), torch.randint(0, 2 ** 24, (4, 5), generator=gen).float() / 2 ** 24
    theta, q = I.quantiles(x, taus, ps, (1,), 3, 16)
    assert theta.shape == (4, 3, 5) and torch.allclose(q, theta.mean(-1))
    b, s = 2, 3                                                             # one expanded row by hand
    c = torch.cos(torch.pi * (taus[b, s] * torch.arange(16, dtype=torch.float32)).double())
    z = x[b] * torch.relu(ps[0] @ c + ps[1])
    assert torch.allclose(theta[b, :, s], ps[4] @ torch.relu(ps[2] @ z + ps[3]) + ps[5])
    # N' differs from N: the targets have N' columns and the loss averages over them
    nxt = torch.arange(24, dtype=f64).reshape(1, 3, 8)
    out = I.iqn_loss(theta[:1], taus[:1], nxt, torch.tensor([[1.0, 2.0, 2.0]], dtype=f64), torch.tensor([0]), torch.tensor([1.0], dtype=f64),
                     torch.tensor([0], dtype=torch.uint8), 0.5)
    assert out[2].item() == 1.0 + 0.5 * 11.5                                # action 1's values 8 .. 15: a tie of next_q takes the lower action


# ---- config and the algorithm's arguments
def test_iqn_config_composes_and_its_kwargs_are_dqns():
    from ocrl_amd import sb3s
    rainbow, iqn = compose(os.path.join(CFG, "sb3"), "rainbow").to_dict(), compose(os.path.join(CFG, "sb3"), "iqn").to_dict()
    assert iqn["name"] == "DQN"
    want = {k: v for k, v in rainbow["algo_kwargs"].items() if k not in ("v_min", "v_max")}
    assert iqn["algo_kwargs"] == dict(want, dueling=False, n_atoms=1, n_tau_samples=8, n_tau_prime_samples=8, n_act_samples=32, n_cos=64, huber_kappa=1.0)
    params = inspect.signature(sb3s.DQN.__init__).parameters
    assert set(iqn["algo_kwargs"]) <= set(params) and {k: params[k].default for k in NEW_KWARGS} == NEW_KWARGS
    assert set(NEW_KWARGS) <= set(sb3s.DQN.HYPER)
    pp = inspect.signature(sb3s.DQNPolicy.__init__).parameters
    assert (pp["n_tau_samples"].default, pp["n_act_samples"].default, pp["n_cos"].default) == (0, 32, 64)
    full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=iqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
    assert full.sb3.to_dict() == iqn
    assert {"ImplicitQuantileQNetwork", "iqn_loss"} <= set(sb3s.__all__)
    lp = inspect.signature(sb3s.iqn_loss).parameters
    assert list(lp) == ["policy", "features", "taus", "next_quantiles", "next_q", "actions", "rewards", "dones", "gamma", "kappa", "discounts", "weights"]
    assert lp["kappa"].default == 1.0
    import train_sb3
    assert set(train_sb3.ALGOS) == {"PPO", "A2C", "DQN"}


def _env(n=4):
    return types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=n))


@pytest.mark.parametrize("kw, name", [(dict(n_tau_samples=-1), "n_tau_samples"), (dict(n_tau_samples=65), "n_tau_samples"),
                                      (dict(n_tau_samples=8, n_tau_prime_samples=-1), "n_tau_prime_samples"),
                                      (dict(n_tau_samples=8, n_tau_prime_samples=65), "n_tau_prime_samples"),
                                      (dict(n_tau_samples=8, n_act_samples=0), "n_act_samples"), (dict(n_tau_samples=8, n_act_samples=65), "n_act_samples"),
                                      (dict(n_tau_samples=8, n_cos=0), "n_cos"), (dict(n_tau_samples=8, n_cos=6), "n_cos"),
                                      (dict(n_tau_samples=8, n_cos=68), "n_cos"), (dict(n_tau_samples=8, huber_kappa=0.0), "huber_kappa"),
                                      (dict(n_tau_samples=8, n_atoms=51), "n_tau_samples > 0 with n_atoms > 1 or n_quantiles > 0"),
                                      (dict(n_tau_samples=8, n_quantiles=8), "n_tau_samples > 0 with n_atoms > 1 or n_quantiles > 0"),
                                      (dict(n_tau_samples=8, dueling=True), "dueling.*n_tau_samples")])
def test_bad_values_name_their_argument(kw, name):
    from ocrl_amd.sb3s import DQN, DQNPolicy
    with pytest.raises(ValueError, match=name):
        DQN(DQNPolicy, _env(), device="cpu", **kw)


def test_the_head_follows_the_arguments():
    from ocrl_amd.sb3s import DQN, DQNPolicy, ImplicitQuantileQNetwork, NoisyLinear, QNetwork
    env = _env()
    plain = DQNPolicy(env.observation_space, env.action_space)
    assert type(plain.q_net) is QNetwork and plain.n_tau_samples == 0
    pol = DQNPolicy(env.observation_space, env.action_space, n_tau_samples=8, n_act_samples=4, n_cos=16, net_arch=(8,))
    net = pol.q_net
    assert type(net) is ImplicitQuantileQNetwork and (net.n_actions, net.n_cos, net.n_act_samples) == (4, 16, 4)
    assert list(pol.state_dict()) == ["q_net.q_net.0.weight", "q_net.q_net.0.bias", "q_net.q_net.2.weight", "q_net.q_net.2.bias",
                                      "q_net.tau_embedding.weight", "q_net.tau_embedding.bias"]
    assert [tuple(p.shape) for p in net._param_list()] == [(4, 16), (4,), (8, 4), (8,), (4, 8), (4,)]            # the kernels' order: the embedding first
    assert net.midpoints.tolist() == [0.125, 0.375, 0.625, 0.875]
    noisy = DQNPolicy(env.observation_space, env.action_space, n_tau_samples=8, net_arch=(8,), noisy=True)
    assert all(type(m) is NoisyLinear for m in noisy.q_net.q_net if isinstance(m, torch.nn.Linear))
    assert type(noisy.q_net.tau_embedding) is torch.nn.Linear                  # the embedding is always plain
    assert {"q_net.tau_embedding.weight", "q_net.tau_embedding.bias", "q_net.q_net.0.weight_sigma"} <= set(noisy.state_dict())
    model = DQN(DQNPolicy, env, device="cpu", n_tau_samples=8, n_tau_prime_samples=5, n_act_samples=4, n_cos=16)
    assert type(model.policy.q_net) is ImplicitQuantileQNetwork and type(model.target.q_net) is ImplicitQuantileQNetwork
    assert (model.n_tau_samples, model.n_tau_prime_samples, model.n_act_samples, model.n_cos, model.huber_kappa) == (8, 5, 4, 16, 1.0)
    assert (model.policy.q_net.n_act_samples, model.policy.q_net.n_cos) == (4, 16)
    for bad in (dict(n_tau_samples=8, n_atoms=51), dict(n_tau_samples=8, n_quantiles=4)):
        with pytest.raises(ValueError, match="n_tau_samples"):
            DQNPolicy(env.observation_space, env.action_space, **bad)
    with pytest.raises(ValueError, match="dueling.*n_tau_samples"):
        DQNPolicy(env.observation_space, env.action_space, n_tau_samples=8, dueling=True)
    # a policy instance whose head disagrees with the arguments
    for kw in (dict(), dict(n_tau_samples=8), dict(n_tau_samples=8, n_act_samples=4), dict(n_tau_samples=8, n_cos=16)):
        with pytest.raises(ValueError, match="n_tau_samples"):
            DQN(pol, env, device="cpu", **kw)
    with pytest.raises(ValueError, match="n_tau_samples"):
        DQN(plain, env, device="cpu", n_tau_samples=8)
    DQN(pol, env, device="cpu", n_tau_samples=3, n_act_samples=4, n_cos=16)    # the sample counts of an update are the algorithm's alone
    for call in (lambda: net.quantiles(torch.zeros(2, 4), torch.zeros(2, 3)), lambda: net.quantile_values(torch.zeros(2, 4), torch.zeros(2, 3)),
                 lambda: net(torch.zeros(2, 4)), lambda: pol.act(torch.zeros(2, 4), deterministic=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_a_checkpoint_without_the_new_keys_loads_with_the_defaults(tmp_path):
    """what an earlier version wrote has none of the four arguments under ``hyper``: it loads, and they keep their defaults; a checkpoint
    that disagrees about the head is refused by the argument's name"""
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env = _env()
    model = DQN(DQNPolicy, env, device="cpu", policy_kwargs=dict(net_arch=(8,)))
    path = str(tmp_path / "old.pt")
    model.save(path)
    ck = torch.load(path, weights_only=True)
    assert {k: ck["hyper"][k] for k in NEW_KWARGS} == NEW_KWARGS
    for k in NEW_KWARGS:
        del ck["hyper"][k]
    torch.save(ck, path)
    other = DQN(DQNPolicy, env, device="cpu", seed=3, policy_kwargs=dict(net_arch=(8,)))
    assert other.load(path) is other and {k: getattr(other, k) for k in NEW_KWARGS} == NEW_KWARGS and torch.equal(other.flat_p, model.flat_p)
    iqn = DQN(DQNPolicy, env, device="cpu", n_tau_samples=8, n_cos=16, policy_kwargs=dict(net_arch=(8,)))
    keep = iqn.flat_p.clone()
    with pytest.raises(ValueError, match="n_tau_samples = 0, this instance has n_tau_samples = 8"):
        iqn.load(path)
    ipath = str(tmp_path / "iqn.pt")
    iqn.save(ipath)
    with pytest.raises(ValueError, match="n_tau_samples = 8, this instance has n_tau_samples = 0"):
        other.load(ipath)
    for kw, name in ((dict(n_tau_samples=8, n_cos=32), "n_cos"), (dict(n_tau_samples=4, n_cos=16), "n_tau_samples"),
                     (dict(n_tau_samples=8, n_cos=16, n_act_samples=8), "n_act_samples"), (dict(n_tau_samples=8, n_cos=16, n_tau_prime_samples=4), "n_tau_prime_samples")):
        with pytest.raises(ValueError, match=f"the checkpoint was written with {name}"):
            DQN(DQNPolicy, env, device="cpu", policy_kwargs=dict(net_arch=(8,)), **kw).load(ipath)
    twin = DQN(DQNPolicy, env, device="cpu", seed=5, n_tau_samples=8, n_cos=16, policy_kwargs=dict(net_arch=(8,)))
    assert twin.load(ipath) is twin and torch.equal(twin.flat_p, keep) and torch.equal(iqn.flat_p, keep)
