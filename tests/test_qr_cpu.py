"""What DQN's quantile head promises without a GPU: the header (include/ocrl_hip_qr.h) parses, binds and is exported; the Makefile lists
the new parts; every rejection its entry points make before a launch; the hand-worked values of tests/qr_ref.py; the qrdqn config; and the
ValueErrors of DQN's new arguments."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import qr_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
FUNCTIONS = {"ocrl_qr_desc_size": 0, "ocrl_qr_ws_floats": 1, "ocrl_qr_fwd": 9, "ocrl_qr_bwd": 9, "ocrl_qr_act": 10, "ocrl_qr_td_fwd_bwd": 19}
NEW_KWARGS = dict(n_quantiles=0, huber_kappa=1.0)


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_qr.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {} and set(abi.structs) == {"ocrl_qr_desc"}
    assert [f[0] for f in abi.structs["ocrl_qr_desc"]._fields_] == ["B", "F", "A", "N", "n", "dueling", "dims", "acts"]
    assert all(t in (ctypes.c_int, ctypes.c_int * 8) for _, t in abi.structs["ocrl_qr_desc"]._fields_)          # int fields only
    assert set(_lib.ABI_QR.functions) == set(FUNCTIONS)
    L = _lib.lib()
    for name, n in FUNCTIONS.items():
        assert len(getattr(L, name).argtypes) == n, name
    td = L.ocrl_qr_td_fwd_bwd.argtypes
    assert L.ocrl_qr_ws_floats.restype is ctypes.c_size_t and td[10] is ctypes.c_float and td[11] is ctypes.c_float      # gamma, kappa
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_QR_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                      # self-contained
    assert _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    older = set(_lib.ABI.functions) | set(_lib.ABI_DQN.functions) | set(_lib.ABI_REPLAY.functions) | set(_lib.ABI_C51.functions)
    assert not set(FUNCTIONS) & older


def test_the_makefile_lists_the_new_parts():
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    srcs, objs, hdrs = (re.search(rf"^{k} = (.*)$", makefile, re.M).group(1).split() for k in ("SRCS", "OBJS", "HDRS"))
    assert "qr.hip" in srcs and "qr_unit.o" in objs and "qr.h" in hdrs and "../../include/ocrl_hip_qr.h" in hdrs
    assert "qhead_tile.h" in hdrs
    for dep, objects in (("acnet.h", ("qr.o", "qr_unit.o")), ("acnet_tile.h", ("qr.o",)), ("acnet_host.h", ("qr_unit.o",)), ("qhead_tile.h", ("qr.o",))):
        line = re.search(rf"^([^#\n]*): {re.escape(dep)}$", makefile, re.M).group(1).split()
        assert set(objects) <= set(line), (dep, line)
    for f in ("qr.hip", "qr.h", "qr_unit.cpp"):
        assert os.path.exists(os.path.join(ROOT, "ocrl_amd", "csrc", f)), f


def test_descriptor_size_is_the_ctypes_struct():
    assert _lib.lib().ocrl_qr_desc_size() == ctypes.sizeof(_lib.QrDesc) == 22 * 4
    d = _lib.qr_desc(5, 8, 4, 50, [64, 32], [1, 2], dueling=True)
    assert (d.B, d.F, d.A, d.N, d.n, d.dueling, list(d.dims)[:3], list(d.acts)[:3]) == (5, 8, 4, 50, 2, 1, [64, 32, 0], [1, 2, 0])
    with pytest.raises(ValueError, match="at most 8 hidden layers"):
        _lib.qr_desc(5, 8, 4, 50, [4] * 9, [1] * 9)


# ---- rejections before any launch
def test_arguments_are_checked_before_any_launch():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)
    desc = lambda A=4, N=50, dueling=True, dims=(8, 8), B=5, F=8: _lib.qr_desc(B, F, A, N, list(dims), [1] * len(dims), dueling)
    good = desc()
    w = (ctypes.c_void_p * 8)(*[FAKE] * 8)
    hole = (ctypes.c_void_p * 8)(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE)
    big = 1 << 40

    def fwd(d=good, ww=w, outs=(p, p), save=0, ws=None, n=0):
        return L.ocrl_qr_fwd(ctypes.byref(d) if d is not None else None, p, ww, *outs, save, ws, n, None)

    def bwd(d=good, ww=w, dw=w, dq=p, n=big):
        return L.ocrl_qr_bwd(ctypes.byref(d), p, ww, dq, None, dw, p, n, None)

    def act(d=good, ww=w, actions=p):
        return L.ocrl_qr_act(ctypes.byref(d), p, ww, 0, 0, 0.1, None, actions, None, None)

    def td(d=good, ww=w, dw=w, kappa=1.0, nq=p, n=big):
        return L.ocrl_qr_td_fwd_bwd(ctypes.byref(d), p, ww, nq, p, p, p, p, None, None, 0.99, kappa, p, None, None, dw, p, n, None)

    limits = ((desc(N=0), "1 <= n_quantiles <= 64"), (desc(N=65, A=2), "1 <= n_quantiles <= 64"), (desc(A=5, N=52), "n_actions * n_quantiles <= 256"),
              (desc(A=65, N=2), "1 <= n_actions <= 64"), (desc(A=0), "1 <= n_actions <= 64"), (desc(dims=(6,)), "multiples of 4"),
              (desc(dims=(260,)), "multiples of 4"), (desc(B=0), "batch >= 1"), (desc(F=0), "feature_dim >= 1"))
    assert limits[2][0].A * limits[2][0].N == 260
    for bad, msg in limits:
        for call in (fwd, bwd, act, td):
            assert call(d=bad) != 0 and msg in last_error(), (msg, last_error())
        assert L.ocrl_qr_ws_floats(ctypes.byref(bad)) == 0 and msg in last_error()
    nine = desc()
    nine.n = 9
    for call, msg in ((lambda: fwd(d=None), "ocrl_qr_fwd: null descriptor"),
                      (lambda: fwd(d=nine), "at most 8 hidden layers"),
                      (lambda: td(kappa=0.0), "ocrl_qr_td_fwd_bwd: kappa finite and > 0"),
                      (lambda: td(kappa=float("inf")), "kappa finite and > 0"),
                      (lambda: td(kappa=-1.0), "kappa finite and > 0"),
                      (lambda: td(kappa=float("nan")), "kappa finite and > 0"),
                      (lambda: fwd(outs=(None, None)), "quantiles and q are both null"),
                      (lambda: fwd(ww=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: fwd(ww=None), "ocrl_qr_fwd: null argument"),
                      (lambda: fwd(save=1, ws=p, n=8), "workspace too small"),
                      (lambda: fwd(save=1, ws=None, n=big), "workspace too small"),
                      (lambda: bwd(dw=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: bwd(dq=None), "ocrl_qr_bwd: null argument"),
                      (lambda: bwd(n=8), "workspace too small"),
                      (lambda: act(ww=hole), "parameter pointer 6 of 8 is null"),
                      (lambda: act(actions=None), "ocrl_qr_act: null argument"),
                      (lambda: td(nq=None), "ocrl_qr_td_fwd_bwd: null argument"),
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
    n_par = 8 * 8 + 8 + 8 * 8 + 8 + 200 * 8 + 200 + 50 * 8 + 50
    assert L.ocrl_qr_ws_floats(ctypes.byref(d)) == 2 * up(37 * 8) + up(3 * n_par) + up(3 * 8)
    assert L.ocrl_qr_ws_floats(ctypes.byref(desc(N=1, A=1))) > 0 and L.ocrl_qr_ws_floats(ctypes.byref(desc(N=64, A=4))) > 0      # the limits themselves


# ---- the restatement against values worked on paper (tests/qr_ref.py's docstring)
def test_one_quantile_is_half_the_huber_loss():
    """N = 1: tau = 0.5 for either sign of u, so ql = 0.5 L(T - theta).  theta 0.25: T 0.75 -> 0.5 * 0.5 * 0.5^2 = 0.0625 (quadratic),
    T 3.25 -> 0.5 * 1 * (3 - 0.5) = 1.25 (linear), T -2.75 -> the same 1.25 (u = -3)."""
    assert Q.taus(1).tolist() == [0.5]
    for T, want in ((0.75, 0.0625), (3.25, 1.25), (-2.75, 1.25)):
        f = torch.tensor([[[T]]], dtype=torch.float64)
        loss, mq, mt, ql = Q.qr_loss(torch.tensor([[[0.25]]], dtype=torch.float64), f, torch.zeros(1, 1, dtype=torch.float64), torch.tensor([0]),
                                     torch.zeros(1, dtype=torch.float64), torch.tensor([0], dtype=torch.uint8), 1.0)
        assert ql.tolist() == [want] and loss.item() == want and mq.item() == 0.25 and mt.item() == T
    # kappa 2: u = 3 -> 0.5 * 2 * (3 - 1) = 2
    f = torch.tensor([[[3.25]]], dtype=torch.float64)
    assert Q.qr_loss(torch.tensor([[[0.25]]], dtype=torch.float64), f, torch.zeros(1, 1, dtype=torch.float64), torch.tensor([0]),
                     torch.zeros(1, dtype=torch.float64), torch.tensor([0], dtype=torch.uint8), 1.0, kappa=2.0)[3].tolist() == [2.0]


def test_two_quantiles_worked_on_paper():
    """N = 2, theta = (0, 1), T = (0.5, 3), kappa = 1, tau = (0.25, 0.75).
    i = 0: u = (0.5, 3), both >= 0, weight 0.25 each:   0.25 * (0.5 * 0.25) + 0.25 * (3 - 0.5) = 0.03125 + 0.625  = 0.65625
    i = 1: u = (-0.5, 2): weights |0.75 - 1| = 0.25 and 0.75:   0.25 * 0.125 + 0.75 * (2 - 0.5)  = 0.03125 + 1.125  = 1.15625
    ql = (1 / 2) 0.65625 + (1 / 2) 1.15625 = 0.90625.
    dql/dtheta_i = -(1 / 2) sum_j weight * clamp(u, -1, 1):  i = 0: -(0.25 * 0.5 + 0.25 * 1) / 2 = -0.1875;  i = 1: -(-0.25 * 0.5 + 0.75 * 1) / 2
    = -0.3125.  With the row's weight 2 the loss and the gradient double, row_loss does not."""
    assert Q.taus(2).tolist() == [0.25, 0.75]
    theta = torch.tensor([[[0.0, 1.0]]], dtype=torch.float64, requires_grad=True)
    nxt = torch.tensor([[[0.5, 3.0]]], dtype=torch.float64)
    args = (nxt, torch.zeros(1, 1, dtype=torch.float64), torch.tensor([0]), torch.zeros(1, dtype=torch.float64), torch.tensor([0], dtype=torch.uint8), 1.0)
    loss, mq, mt, ql = Q.qr_loss(theta, *args)
    assert ql.tolist() == [0.90625] and loss.item() == 0.90625 and mq.item() == 0.5 and mt.item() == 1.75
    assert torch.autograd.grad(loss, theta)[0].flatten().tolist() == [-0.1875, -0.3125]
    loss2, _, _, ql2 = Q.qr_loss(theta, *args, weights=torch.tensor([2.0], dtype=torch.float64))
    assert loss2.item() == 1.8125 and ql2.tolist() == [0.90625] and torch.autograd.grad(loss2, theta)[0].flatten().tolist() == [-0.375, -0.625]
    # a finished row: T = r, its NaN next quantiles and infinite next_q are never read.  r = 0.5: u = (0.5, 0.5 | -0.5, -0.5):
    # i = 0: 2 * 0.25 * 0.125 = 0.0625, i = 1: 2 * 0.25 * 0.125 = 0.0625, ql = 0.0625
    done = Q.qr_loss(theta, torch.full((1, 1, 2), float("nan"), dtype=torch.float64), torch.full((1, 1), float("inf"), dtype=torch.float64),
                     torch.tensor([7]), torch.tensor([0.5], dtype=torch.float64), torch.tensor([1], dtype=torch.uint8), 0.9)
    assert done[3].tolist() == [0.0625] and done[2].item() == 0.5


def test_the_head_of_the_restatement():
    """the dueling rule on quantile values and the mean q; a tie of next_q takes the lower action"""
    ps = Q.make_params(6, 3, 5, (8,), True, 4, torch.float64)
    assert [tuple(p.shape) for p in ps] == [(8, 6), (8,), (15, 8), (15,), (5, 8), (5,)]
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    theta, q = Q.quantiles(x, ps, (1,), 3, 5, True)
    h = torch.relu(x @ ps[0].T + ps[1])
    assert theta.shape == (4, 3, 5) and torch.allclose(theta.mean(dim=1), h @ ps[4].T + ps[5]) and torch.allclose(q, theta.mean(-1))
    nxt = torch.arange(12, dtype=torch.float64).reshape(1, 3, 4)
    T = Q.targets(nxt, torch.tensor([[1.0, 2.0, 2.0]], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64), torch.tensor([0], dtype=torch.uint8),
                  torch.tensor([0.5], dtype=torch.float64))
    assert T.tolist() == [[3.0, 3.5, 4.0, 4.5]]                              # action 1's quantiles 4 .. 7


# ---- config and the algorithm's arguments
def test_qrdqn_config_composes_and_its_kwargs_are_dqns():
    from ocrl_amd import sb3s
    rainbow, qr = compose(os.path.join(CFG, "sb3"), "rainbow").to_dict(), compose(os.path.join(CFG, "sb3"), "qrdqn").to_dict()
    assert qr["name"] == "DQN"
    want = {k: v for k, v in rainbow["algo_kwargs"].items() if k not in ("v_min", "v_max")}
    assert qr["algo_kwargs"] == dict(want, n_atoms=1, n_quantiles=50, huber_kappa=1.0)
    params = inspect.signature(sb3s.DQN.__init__).parameters
    assert set(qr["algo_kwargs"]) <= set(params) and {k: params[k].default for k in NEW_KWARGS} == NEW_KWARGS
    assert {"n_quantiles", "huber_kappa"} <= set(sb3s.DQN.HYPER)
    assert inspect.signature(sb3s.DQNPolicy.__init__).parameters["n_quantiles"].default == 0
    full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=qrdqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
    assert full.sb3.to_dict() == qr
    assert {"QuantileQNetwork", "qr_loss"} <= set(sb3s.__all__)
    lp = inspect.signature(sb3s.qr_loss).parameters
    assert list(lp) == ["policy", "features", "next_quantiles", "next_q", "actions", "rewards", "dones", "gamma", "kappa", "discounts", "weights"]
    assert lp["kappa"].default == 1.0
    import train_sb3
    assert set(train_sb3.ALGOS) == {"PPO", "A2C", "DQN"}


def _env(n=4):
    return types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=n))


@pytest.mark.parametrize("kw, n, name", [(dict(n_quantiles=-1), 4, "n_quantiles"), (dict(n_quantiles=65), 4, "n_quantiles"),
                                         (dict(n_quantiles=52), 5, r"n_actions \* n_quantiles"), (dict(n_quantiles=8, huber_kappa=0.0), 4, "huber_kappa"),
                                         (dict(n_quantiles=8, huber_kappa=-1.0), 4, "huber_kappa"), (dict(huber_kappa=float("nan")), 4, "huber_kappa"),
                                         (dict(n_quantiles=8, n_atoms=51), 4, "n_quantiles > 0 and n_atoms > 1")])
def test_bad_values_name_their_argument(kw, n, name):
    from ocrl_amd.sb3s import DQN, DQNPolicy
    with pytest.raises(ValueError, match=name):
        DQN(DQNPolicy, _env(n), **kw)


def test_the_head_follows_the_arguments():
    from ocrl_amd.sb3s import DQN, DQNPolicy, NoisyLinear, QNetwork, QuantileQNetwork
    env = _env()
    plain = DQNPolicy(env.observation_space, env.action_space)
    assert type(plain.q_net) is QNetwork and plain.n_quantiles == 0
    qr = DQNPolicy(env.observation_space, env.action_space, n_quantiles=11, dueling=True, net_arch=(8,))
    net = qr.q_net
    assert type(net) is QuantileQNetwork and (net.n_actions, net.n_quantiles, net.dueling) == (4, 11, True)
    assert list(qr.state_dict()) == ["q_net.q_net.0.weight", "q_net.q_net.0.bias", "q_net.q_net.2.weight", "q_net.q_net.2.bias",
                                     "q_net.value_net.weight", "q_net.value_net.bias"]
    assert [tuple(p.shape) for p in net._param_list()] == [(8, 4), (8,), (44, 8), (44,), (11, 8), (11,)]
    assert torch.allclose(net.taus, (torch.arange(11.0) + 0.5) / 11)
    noisy = DQNPolicy(env.observation_space, env.action_space, n_quantiles=5, dueling=True, net_arch=(8,), noisy=True)
    assert all(type(m) is NoisyLinear for m in noisy.q_net.modules() if isinstance(m, torch.nn.Linear)) and type(noisy.q_net.value_net) is NoisyLinear
    # dueling is accepted with the quantile head; without either distributional head it keeps raising today's message
    model = DQN(DQNPolicy, env, device="cpu", n_quantiles=8, dueling=True)
    assert type(model.policy.q_net) is QuantileQNetwork and type(model.target.q_net) is QuantileQNetwork and model.policy.q_net.dueling
    assert (model.n_quantiles, model.huber_kappa) == (8, 1.0)
    with pytest.raises(ValueError, match="dueling is built for the categorical head only: set n_atoms >= 2"):
        DQN(DQNPolicy, env, device="cpu", dueling=True)
    with pytest.raises(ValueError, match="n_quantiles"):
        DQNPolicy(env.observation_space, env.action_space, n_quantiles=8, n_atoms=51)
    # a policy instance whose head disagrees with the arguments
    for kw in (dict(dueling=True), dict(n_quantiles=8, dueling=True), dict(n_quantiles=11)):
        with pytest.raises(ValueError, match="n_quantiles|dueling"):
            DQN(qr, env, device="cpu", **kw)
    with pytest.raises(ValueError, match="n_quantiles"):
        DQN(plain, env, device="cpu", n_quantiles=11)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.quantiles(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.quantile_values(torch.zeros(2, 4))


def test_a_checkpoint_without_the_new_keys_loads_with_the_defaults(tmp_path):
    """what an earlier version wrote has neither n_quantiles nor huber_kappa under ``hyper``: it loads, and the two keep their defaults"""
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env = _env()
    model = DQN(DQNPolicy, env, device="cpu", policy_kwargs=dict(net_arch=(8,)))
    path = str(tmp_path / "old.pt")
    model.save(path)
    ck = torch.load(path, weights_only=True)
    assert ck["hyper"]["n_quantiles"] == 0 and ck["hyper"]["huber_kappa"] == 1.0
    del ck["hyper"]["n_quantiles"], ck["hyper"]["huber_kappa"]
    torch.save(ck, path)
    other = DQN(DQNPolicy, env, device="cpu", seed=3, policy_kwargs=dict(net_arch=(8,)))
    assert other.load(path) is other and (other.n_quantiles, other.huber_kappa) == (0, 1.0) and torch.equal(other.flat_p, model.flat_p)
    # a quantile head's checkpoint is refused by name where the instance has none of the same layout
    qr = DQN(DQNPolicy, env, device="cpu", n_quantiles=1, policy_kwargs=dict(net_arch=(8,)))
    with pytest.raises(ValueError, match="n_quantiles|Adam entries"):
        qr.load(path)
