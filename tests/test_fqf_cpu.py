"""What DQN's fully parameterized quantile function promises without a GPU: the header (include/ocrl_hip_fqf.h) parses, binds and is
exported; the Makefile lists the new parts; every rejection the entry points make before a launch; the fqf config; the ValueErrors of
DQN's new arguments; the state_dict keys; checkpoints with and without the new keys; and the restatement of tests/fqf_ref.py against
itself: the analytic dW1 / dtau against autograd of the exact integral, dz against autograd through log_softmax and cumsum."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import fqf_ref as FQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
NEW_KWARGS = dict(fqf=False, fqf_fraction_lr=2.5e-9, fqf_ent_coef=0.0)
ON = dict(fqf=True, fqf_fraction_lr=2.5e-9, fqf_ent_coef=0.0)
FUNCS = {"ocrl_fqf_desc_size": 0, "ocrl_fqf_ws_floats": 3, "ocrl_fqf_fractions": 12, "ocrl_fqf_q": 7, "ocrl_fqf_act": 11, "ocrl_fqf_fraction_bwd": 17}
f64 = torch.float64


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    path = os.path.join(ROOT, "include", "ocrl_hip_fqf.h")
    text = open(path).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCS and abi.consts == {} and set(abi.structs) == {"ocrl_fqf_desc"}
    assert set(_lib.ABI_FQF.functions) == set(FUNCS) and os.path.samefile(_lib.FQF_HEADER_PATH, path)
    L = _lib.lib()
    for name in FUNCS:
        assert len(getattr(L, name).argtypes) == FUNCS[name], name
    assert L.ocrl_fqf_ws_floats.restype is ctypes.c_size_t and L.ocrl_fqf_desc_size() == ctypes.sizeof(_lib.FqfDesc) == ctypes.sizeof(_lib.IqnDesc)
    assert [f[0] for f in _lib.FqfDesc._fields_] == [f[0] for f in _lib.IqnDesc._fields_]
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_FQF_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                      # self-contained
    assert _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    older = [_lib.ABI, _lib.ABI_DQN, _lib.ABI_ROLLOUT, _lib.ABI_REPLAY, _lib.ABI_C51, _lib.ABI_NOISY, _lib.ABI_CLASSIFIER, _lib.ABI_IODINE, _lib.ABI_QR,
             _lib.ABI_IQN, _lib.ABI_MUNCHAUSEN, _lib.ABI_SLATE_KERNELS, _lib.ABI_VIT_KERNELS]
    assert len(older) == 13 and not set(FUNCS) & set().union(*(set(a.functions) for a in older))
    assert "include/ocrl_hip_fqf.h" in _lib.__doc__


def test_the_makefile_lists_the_new_parts():
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    srcs, objs, hdrs = (re.search(rf"^{k} = (.*)$", makefile, re.M).group(1).split() for k in ("SRCS", "OBJS", "HDRS"))
    assert "fqf.hip" in srcs and "fqf_unit.o" in objs and "fqf.h" in hdrs and "../../include/ocrl_hip_fqf.h" in hdrs
    assert re.search(r"^fqf\.o: CXXFLAGS \+= -ffp-contract=off$", makefile, re.M)
    for f in ("fqf.hip", "fqf.h", "fqf_unit.cpp"):
        assert os.path.exists(os.path.join(ROOT, "ocrl_amd", "csrc", f)), f


# ---- rejections before the launch
LIMITS = [(dict(B=0), "batch >= 1"), (dict(B=-2), "batch >= 1"), (dict(F=0), "feature_dim is a multiple of 4 in 4 .. 256"),
          (dict(F=6), "feature_dim is a multiple of 4 in 4 .. 256"), (dict(F=260), "feature_dim is a multiple of 4 in 4 .. 256"),
          (dict(N=1), "2 <= n_fractions <= 32"), (dict(N=33), "2 <= n_fractions <= 32"), (dict(N=0), "2 <= n_fractions <= 32"),
          (dict(A=0), "1 <= n_actions <= 64"), (dict(A=65), "1 <= n_actions <= 64")]


def test_arguments_are_checked_before_the_launch():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)

    def fractions(B=5, F=8, N=8, A=None, x=p, W=p, b=p, taus=p):
        return L.ocrl_fqf_fractions(x, W, b, B, F, N, taus, p, p, p, p, None)

    def q(B=5, A=4, N=8, F=None, th=p, taus=p, out=p):
        return L.ocrl_fqf_q(th, taus, B, A, N, out, None)

    def bwd(B=5, F=8, A=4, N=8, ent=0.0, x=p, logp=p, H=p, th=p, actions=p, dW=p, db=p, scal=p, ws=p, n=1 << 20):
        return L.ocrl_fqf_fraction_bwd(x, logp, H, th, actions, None, ent, B, F, A, N, dW, db, scal, ws, n, None)

    def act(B=5, F=8, A=4, N=8, C=8, dims=(8,), acts=(1,), d=True, x=p, w=True, taus=p, actions=p):
        desc = _lib.fqf_desc(B, F, A, N, C, dims, acts)
        return L.ocrl_fqf_act(ctypes.byref(desc) if d else None, x, _lib.ptrs([None] * 0) if not w else (ctypes.c_void_p * 6)(*[FAKE] * 6), taus, 1, 0,
                              0.1, None, actions, p, None)

    def ws(B=5, F=8, N=8, A=None):
        return 0 if L.ocrl_fqf_ws_floats(B, F, N) else 1

    for fn, name, takes in ((fractions, "ocrl_fqf_fractions", "BFN"), (q, "ocrl_fqf_q", "BAN"), (bwd, "ocrl_fqf_fraction_bwd", "BFAN"),
                            (act, "ocrl_fqf_act", "BFAN"), (ws, "ocrl_fqf_ws_floats", "BFN")):
        for kw, msg in LIMITS:
            if next(iter(kw)) not in takes:
                continue
            assert fn(**kw) != 0 and f"{name}: " in last_error() and msg in last_error(), (name, kw, msg, last_error())
    assert L.ocrl_fqf_ws_floats(5, 8, 8) == 64 + 64 and L.ocrl_fqf_ws_floats(130, 8, 8) == 16 * 128 and L.ocrl_fqf_ws_floats(3, 256, 32) == 8256
    for fn, name, kws in ((fractions, "ocrl_fqf_fractions", [dict(x=None), dict(W=None), dict(b=None), dict(taus=None)]),
                          (q, "ocrl_fqf_q", [dict(th=None), dict(taus=None), dict(out=None)]),
                          (bwd, "ocrl_fqf_fraction_bwd", [dict(x=None), dict(logp=None), dict(H=None), dict(th=None), dict(actions=None), dict(dW=None),
                                                          dict(db=None), dict(scal=None), dict(ws=None)]),
                          (act, "ocrl_fqf_act", [dict(x=None), dict(taus=None), dict(actions=None)])):
        for kw in kws:
            assert fn(**kw) != 0 and f"{name}: null argument" in last_error(), (name, kw, last_error())
    assert act(d=False) != 0 and "ocrl_fqf_act: null descriptor" in last_error()
    assert bwd(n=127) != 0 and "ocrl_fqf_fraction_bwd: workspace of 127 floats, ocrl_fqf_ws_floats asks for 128" in last_error()
    for ent in (float("nan"), float("inf")):
        assert bwd(ent=ent) != 0 and "ocrl_fqf_fraction_bwd: ent_coef finite" in last_error()
    # the head's own limits reach ocrl_fqf_act under its name
    for kw, msg in ((dict(C=6), "n_cos is a multiple of 4 in 4 .. 64"), (dict(C=68), "n_cos"), (dict(dims=(6,)), "ocrl_fqf_act: ")):
        assert act(**kw) != 0 and "ocrl_fqf_act: " in last_error() and msg in last_error(), (kw, last_error())


# ---- config and the algorithm's arguments
def test_the_config_composes_and_its_kwargs_are_dqns():
    from ocrl_amd import sb3s
    sb3 = lambda name: compose(os.path.join(CFG, "sb3"), name).to_dict()
    iqn, fqf = sb3("iqn"), sb3("fqf")
    assert fqf["name"] == "DQN"
    assert fqf["algo_kwargs"] == dict(iqn["algo_kwargs"], n_tau_samples=32, n_tau_prime_samples=0, **ON)
    params = inspect.signature(sb3s.DQN.__init__).parameters
    assert set(fqf["algo_kwargs"]) <= set(params)
    assert {k: params[k].default for k in NEW_KWARGS} == NEW_KWARGS and set(NEW_KWARGS) <= set(sb3s.DQN.HYPER)
    assert inspect.signature(sb3s.DQNPolicy.__init__).parameters["fqf"].default is False
    text = open(os.path.join(CFG, "sb3", "fqf.yaml")).read()
    assert text.startswith("# ") and "include/ocrl_hip_fqf.h" in text
    full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=fqf", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
    assert full.sb3.to_dict() == fqf
    assert {"FullyParameterizedQuantileQNetwork", "fqf_fraction_loss"} <= set(sb3s.__all__)
    fp = inspect.signature(sb3s.fqf_fraction_loss).parameters
    assert list(fp)[:5] == ["policy", "features", "actions", "weights", "ent_coef"] and fp["weights"].default is None and fp["ent_coef"].default == 0.0
    assert all(v.default is not inspect.Parameter.empty for v in list(fp.values())[5:])
    import train_sb3
    assert set(train_sb3.ALGOS) == {"PPO", "A2C", "DQN"} and "sb3=fqf" in train_sb3.__doc__


def _env(n=4):
    return types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=n))


@pytest.mark.parametrize("kw, name", [(dict(fqf=True), "fqf.*n_tau_samples"), (dict(fqf=True, n_tau_samples=0), "fqf.*n_tau_samples"),
                                      (dict(fqf=True, n_tau_samples=1), "fqf.*n_tau_samples"), (dict(fqf=True, n_tau_samples=33), "fqf.*n_tau_samples"),
                                      (dict(fqf=True, n_tau_samples=8, n_tau_prime_samples=5), "fqf.*n_tau_prime_samples"),
                                      (dict(fqf=True, n_tau_samples=8, munchausen=True), "fqf.*munchausen"),
                                      (dict(fqf=True, n_tau_samples=8, dueling=True), "fqf.*dueling"),
                                      (dict(fqf=True, n_tau_samples=8, n_atoms=51), "fqf.*n_atoms"),
                                      (dict(fqf=True, n_tau_samples=8, n_quantiles=8), "fqf.*n_quantiles"),
                                      (dict(fqf_fraction_lr=-1.0), "fqf_fraction_lr"), (dict(fqf_ent_coef=float("nan")), "fqf_ent_coef")])
def test_refusals_name_their_arguments(kw, name):
    from ocrl_amd.sb3s import DQN, DQNPolicy
    with pytest.raises(ValueError, match=name):
        DQN(DQNPolicy, _env(), device="cpu", **kw)


def test_the_policy_refuses_too_and_a_mismatch_is_named():
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env = _env()
    for kw, name in ((dict(fqf=True), "fqf.*n_tau_samples"), (dict(fqf=True, n_tau_samples=40), "fqf.*n_tau_samples"),
                     (dict(fqf=True, n_tau_samples=8, dueling=True), "fqf.*dueling"), (dict(fqf=True, n_tau_samples=8, n_atoms=51), "fqf.*n_atoms")):
        with pytest.raises(ValueError, match=name):
            DQNPolicy(env.observation_space, env.action_space, **kw)
    plain = DQNPolicy(env.observation_space, env.action_space, n_tau_samples=8, net_arch=(8,))
    with pytest.raises(ValueError, match="the policy's head has fqf = False.*the arguments say fqf = True"):
        DQN(plain, env, device="cpu", fqf=True, n_tau_samples=8)


def test_state_dict_keys_and_the_buffers():
    """an IQN policy's keys are what they were; an fqf one adds exactly the proposal's two; the proposal lives outside flat_p"""
    from ocrl_amd import sb3s
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env, arch = _env(), dict(policy_kwargs=dict(net_arch=(8,)))
    iqn = DQN(DQNPolicy, env, device="cpu", n_tau_samples=8, **arch)
    fqf = DQN(DQNPolicy, env, device="cpu", fqf=True, n_tau_samples=8, n_act_samples=7, noisy=True, double_q=True, n_step=3, prioritized_replay=True, **arch)
    keys = ["q_net.q_net.0.weight", "q_net.q_net.0.bias", "q_net.q_net.2.weight", "q_net.q_net.2.bias", "q_net.tau_embedding.weight", "q_net.tau_embedding.bias"]
    assert list(iqn.policy.state_dict()) == keys and type(iqn.policy.q_net) is sb3s.ImplicitQuantileQNetwork
    assert not hasattr(iqn, "frac_p") and not hasattr(iqn.policy.q_net, "fraction_net") and iqn.fqf is False
    plain = DQN(DQNPolicy, env, device="cpu", fqf=True, n_tau_samples=8, **arch)
    assert set(plain.policy.state_dict()) - set(keys) == {"q_net.fraction_net.weight", "q_net.fraction_net.bias"} and set(keys) <= set(plain.policy.state_dict())
    assert set(fqf.policy.state_dict()) - set(iqn.policy.state_dict()) >= {"q_net.fraction_net.weight", "q_net.fraction_net.bias"}
    assert not any("fraction_net" in k and "sigma" in k for k in fqf.policy.state_dict())          # never noisy
    for m in (plain, fqf):
        net = m.policy.q_net
        assert type(net) is sb3s.FullyParameterizedQuantileQNetwork and type(m.target.q_net) is sb3s.FullyParameterizedQuantileQNetwork
        W, b = net.fraction_net.weight, net.fraction_net.bias
        assert tuple(W.shape) == (8, 4) and (b == 0).all() and W.abs().max() <= 0.01 * (6 / 12) ** 0.5 + 1e-9 and (W != 0).any()
        assert m.frac_p.numel() == 40 and (m.frac_sq == 1).all() and (m.frac_g == 0).all()
        assert W.data_ptr() == m.frac_p.data_ptr() and W.grad.data_ptr() == m.frac_g.data_ptr() and b.grad.data_ptr() == m.frac_g[32:].data_ptr()
        assert m.flat_p.numel() == iqn.flat_p.numel() + (0 if m is plain else m.flat_p.numel() - iqn.flat_p.numel())
        assert all(not p.requires_grad for p in m.target.q_net.fraction_net.parameters())
        assert torch.equal(m.target.q_net.fraction_net.weight, W) and m.target.q_net.fraction_net.weight.data_ptr() != W.data_ptr()
        st = m.train_stats()
        assert {"fraction_loss", "fraction_entropy"} <= set(st)
    assert plain.flat_p.numel() == iqn.flat_p.numel() and "fraction_loss" not in iqn.train_stats()
    z = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        plain.policy.q_net.fractions(z)
    with pytest.raises(TypeError, match="not a FullyParameterizedQuantileQNetwork"):
        sb3s.fqf_fraction_loss(iqn.policy, z, torch.zeros(2, dtype=torch.int64))


def test_checkpoints_carry_the_three_values(tmp_path):
    """save writes them, the proposal and its square average; a mismatch is refused by the key's name; what an earlier version wrote
    has none of them and loads as fqf=False"""
    from ocrl_amd.sb3s import DQN, DQNPolicy
    env, arch = _env(), dict(policy_kwargs=dict(net_arch=(8,)), n_tau_samples=8)
    model = DQN(DQNPolicy, env, device="cpu", fqf=True, **arch)
    model.frac_sq.mul_(0.5)
    path = str(tmp_path / "f.pt")
    model.save(path)
    ck = torch.load(path, weights_only=True)
    assert {k: ck["hyper"][k] for k in ON} == ON and torch.equal(ck["optimizer"]["frac_sq"], model.frac_sq)
    assert "q_net.fraction_net.weight" in ck["policy"] and "q_net.fraction_net.bias" in ck["target"]
    twin = DQN(DQNPolicy, env, device="cpu", seed=4, fqf=True, **arch)
    assert not torch.equal(twin.frac_p, model.frac_p)
    assert twin.load(path) is twin and torch.equal(twin.flat_p, model.flat_p) and torch.equal(twin.frac_p, model.frac_p) and torch.equal(twin.frac_sq, model.frac_sq)
    assert twin.policy.q_net.fraction_net.weight.data_ptr() == twin.frac_p.data_ptr() and twin.fqf is True
    for kw, key in ((dict(), "fqf"), (dict(fqf=True, fqf_fraction_lr=1e-3), "fqf_fraction_lr"), (dict(fqf=True, fqf_ent_coef=0.01), "fqf_ent_coef")):
        other = DQN(DQNPolicy, env, device="cpu", seed=3, **arch, **kw)
        keep = other.flat_p.clone()
        with pytest.raises(ValueError, match=f"the checkpoint was written with {key} = "):
            other.load(path)
        assert torch.equal(other.flat_p, keep)
    iqn = DQN(DQNPolicy, env, device="cpu", **arch)
    old = str(tmp_path / "old.pt")
    iqn.save(old)
    ck = torch.load(old, weights_only=True)
    for k in ON:
        del ck["hyper"][k]                                   # as a version before these keys wrote it
    torch.save(ck, old)
    plain = DQN(DQNPolicy, env, device="cpu", seed=3, **arch)
    assert plain.load(old) is plain and {k: getattr(plain, k) for k in NEW_KWARGS} == NEW_KWARGS and torch.equal(plain.flat_p, iqn.flat_p)
    with pytest.raises(ValueError, match="the checkpoint was written with fqf = False, this instance has fqf = True"):
        DQN(DQNPolicy, env, device="cpu", fqf=True, **arch).load(old)


# ---- the restatement against itself
def _bounds(N, seed):
    gen = torch.Generator().manual_seed(seed)
    z = (torch.randn(1, N, generator=gen, dtype=f64) * 1.5).requires_grad_(True)
    p = torch.softmax(z, dim=1)
    return z, torch.cat([torch.zeros(1, 1, dtype=f64), p.cumsum(1)[:, :-1], torch.ones(1, 1, dtype=f64)], dim=1)[0]


# F^-1(w) = w^2, and one whose slope is not monotone (w + sin(2 pi w) / (4 pi): slope 1 + cos(2 pi w) / 2 > 0), with their primitives
QFS = {"square": (lambda w: w ** 2, lambda w: w ** 3 / 3),
       "wavy": (lambda w: w + torch.sin(2 * torch.pi * w) / (4 * torch.pi), lambda w: w ** 2 / 2 - torch.cos(2 * torch.pi * w) / (8 * torch.pi ** 2))}


@pytest.mark.parametrize("name", list(QFS))
@pytest.mark.parametrize("N", [2, 5, 32])
def test_the_analytic_gradient_is_autograd_of_the_exact_integral(name, N):
    Finv, prim = QFS[name]
    _, taus = _bounds(N, 7 + N)
    taus = taus.detach().requires_grad_(True)
    want = torch.autograd.grad(FQ.w1_exact(taus, Finv, prim), taus)[0][1:-1]
    t = taus.detach()
    got = FQ.g_analytic(Finv(t[1:-1]), Finv(0.5 * (t[:-1] + t[1:])))
    assert got.shape == want.shape == (N - 1,) and (got - want).abs().max().item() <= 1e-14
    # and W1 itself is the integral: against a fine midpoint rule
    w = (torch.arange(200000, dtype=f64) + 0.5) / 200000
    stair = Finv(0.5 * (t[:-1] + t[1:]))[(torch.bucketize(w, t[1:-1].contiguous(), right=True))]
    assert abs((Finv(w) - stair).abs().mean().item() - FQ.w1_exact(t, Finv, prim).item()) <= 1e-6


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_dz_is_autograd_through_log_softmax_and_cumsum(ent_coef):
    B, N = 6, 9
    gen = torch.Generator().manual_seed(3)
    z = (torch.randn(B, N, generator=gen, dtype=f64) * 2).requires_grad_(True)
    g = torch.randn(B, N - 1, generator=gen, dtype=f64) / B
    want = torch.autograd.grad(FQ.fraction_objective(z, g, ent_coef), z)[0]
    logp = torch.log_softmax(z.detach(), dim=1)
    H = -(logp.exp() * logp).sum(1)
    got = FQ.fraction_dz(logp, H, g, ent_coef)
    assert (got - want).abs().max().item() <= 1e-15 and (ent_coef == 0.0 or (got - FQ.fraction_dz(logp, H, g, 0.0)).abs().max() > 1e-6)
    # through the Linear: fraction_grads is dz^T x, sum_b dz and the two scalars
    F, A = 4, 3
    x = torch.randn(B, F, generator=gen, dtype=f64)
    theta = torch.randn(B, A, 2 * N - 1, generator=gen, dtype=f64).cumsum(-1)
    actions, w = torch.tensor([0, 1, 2, -4, 9, 1]), torch.rand(B, generator=gen, dtype=f64) + 0.1
    th = theta[torch.arange(B), actions.clamp(0, A - 1)]
    g = (w / B).unsqueeze(1) * FQ.g_analytic(th[:, :N - 1], th[:, N - 1:])
    dW, db, scal = FQ.fraction_grads(x, logp, H, theta, actions, w, ent_coef)
    dz = FQ.fraction_dz(logp, H, g, ent_coef)
    assert torch.allclose(dW, dz.T @ x, atol=1e-15) and torch.allclose(db, dz.sum(0), atol=1e-15)
    assert abs(scal[0].item() - (g * logp.exp().cumsum(1)[:, :-1]).sum().item()) <= 1e-15 and abs(scal[1].item() - H.mean().item()) <= 1e-15


@pytest.mark.parametrize("dtype", [torch.float32, f64])
def test_the_fractions_start_at_0_end_at_1_and_never_fall(dtype):
    gen = torch.Generator().manual_seed(11)
    for N, gap in ((2, 1.0), (5, 3.0), (17, 10.0), (32, 40.0), (32, 200.0)):
        x = torch.randn(64, 8, generator=gen).to(dtype)
        W, b = (torch.randn(N, 8, generator=gen) * gap / 4).to(dtype), torch.randn(N, generator=gen).to(dtype)
        taus, hats, ev, logp, H = FQ.fractions(x, W, b)
        assert taus.shape == (64, N + 1) and (taus[:, 0] == 0).all() and (taus[:, -1] == 1).all() and (taus[:, 1:] >= taus[:, :-1]).all()
        assert torch.equal(ev, torch.cat([taus[:, 1:-1], hats], dim=1)) and torch.equal(hats, 0.5 * (taus[:, :-1] + taus[:, 1:]))
        assert torch.isfinite(logp).all() and torch.isfinite(H).all() and (H >= -1e-6).all() and (H <= torch.log(torch.tensor(float(N))) + 1e-5).all()
        want = torch.softmax((x.double() @ W.double().T + b.double()), dim=1)
        assert (taus[:, 1:].double() - want.cumsum(1)).abs().max().item() <= (1e-14 if dtype is f64 else 1e-5)
    q = FQ.weighted_q(torch.ones(64, 3, 32, dtype=dtype), taus)
    assert (q - 1).abs().max().item() <= (1e-14 if dtype is f64 else 1e-5)                # the intervals add up to 1
