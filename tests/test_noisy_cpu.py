"""What DQN's noisy linear layers promise without a GPU: the sixth header (include/ocrl_hip_noisy.h) parses, binds and is exported while the
five older tables stay as they were; the layout of `factors`; every rejection its entry points make before a launch; the Makefile's parts;
the rainbow config; NoisyLinear's parameters; and that a policy built without the new arguments keeps its state_dict keys."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import gpu_util as G
from tests import noisy_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
# the header declares five entry points (its prototypes are the issue's, word for word) and one struct
FUNCTIONS = {"ocrl_noisy_desc_size": 0, "ocrl_noisy_factor_floats": 1, "ocrl_noisy_factors": 6, "ocrl_noisy_perturb": 6, "ocrl_noisy_grad": 5}
C51_FUNCTIONS = {"ocrl_c51_desc_size", "ocrl_c51_ws_floats", "ocrl_c51_fwd", "ocrl_c51_bwd", "ocrl_c51_act", "ocrl_c51_td_fwd_bwd"}
DQN_FUNCTIONS = {"ocrl_qnet_desc_size", "ocrl_qnet_ws_floats", "ocrl_qnet_fwd", "ocrl_qnet_bwd", "ocrl_dqn_act", "ocrl_dqn_act_uniforms",
                 "ocrl_dqn_td_fwd_bwd", "ocrl_replay_gather", "ocrl_replay_sample"}
REPLAY_FUNCTIONS = {"ocrl_replay_sample_nstep", "ocrl_replay_gather_nstep", "ocrl_dqn_td_fwd_bwd_ext", "ocrl_per_bytes", "ocrl_per_init",
                    "ocrl_per_set_range", "ocrl_per_update", "ocrl_per_sample"}
NEW_KWARGS = dict(noisy=False, noisy_sigma0=0.5)
CASE_A = [(6, 8), (8, 4), (4, 15), (4, 5)]


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_noisy.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {} and set(abi.structs) == {"ocrl_noisy_desc"}
    assert [f[0] for f in abi.structs["ocrl_noisy_desc"]._fields_] == ["n_layers", "in", "out"]
    assert [t for _, t in abi.structs["ocrl_noisy_desc"]._fields_] == [ctypes.c_int, ctypes.c_int * 10, ctypes.c_int * 10]
    assert set(_lib.ABI_NOISY.functions) == set(FUNCTIONS)
    L = _lib.lib()
    for name, n in FUNCTIONS.items():
        assert len(getattr(L, name).argtypes) == n, name
    assert L.ocrl_noisy_factor_floats.restype is ctypes.c_size_t and L.ocrl_noisy_desc_size.restype is ctypes.c_size_t
    assert L.ocrl_noisy_factors.argtypes[1] is ctypes.c_ulonglong and L.ocrl_noisy_factors.argtypes[2] is ctypes.c_ulonglong
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_NOISY_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                      # self-contained
    # the five older tables are what they were
    assert len(_lib.ABI.functions) == 146 and _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    assert set(_lib.ABI_DQN.functions) == DQN_FUNCTIONS and set(_lib.ABI_ROLLOUT.functions) == {"ocrl_task_scenes_rollout_batch"}
    assert set(_lib.ABI_REPLAY.functions) == REPLAY_FUNCTIONS and set(_lib.ABI_C51.functions) == C51_FUNCTIONS
    older = set(_lib.ABI.functions) | DQN_FUNCTIONS | REPLAY_FUNCTIONS | C51_FUNCTIONS | set(_lib.ABI_ROLLOUT.functions)
    assert not set(FUNCTIONS) & older


def test_the_makefile_names_the_new_parts():
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    for part in ("noisy.hip", "noisy_unit.o", "noisy.h", "ocrl_hip_noisy.h"):
        assert part in makefile, part
    assert re.search(r"^(?:\S+ )*noisy\.o(?: \S+)*: CXXFLAGS \+= -ffp-contract=off$", makefile, re.M)
    assert "SITE_NOISY 440u" in open(os.path.join(ROOT, "ocrl_amd", "csrc", "noisy.h")).read()


def test_descriptor_size_is_the_ctypes_struct():
    assert _lib.lib().ocrl_noisy_desc_size() == ctypes.sizeof(_lib.NoisyDesc) == 21 * 4
    d = _lib.noisy_desc(CASE_A)
    assert (d.n_layers, list(getattr(d, "in"))[:5], list(d.out)[:5]) == (4, [6, 8, 4, 4, 0], [8, 4, 15, 5, 0])
    with pytest.raises(ValueError, match="1 .. 10 noisy layers"):
        _lib.noisy_desc([(4, 4)] * 11)
    with pytest.raises(ValueError, match="1 .. 10 noisy layers"):
        _lib.noisy_desc([])


def test_factor_floats_is_the_stated_layout():
    L = _lib.lib()
    # by hand: f_in then f_out per layer, each block rounded up to a multiple of 4 floats
    assert L.ocrl_noisy_factor_floats(ctypes.byref(_lib.noisy_desc(CASE_A))) == (8 + 8) + (8 + 4) + (4 + 16) + (4 + 8) == 60
    assert N.layout(CASE_A) == ([(0, 8), (16, 24), (28, 32), (48, 52)], 60)
    for layers in ([(1, 1)], [(130, 36), (36, 15)], [(4, 4)] * 10, [(65536, 65536)], [(5, 1), (1, 7)]):
        assert L.ocrl_noisy_factor_floats(ctypes.byref(_lib.noisy_desc(layers))) == N.layout(layers)[1], layers
    assert N.layout([(1, 1)])[1] == 8 and N.layout([(130, 36), (36, 15)])[1] == 132 + 36 + 36 + 16


# ---- rejections before any launch
def test_arguments_are_checked_before_any_launch():
    L, p = _lib.lib(), ctypes.c_void_p(FAKE)
    good = _lib.noisy_desc(CASE_A)
    w = (ctypes.c_void_p * 8)(*[FAKE] * 8)
    hole = (ctypes.c_void_p * 8)(FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE)
    odd = (ctypes.c_void_p * 8)(FAKE, FAKE, FAKE + 4, FAKE, FAKE, FAKE, FAKE, FAKE)

    def factors(d=good, out=p):
        return L.ocrl_noisy_factors(ctypes.byref(d) if d is not None else None, 0, 0, None, out, None)

    def perturb(d=good, mu=w, sigma=w, fac=p, out=w):
        return L.ocrl_noisy_perturb(ctypes.byref(d), mu, sigma, fac, out, None)

    def grad(d=good, dw=w, fac=p, out=w):
        return L.ocrl_noisy_grad(ctypes.byref(d), dw, fac, out, None)

    def desc(n=1, i=4, o=4):
        d = _lib.noisy_desc([(4, 4)] * min(max(n, 1), 10))
        d.n_layers = n
        getattr(d, "in")[0], d.out[0] = i, o
        return d

    limits = ((desc(n=0), "1 <= n_layers <= 10"), (desc(n=11), "1 <= n_layers <= 10"), (desc(n=-1), "1 <= n_layers <= 10"),
              (desc(i=0), "1 <= in, out <= 65536"), (desc(o=0), "1 <= in, out <= 65536"), (desc(i=65537), "1 <= in, out <= 65536"),
              (desc(o=65537), "1 <= in, out <= 65536"), (desc(n=3, o=-2), "1 <= in, out <= 65536"))
    for bad, msg in limits:
        for call in (factors, perturb, grad):
            assert call(d=bad) != 0 and msg in last_error(), (msg, last_error())
        assert L.ocrl_noisy_factor_floats(ctypes.byref(bad)) == 0 and msg in last_error()
    late = _lib.noisy_desc([(4, 4), (4, 4), (4, 70000)])                    # a limit broken in a later layer names the layer
    assert perturb(d=late) != 0 and "layer 2 has in 4, out 70000" in last_error()
    assert L.ocrl_noisy_factor_floats(None) == 0 and "ocrl_noisy_factor_floats: null descriptor" in last_error()
    for call, msg in ((lambda: factors(d=None), "ocrl_noisy_factors: null descriptor"),
                      (lambda: factors(out=None), "ocrl_noisy_factors: null argument"),
                      (lambda: perturb(mu=None), "ocrl_noisy_perturb: null argument"),
                      (lambda: perturb(sigma=None), "ocrl_noisy_perturb: null argument"),
                      (lambda: perturb(fac=None), "ocrl_noisy_perturb: null argument"),
                      (lambda: perturb(out=None), "ocrl_noisy_perturb: null argument"),
                      (lambda: perturb(mu=hole), "ocrl_noisy_perturb: parameter pointer 5 of 8 is null"),
                      (lambda: perturb(sigma=hole), "parameter pointer 5 of 8 is null"),
                      (lambda: perturb(out=hole), "parameter pointer 5 of 8 is null"),
                      (lambda: perturb(mu=odd), "parameter pointer 2 of 8 is not 16-byte aligned"),
                      (lambda: perturb(fac=ctypes.c_void_p(FAKE + 8)), "factors must be 16-byte aligned"),
                      (lambda: grad(dw=None), "ocrl_noisy_grad: null argument"),
                      (lambda: grad(fac=None), "ocrl_noisy_grad: null argument"),
                      (lambda: grad(out=None), "ocrl_noisy_grad: null argument"),
                      (lambda: grad(dw=hole), "ocrl_noisy_grad: parameter pointer 5 of 8 is null"),
                      (lambda: grad(out=hole), "parameter pointer 5 of 8 is null"),
                      (lambda: grad(out=odd), "parameter pointer 2 of 8 is not 16-byte aligned")):
        assert call() != 0 and msg in last_error(), (msg, last_error())
    # a shorter descriptor reads a shorter list: the hole at 5 is past the end of two layers' four pointers
    two = _lib.noisy_desc(CASE_A[:2])
    four = (ctypes.c_void_p * 4)(FAKE, FAKE, FAKE, None)
    assert perturb(d=two, mu=four) != 0 and "parameter pointer 3 of 4 is null" in last_error()


# ---- the restatement's own arithmetic
def test_the_restatement_draws_what_the_header_states():
    # draw 0: the word of gpu_util.rng_bits4 itself at the counter (l << 28) | (s << 27) | i
    x, y = N.bits(7, 0, 3, 1, 5)
    wx, wy = G.rng_bits4(7, 440, (3 << 28) | (1 << 27) | np.arange(5, dtype=np.uint64))
    assert (x == wx).all() and (y == wy).all()
    # another draw enters the key's high word: other words, and 2^32 draws later the same again
    x1, _ = N.bits(7, 1, 3, 1, 5)
    x2, _ = N.bits(7, 1 + 2 ** 32, 3, 1, 5)
    assert (x1 != x).any() and (x1 == x2).all()
    # u01_24 rounds its sum to fp32: the largest 24 bits give exactly 1, whose Gaussian is 0
    assert N.u01_24(np.array([0xFFFFFFFF], dtype=np.uint64))[0] == 1.0 and N.u01_24(np.array([0], dtype=np.uint64))[0] == 0.5 / 2 ** 24
    assert N.f_of([-4.0, 0.0, 9.0]).tolist() == [-2.0, 0.0, 3.0]
    g = np.concatenate([N.gaussians(3, t, 0, 0, 4096) for t in range(4)])
    assert abs(g.mean()) < 5 / math.sqrt(g.size) and abs((g * g).mean() - 1) < 5 * math.sqrt(2 / g.size)
    fac = N.factors(CASE_A, 3, 2)
    offs, n = N.layout(CASE_A)
    assert fac.shape == (n,) and (fac[6:8] == 0).all() and (fac[47:48] == 0).all() and fac[46] != 0 and (fac[57:60] == 0).all() and (fac[:6] != 0).all()
    # perturb / grad on a case small enough to follow: one layer, in 2, out 1
    mu, sg = [torch.tensor([[1.0, 2.0]]), torch.tensor([3.0])], [torch.tensor([[0.5, -1.0]]), torch.tensor([2.0])]
    f = torch.tensor([2.0, -3.0, 0, 0, 0.5, 0, 0, 0])
    w, b = N.perturb([(2, 1)], mu, sg, f)
    assert w.tolist() == [[1.0 + 0.5 * 1.0, 2.0 - 1.0 * -1.5]] and b.tolist() == [3.0 + 2.0 * 0.5]
    dw, db = N.grad([(2, 1)], [torch.tensor([[4.0, 8.0]]), torch.tensor([-2.0])], f)
    assert dw.tolist() == [[4.0, -12.0]] and db.tolist() == [-1.0]


# ---- config and the algorithm's arguments
def test_rainbow_config_composes_and_its_kwargs_are_dqns():
    from ocrl_amd import sb3s
    c51, rainbow = compose(os.path.join(CFG, "sb3"), "dqn_c51").to_dict(), compose(os.path.join(CFG, "sb3"), "rainbow").to_dict()
    assert rainbow["name"] == "DQN"
    assert rainbow["algo_kwargs"] == dict(c51["algo_kwargs"], noisy=True, noisy_sigma0=0.5)
    assert rainbow["algo_kwargs"]["noisy"] is True
    params = inspect.signature(sb3s.DQN.__init__).parameters
    assert set(rainbow["algo_kwargs"]) <= set(params) and {k: params[k].default for k in NEW_KWARGS} == NEW_KWARGS
    assert {"noisy", "noisy_sigma0"} <= set(sb3s.DQN.HYPER)
    for cls in (sb3s.DQNPolicy, sb3s.QNetwork, sb3s.CategoricalQNetwork):
        pp = inspect.signature(cls.__init__).parameters
        assert {k: pp[k].default for k in NEW_KWARGS} == NEW_KWARGS, cls
    full = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", "sb3=rainbow", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4"])
    assert full.sb3.to_dict() == rainbow
    assert open(os.path.join(CFG, "sb3", "rainbow.yaml")).read().startswith("# Rainbow")
    assert "NoisyLinear" in sb3s.__all__ and issubclass(sb3s.NoisyLinear, torch.nn.Linear)
    assert "rainbow" in __import__("train_sb3").__doc__


@pytest.mark.parametrize("fin, fout, sigma0", [(6, 8, 0.5), (64, 204, 0.5), (1, 1, 0.25), (130, 36, 1.0)])
def test_noisy_linear_parameters(fin, fout, sigma0):
    from ocrl_amd.sb3s import NoisyLinear
    torch.manual_seed(5)
    m = NoisyLinear(fin, fout, sigma0)
    assert [k for k, _ in m.named_parameters()] == ["weight", "bias", "weight_sigma", "bias_sigma"] == list(m.state_dict())
    assert [tuple(p.shape) for p in m.parameters()] == [(fout, fin), (fout,), (fout, fin), (fout,)]
    assert all(p.requires_grad and p.dtype == torch.float32 for p in m.parameters())
    s = torch.tensor(sigma0 / math.sqrt(fin), dtype=torch.float32)
    assert (m.weight_sigma == s).all() and (m.bias_sigma == s).all()
    bound = 1 / math.sqrt(fin)
    assert m.weight.abs().max().item() <= bound and m.bias.abs().max().item() <= bound
    # nn.Linear's own initialisation, draw for draw
    torch.manual_seed(5)
    plain = torch.nn.Linear(fin, fout)
    assert torch.equal(plain.weight, m.weight) and torch.equal(plain.bias, m.bias)
    if fin * fout >= 48:
        assert m.weight.abs().max().item() > 0.8 * bound                               # U(+-1/sqrt(in)) fills its range


def _env(n=4):
    return types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=n))


def test_a_policy_without_the_new_arguments_keeps_its_keys():
    from ocrl_amd.sb3s import DQN, DQNPolicy, NoisyLinear
    env = _env()
    plain = DQNPolicy(env.observation_space, env.action_space, noisy=False)
    assert list(plain.state_dict()) == ["q_net.q_net.0.weight", "q_net.q_net.0.bias", "q_net.q_net.2.weight", "q_net.q_net.2.bias",
                                        "q_net.q_net.4.weight", "q_net.q_net.4.bias"]
    cat = DQNPolicy(env.observation_space, env.action_space, n_atoms=11, v_min=-1.0, v_max=1.0, dueling=True, net_arch=(8,), noisy=False)
    assert list(cat.state_dict()) == ["q_net.q_net.0.weight", "q_net.q_net.0.bias", "q_net.q_net.2.weight", "q_net.q_net.2.bias",
                                      "q_net.value_net.weight", "q_net.value_net.bias"]
    assert not any(isinstance(m, NoisyLinear) for p in (plain, cat) for m in p.modules()) and not plain.noisy and not cat.noisy
    # the same initialisation as without the arguments, and the mean parameters are the kernels' list themselves
    torch.manual_seed(3)
    a = DQNPolicy(env.observation_space, env.action_space)
    torch.manual_seed(3)
    b = DQNPolicy(env.observation_space, env.action_space, noisy=False, noisy_sigma0=0.5)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert all(x is y for x, y in zip(b.q_net._param_list(), b.q_net.parameters()))
    plain.set_noise(3)                                                                 # nothing to choose: no stream is asked for
    assert plain.q_net._noise is None


def test_a_noisy_policy_holds_noisy_layers_everywhere():
    from ocrl_amd.sb3s import DQN, DQNPolicy, NoisyLinear
    env = _env()
    cat = DQNPolicy(env.observation_space, env.action_space, n_atoms=11, v_min=-1.0, v_max=1.0, dueling=True, net_arch=(8,), noisy=True, noisy_sigma0=0.25)
    keys = [f"q_net.{m}.{p}" for m in ("q_net.0", "q_net.2", "value_net") for p in ("weight", "bias", "weight_sigma", "bias_sigma")]
    assert list(cat.state_dict()) == keys
    lin = [m for m in cat.modules() if isinstance(m, torch.nn.Linear)]
    assert len(lin) == 3 and all(type(m) is NoisyLinear for m in lin)
    assert cat.q_net.value_net.weight_sigma[0, 0].item() == pytest.approx(0.25 / math.sqrt(8))
    scalar = DQNPolicy(env.observation_space, env.action_space, noisy=True)
    assert all(type(m) is NoisyLinear for m in scalar.modules() if isinstance(m, torch.nn.Linear)) and len(list(scalar.parameters())) == 12
    # the mean weights need no stream and no GPU: the kernels' list is the mu parameters themselves
    assert cat.q_net._noise is None
    assert all(x is y for x, y in zip(cat.q_net._param_list(), [p for m in lin for p in (m.weight, m.bias)]))
    with pytest.raises(RuntimeError, match="set_sampling"):
        cat.set_noise(0)
    cat.set_sampling(9)
    cat.set_noise(4)
    assert cat.q_net._noise == (9, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cat.q_net._param_list()
    cat.set_noise(None)
    assert cat.q_net._noise is None
    # the algorithm: epsilon is 0 from the start, the arguments and the policy must agree
    model = DQN(cat, env, device="cpu", n_atoms=11, v_min=-1.0, v_max=1.0, dueling=True, noisy=True, noisy_sigma0=0.25, exploration_initial_eps=1.0)
    assert model.exploration_rate == 0.0 and model.epsilon() == 0.0 and model.noise_draws == 0
    assert model.target._sample_seed == model.policy._sample_seed + 1
    with pytest.raises(ValueError, match="noisy"):
        DQN(cat, env, device="cpu", n_atoms=11, v_min=-1.0, v_max=1.0, dueling=True)
    with pytest.raises(ValueError, match="noisy_sigma0"):
        DQN(DQNPolicy, env, device="cpu", noisy=True, noisy_sigma0=-1.0)
