"""CPU checks of the actor-critic surface: tests/acnet_ref.py reproduces the reference fixture (fp32 torch against fp32 torch from the
same weights: 1e-6 of each tensor's maximum), ocrl_amd.sb3s.CustomNetwork has the reference's state_dict and latent widths, the YAML
files resolve to the reference's values, the exported symbols exist, and the GAE restatement matches a hand-worked example."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import acnet_ref as R
from tests.golden.make_golden_acnet import CASES, CLIP, ENT_COEF, FIXTURE, VF_COEF, case_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"relu": 1, "tanh": 2}


def _close(got, want, tag):
    want = torch.as_tensor(want)
    e = (got.detach().double() - want.double()).abs().max().item() / max(want.double().abs().max().item(), 1e-30)
    assert e <= 1e-6, (tag, e)


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_reproduces_the_reference_fixture(tag):
    fx = np.load(FIXTURE)
    F, B, A, c = CASES[tag]
    dims = tuple(tuple(c[t]["dims"]) for t in ("shared_net", "policy_net", "value_net"))
    acts = tuple(tuple(c[t]["acts"]) for t in ("shared_net", "policy_net", "value_net"))
    names = [f"w.{k}" for k in fx[f"{tag}.keys"]] + ["action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"]
    w = [torch.from_numpy(fx[f"{tag}.{k}"]).requires_grad_(True) for k in names]
    assert [tuple(p.shape) for p in w] == R.param_shapes(F, A, dims)
    x = torch.from_numpy(fx[f"{tag}.features"]).requires_grad_(True)
    lp, lv, lg, vl = R.forward(x, w, dims, acts)
    for k, got in (("latent_pi", lp), ("latent_vf", lv), ("logits", lg), ("values", vl)):
        _close(got, fx[f"{tag}.{k}"], k)
    t = lambda k: torch.from_numpy(fx[f"{tag}.{k}"])
    s = R.ppo(lg, vl, t("actions"), t("old_log_prob"), t("advantages"), t("returns"), CLIP, VF_COEF, ENT_COEF, True)
    for i, k in enumerate(R.SCALARS):
        assert abs(s[k].item() - fx[f"{tag}.scalars"][i]) <= 1e-6 * max(abs(fx[f"{tag}.scalars"][:5]).max(), 1e-30), k
    assert 0.0 < fx[f"{tag}.scalars"][5] < 1.0
    s["loss"].backward()
    _close(x.grad, fx[f"{tag}.grad.features"], "features")
    for k, p in zip(names, w):
        _close(p.grad, fx[f"{tag}.grad.{k}"], k)


@pytest.mark.parametrize("tag", list(CASES) + ["identity"])
def test_custom_network_has_the_reference_state_dict(tag):
    from ocrl_amd.sb3s import CustomNetwork
    fx = np.load(FIXTURE)
    F = 24 if tag == "identity" else CASES[tag][0]
    net = CustomNetwork(F, case_config(tag))
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in fx[f"{tag}.keys"]]
    assert [net.latent_dim_pi, net.latent_dim_vf] == list(fx[f"{tag}.latent_dims"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(fx[f"{tag}.shape.{k}"])
    if tag == "identity":
        assert len(list(net.parameters())) == 0 and bool(fx["identity.returns_input"].all())
    else:
        net.load_state_dict({k: torch.from_numpy(fx[f"{tag}.w.{k}"]) for k in sd})
        c = CASES[tag][3]
        assert net._layout() == (tuple(tuple(c[t]["dims"]) for t in ("shared_net", "policy_net", "value_net")),
                                 tuple(tuple(CODE[a] for a in c[t]["acts"]) for t in ("shared_net", "policy_net", "value_net")))
        with pytest.raises(RuntimeError):
            net(torch.zeros(2, F))                                  # no CPU fallback


def test_bad_activation_raises():
    from ocrl_amd.sb3s import CustomNetwork
    cfg = case_config("mlp")
    cfg.policy_net.acts = ["gelu"]
    with pytest.raises(ValueError, match="gelu is not implemented"):
        CustomNetwork(16, cfg)


def test_configs_resolve_to_the_reference_values():
    from ocrl_amd.utils.config import compose
    want_mlp = dict(shared_net=dict(dims=[64, 64], acts=["relu", "relu"]), policy_net=dict(dims=[64], acts=["tanh"]),
                    value_net=dict(dims=[64], acts=["tanh"]))
    empty = dict(shared_net=dict(dims=[], acts=[]), policy_net=dict(dims=[], acts=[]), value_net=dict(dims=[], acts=[]))
    for name, label, ortho, nets in (("mlp", "MLP", False, want_mlp), ("mlp_orthoinit", "MLPOrthoInit", True, want_mlp),
                                     ("identity", "Identity", False, empty), ("identity_orthoinit", "IdentityOrthoInit", True, empty)):
        assert compose(os.path.join(ROOT, "configs", "sb3_acnet"), name).to_dict() == dict(name=label, ortho_init=ortho, **nets)
    assert compose(os.path.join(ROOT, "configs", "sb3_acnet"), "_base").to_dict() == dict(ortho_init=False, **empty)
    assert compose(os.path.join(ROOT, "configs", "sb3"), "ppo").to_dict() == dict(
        name="PPO", algo_kwargs=dict(n_steps=2048, batch_size=32, learning_rate=3e-4, ent_coef=0.0, gamma=0.99, vf_coef=0.5, target_kl=None,
                                     clip_range=0.2))


def test_exports_and_the_c_surface():
    import ocrl_amd.sb3s as S
    from ocrl_amd import _lib
    for k in ("OCRExtractor", "CustomNetwork", "CustomActorCriticPolicy", "ppo_loss", "compute_gae"):
        assert k in S.__all__ and hasattr(S, k)
    L = _lib.lib()
    for k in ("ocrl_acnet_ws_floats", "ocrl_acnet_fwd", "ocrl_acnet_bwd", "ocrl_acnet_ppo_fwd_bwd", "ocrl_gae"):
        assert hasattr(L, k)
    assert L.ocrl_abi_version() == 5
    import ctypes
    ok = _lib.acnet_desc(4, 128, 4, ((64, 64), (64,), (64,)), ((1, 1), (2,), (2,)))
    assert L.ocrl_acnet_ws_floats(ctypes.byref(ok)) > 0
    bad = _lib.acnet_desc(4, 128, 4, ((66,), (), ()), ((1,), (), ()))
    assert L.ocrl_acnet_ws_floats(ctypes.byref(bad)) == 0 and b"multiples of 4" in L.ocrl_last_error()


def test_policy_heads_action_spaces_and_ortho_init():
    from ocrl_amd.sb3s import CustomActorCriticPolicy
    fe = lambda: torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 32))

    def build(name, space):
        f = fe()
        f.features_dim = 32
        c = types.SimpleNamespace(sb3_acnet=case_config("mlp"))
        c.sb3_acnet.ortho_init = name.endswith("ortho")
        return CustomActorCriticPolicy(None, space, None, config=c, features_extractor=f)
    pol = build("mlp", types.SimpleNamespace(n=4))
    assert pol.action_net.weight.shape == (4, 64) and pol.value_net.weight.shape == (1, 64) and pol.ortho_init is False
    assert pol.mlp_extractor.latent_dim_pi == 64 and pol.features_dim == 32
    pol = build("mlp_ortho", types.SimpleNamespace(n=np.int64(6)))
    for m, gain in ((pol.features_extractor[1], math.sqrt(2)), (pol.mlp_extractor.shared_net[0], math.sqrt(2)), (pol.action_net, 0.01),
                    (pol.value_net, 1.0)):
        w = m.weight.detach().double()
        g = w @ w.t() if w.shape[0] <= w.shape[1] else w.t() @ w
        assert torch.allclose(g, gain * gain * torch.eye(g.shape[0], dtype=torch.float64), atol=1e-5) and (m.bias == 0).all()
    box = types.SimpleNamespace(low=-1.0, high=1.0, shape=(9,))
    with pytest.raises(NotImplementedError, match="Discrete"):
        build("mlp", box)


def test_gae_restatement_on_a_hand_worked_example():
    """T = 3, one environment, gamma = 0.5, lambda = 0.5, an episode start at t = 2, not done at the end:
    t = 2: delta = 1 + 0.5 * 2 - 1 = 1, A = 1;  t = 1: the next step starts an episode, delta = 2 - 3 = -1, A = -1;
    t = 0: delta = 1 + 0.5 * 3 - 2 = 0.5, A = 0.5 + 0.25 * (-1) = 0.25"""
    rw = torch.tensor([[1.0], [2.0], [1.0]])
    val = torch.tensor([[2.0], [3.0], [1.0]])
    st = torch.tensor([[1.0], [0.0], [1.0]])
    adv, ret = R.gae(rw, val, st, torch.tensor([2.0]), torch.tensor([0.0]), 0.5, 0.5)
    assert adv[:, 0].tolist() == [0.25, -1.0, 1.0] and ret[:, 0].tolist() == [2.25, 2.0, 2.0]
    adv, _ = R.gae(rw, val, st, torch.tensor([2.0]), torch.tensor([1.0]), 0.5, 0.5)      # done at the end: t = 2 loses the bootstrap
    assert adv[:, 0].tolist() == [0.25, -1.0, 0.0]
