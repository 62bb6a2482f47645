"""What A2C promises without a GPU: the two new C symbols and every rejection they make before a launch, the a2c config, the package's
exports, train_sb3.build's refusal of an algorithm that is not built, and the restatement of tests/a2c_ref.py against hand-worked numbers
(an RMSprop example and the closed-form cotangents of the loss)."""
import ctypes
import math
import os

import pytest
import torch

from ocrl_amd.utils.config import compose
from tests import a2c_ref as A
from tests import acnet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def test_new_symbols_are_exported_with_the_declared_argument_counts():
    lib, L = _lib()
    assert len(L.ocrl_acnet_a2c_fwd_bwd.argtypes) == 15 and len(L.ocrl_acnet_ppo_fwd_bwd.argtypes) == 17
    assert len(L.ocrl_flat_clip_rmsprop_l2.argtypes) == 12 and len(L.ocrl_flat_clip_rmsprop_ws_floats.argtypes) == 0
    assert L.ocrl_flat_clip_rmsprop_ws_floats() >= 1024 and L.ocrl_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "ocrl_hip.h")).read()
    for name in ("ocrl_acnet_a2c_fwd_bwd", "ocrl_flat_clip_rmsprop_l2", "ocrl_flat_clip_rmsprop_ws_floats"):
        assert hasattr(L, name) and name in header, name
    note = header[header.index("TF-style RMSprop"):header.index("size_t ocrl_flat_clip_rmsprop_ws_floats")]
    assert "INSIDE the square root" in note and "ONES" in note


def _a2c_call(B=4, A=4, norm=0, ws_floats=None, **null):
    """ocrl_acnet_a2c_fwd_bwd on the identity layout with fake pointers; `null` names the arguments passed as NULL"""
    lib, L = _lib()
    d = lib.acnet_desc(B, 8, A, ((), (), ()), ((), (), ()))
    need = L.ocrl_acnet_ws_floats(ctypes.byref(d))
    arr = lambda: (ctypes.c_void_p * 4)(*[FAKE] * 4)
    a = dict(features=FAKE, w=arr(), actions=FAKE, advantages=FAKE, returns=FAKE, scalars=FAKE, dfeatures=FAKE, dw=arr(), ws=FAKE)
    for k in null:
        a[k] = None
    rc = L.ocrl_acnet_a2c_fwd_bwd(ctypes.byref(d), a["features"], a["w"], a["actions"], a["advantages"], a["returns"], 0.5, 0.0, norm, a["scalars"],
                                  a["dfeatures"], a["dw"], a["ws"], need if ws_floats is None else ws_floats, None)
    return rc, L.ocrl_last_error().decode()


def test_a2c_step_rejects_before_any_launch():
    for k in ("features", "w", "actions", "advantages", "returns", "scalars", "dw", "ws"):
        rc, msg = _a2c_call(**{k: True})
        assert rc != 0 and "ocrl_acnet_a2c_fwd_bwd" in msg and "null" in msg, (k, msg)
    rc, msg = _a2c_call(A=0)
    assert rc != 0 and "n_actions" in msg and "heads" in msg
    rc, msg = _a2c_call(B=1, norm=1)
    assert rc != 0 and "normalize_advantage" in msg
    rc, msg = _a2c_call(ws_floats=3)
    assert rc != 0 and "workspace" in msg
    rc, msg = _a2c_call(A=65)
    assert rc != 0 and "n_actions" in msg
    lib, L = _lib()
    assert L.ocrl_acnet_a2c_fwd_bwd(None, FAKE, None, FAKE, FAKE, FAKE, 0.5, 0.0, 0, FAKE, None, None, FAKE, 0, None) != 0
    assert "descriptor" in L.ocrl_last_error().decode()


def _rms_call(p=FAKE, g=FAKE, sq=FAKE, n=8, alpha=0.99, eps=1e-5, norm=FAKE, ws=FAKE, ws_floats=None):
    lib, L = _lib()
    rc = L.ocrl_flat_clip_rmsprop_l2(p, g, sq, n, 0.5, 7e-4, alpha, eps, norm, ws, L.ocrl_flat_clip_rmsprop_ws_floats() if ws_floats is None else ws_floats,
                                     None)
    return rc, L.ocrl_last_error().decode()


@pytest.mark.parametrize("kw,word", [(dict(p=None), "null"), (dict(g=None), "null"), (dict(sq=None), "null"), (dict(norm=None), "norm_out"),
                                     (dict(ws=None), "ws"), (dict(n=0), "n >= 1"), (dict(n=-4), "n >= 1"), (dict(p=FAKE + 4), "aligned"),
                                     (dict(g=FAKE + 8), "aligned"), (dict(sq=FAKE + 12), "aligned"), (dict(ws_floats=1023), "workspace"),
                                     (dict(alpha=0.0), "alpha"), (dict(alpha=1.0), "alpha"), (dict(alpha=-0.5), "alpha"), (dict(alpha=1.5), "alpha"),
                                     (dict(alpha=math.nan), "alpha"), (dict(eps=0.0), "eps"), (dict(eps=-1e-5), "eps"), (dict(eps=math.nan), "eps")])
def test_rmsprop_step_rejects_before_any_launch(kw, word):
    rc, msg = _rms_call(**kw)
    assert rc != 0 and "ocrl_flat_clip_rmsprop_l2" in msg and word in msg, msg


def test_a2c_config_composes_to_the_reference_values():
    c = compose(os.path.join(CFG, "sb3"), "a2c")
    assert c.to_dict() == {"name": "A2C", "algo_kwargs": {"n_steps": 5, "learning_rate": 7e-4}}
    full = compose(CFG, "train_sb3", ["ocr=slate", "pooling=transformer", "sb3=a2c", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=16"])
    assert full.sb3.to_dict() == c.to_dict()


def test_exports_and_the_refusal_of_other_algorithms():
    from ocrl_amd import sb3s
    assert {"A2C", "a2c_loss", "PPO", "ppo_loss"} <= set(sb3s.__all__)
    assert issubclass(sb3s.A2C, sb3s.on_policy.OnPolicyAlgorithm) and issubclass(sb3s.PPO, sb3s.on_policy.OnPolicyAlgorithm)
    for name in ("collect_rollouts", "learn", "predict", "save", "load", "_flatten_parameters"):         # shared, not copied
        assert getattr(sb3s.A2C, name) is getattr(sb3s.PPO, name) is getattr(sb3s.on_policy.OnPolicyAlgorithm, name), name
    import train_sb3
    c = compose(CFG, "train_sb3", ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "env=target-N4C4S3S1", "sb3.name=SAC"])
    with pytest.raises(NotImplementedError, match="SAC is not built") as e:
        train_sb3.build(c)
    assert "PPO" in str(e.value) and "A2C" in str(e.value)


def test_a2c_refuses_what_it_does_not_build():
    import types
    from ocrl_amd.sb3s import A2C, CustomActorCriticPolicy
    env = lambda space: types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=space)
    with pytest.raises(NotImplementedError, match="schedule"):
        A2C(CustomActorCriticPolicy, env(types.SimpleNamespace(n=4)), learning_rate=lambda progress: 7e-4 * progress)
    with pytest.raises(NotImplementedError, match="Discrete action spaces only"):
        A2C(CustomActorCriticPolicy, env(types.SimpleNamespace(shape=(3,), low=-1.0, high=1.0)))


def test_rmsprop_restatement_on_a_hand_worked_example():
    """two steps from sq = 1 on three numbers, lr = 0.1, alpha = 0.99, eps = 1e-5, max_norm = 0.5.
    Step 1: g = (0.3, 0, -0.4), norm 0.5: coef = 0.5 / (0.5 + 1e-6) < 1 only by the 1e-6 (taken as 1 below, within 2e-6);
            sq = 0.99 + 0.01 g^2 = (0.9909, 0.99, 0.9916); p -= 0.1 g / sqrt(sq + 1e-5).
    Step 2: g = (3, 0, -4), norm 5: the clip bites, coef = 0.5 / 5.000001, g' = (0.3, 0, -0.4) (1 - 2e-7);
            sq = 0.99 sq + 0.01 g'^2 = (0.981891, 0.9801, 0.983284)."""
    p0 = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)
    r1 = A.rmsprop_tf_l2(p0, f64(0.3, 0.0, -0.4), torch.ones(3), 0.5, 0.1)
    assert abs(r1.norm.item() - 0.5) < 1e-15 and abs(r1.coef.item() - 0.5 / 0.500001) < 1e-12
    sq1 = [0.9909, 0.99, 0.9916]
    assert torch.allclose(r1.sq, torch.tensor(sq1, dtype=torch.float64), atol=1e-7)
    want1 = [1.0 - 0.1 * 0.3 / math.sqrt(0.9909 + 1e-5), 2.0, 3.0 + 0.1 * 0.4 / math.sqrt(0.9916 + 1e-5)]
    assert torch.allclose(r1.p, torch.tensor(want1, dtype=torch.float64), atol=3e-7)
    r2 = A.rmsprop_tf_l2(r1.p, f64(3.0, 0.0, -4.0), r1.sq, 0.5, 0.1)
    assert abs(r2.norm.item() - 5.0) < 1e-12 and abs(r2.coef.item() - 0.5 / 5.000001) < 1e-15 and r2.coef.item() < 0.11
    sq2 = [0.99 * 0.9909 + 0.01 * 0.09, 0.9801, 0.99 * 0.9916 + 0.01 * 0.16]
    assert torch.allclose(r2.sq, torch.tensor(sq2, dtype=torch.float64), atol=1e-7)
    want2 = [want1[0] - 0.1 * 0.3 / math.sqrt(sq2[0] + 1e-5), 2.0, want1[2] + 0.1 * 0.4 / math.sqrt(sq2[2] + 1e-5)]
    assert torch.allclose(r2.p, torch.tensor(want2, dtype=torch.float64), atol=3e-7)
    # what sets it apart from torch.optim.RMSprop: from sq = 0 and g = 0 the step is 0 / sqrt(eps), finite
    r0 = A.rmsprop_tf_l2(p0, torch.zeros(3), torch.zeros(3), 0.5, 0.1)
    assert torch.equal(r0.p, p0) and torch.isfinite(r0.p).all()
    # without a clip the second step moves ten times as far as the raw gradient is larger
    r3 = A.rmsprop_tf_l2(r1.p, f64(3.0, 0.0, -4.0), r1.sq, 0.0, 0.1)
    assert r3.coef.item() == 1.0 and abs((r3.p[0] - r1.p[0]).item()) > 5 * abs((r2.p[0] - r1.p[0]).item())


@pytest.mark.parametrize("norm", [False, True])
def test_loss_gradient_against_the_closed_form_cotangents(norm):
    """B = 3, A = 2 on the identity layout: autograd's dL/dlogits and dL/dvalues are the closed form the kernel carries into its backward"""
    gen = torch.Generator().manual_seed(5)
    lg = torch.randn(3, 2, generator=gen, dtype=torch.float64).requires_grad_(True)
    vl = torch.randn(3, generator=gen, dtype=torch.float64).requires_grad_(True)
    actions = torch.tensor([1, 0, 5])                                            # the last one is clamped to 1
    adv, ret = torch.tensor([0.7, -1.2, 0.4], dtype=torch.float64), torch.tensor([0.1, 0.5, -0.3], dtype=torch.float64)
    s = A.a2c(lg, vl, actions, adv, ret, 0.5, 0.01, norm)
    dz, dv = torch.autograd.grad(s["loss"], [lg, vl])
    cz, cv = A.cotangents(lg.detach(), vl.detach(), actions, adv, ret, 0.5, 0.01, norm)
    assert (dz - cz).abs().max().item() <= 1e-14 and (dv - cv).abs().max().item() <= 1e-14
    assert abs(s["loss"].item() - (s["policy_loss"] + 0.01 * s["entropy_loss"] + 0.5 * s["value_loss"]).item()) <= 1e-15
    # the policy term by hand for row 0 (action 1): -adv_0 log q_01 / 3 enters the mean
    if not norm:
        logq = torch.log_softmax(lg.detach(), -1)
        by_hand = -(0.7 * logq[0, 1] - 1.2 * logq[1, 0] + 0.4 * logq[2, 1]) / 3
        assert abs(s["policy_loss"].item() - by_hand.item()) <= 1e-15
    # and through the whole restated network: a2c_loss's dw of the action head's bias is the column sum of the cotangents
    x = torch.randn(3, 4, generator=gen)
    ps = [torch.randn(s_, generator=gen) for s_ in R.param_shapes(4, 2, ((), (), ()))]
    scal, dx, dw = A.a2c_loss(x, ps, (((), (), ()), ((), (), ())), actions, adv, ret, 0.5, 0.01, norm)
    _, _, lg2, vl2 = R.forward(x.double(), [p.double() for p in ps], ((), (), ()), ((), (), ()))
    cz2, cv2 = A.cotangents(lg2, vl2, actions, adv, ret, 0.5, 0.01, norm)
    assert (dw[1] - cz2.sum(0)).abs().max().item() <= 1e-14 and abs(dw[3].item() - cv2.sum().item()) <= 1e-14
    assert (dx - (cz2 @ ps[0].double() + cv2[:, None] * ps[2].double())).abs().max().item() <= 1e-14
