"""CPU-only checks of the ground-truth-state encoder (ocr=gt): the Python surface against the reference's fixture (tests/golden/gt.npz,
made by tests/golden/make_golden_gt.py from the reference's GT_Module), the fp64 restatement of its arithmetic against the fixture layer
by layer, the state observation's restatement on hand-made rows, the C ABI's refusals, and the RL entry point up to the GPU.

The arithmetic bound: a fp32 Linear output is a length-K dot product plus a bias, so it differs from the exact value by at most
(K + 2) 2^-24 (|W| |x| + |b|) elementwise (K - 1 additions, K products, the bias addition, first order; a ReLU does not increase a
difference).  Each layer is fed the fixture's own previous activation, so nothing accumulates."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import train_sb3
from ocrl_amd import _lib, envs, ocrs
from ocrl_amd.utils.config import compose
from tests import gt_ref as G
from tests.golden import make_golden_gt as MK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
BASE = ["ocr=gt", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "num_envs=4", "device=cuda:0", "env=target-N4C4S3S1"]
F = np.float32


@pytest.fixture(scope="module")
def fx():
    return np.load(MK.FIXTURE)


@pytest.fixture(scope="module")
def inventory(fx):
    return json.loads(str(fx["inventory"]))


# ---------------------------------------------------------------------------------------------------------------- 1. surface
def test_exports_and_config_compose():
    assert "GT" in ocrs.__all__ and "GT_Module" in ocrs.__all__ and issubclass(ocrs.GT, ocrs.Base)
    c = compose(CFG, "train_sb3", BASE)
    assert c.ocr.to_dict() == {"name": "GT", "dims": [], "acts": []}
    ocr = ocrs.GT(c.ocr, c.env)
    assert (ocr.name, ocr.num_slots, ocr.rep_dim) == ("GT", 5, 5) and not hasattr(ocr, "_opt")
    assert list(ocr._module.parameters()) == [] and ocr._module.trains_through_autograd is True
    x = torch.arange(50.0).reshape(2, 5, 5)
    assert ocr(x) is x and ocr.get_loss(x) == {} and ocr.get_samples(x) == {}
    metrics, rep = ocr.get_loss(x, with_rep=True)
    assert metrics == {} and rep is x
    assert ocr.save() == {"ocr_module_state_dict": {}}
    c = compose(CFG, "train_sb3", BASE + ["ocr.dims=[8,12]", "ocr.acts=[relu,relu]"])
    assert ocrs.GT(c.ocr, c.env).rep_dim == 12


@pytest.mark.parametrize("tag", list(MK.CASES))
def test_attributes_and_state_dict_keys_are_the_references(inventory, tag):
    inv = inventory[tag]
    m = ocrs.GT_Module(*MK.configs(tag))
    assert (m.num_slots, m.rep_dim) == (inv["num_slots"], inv["rep_dim"])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == inv["params"]
    assert isinstance(m._net, nn.Sequential) and len(m._net) == len(inv["members"])
    for mod, name in zip(m._net, inv["members"]):             # a Linear where the reference has one, a placeholder in each ReLU's slot
        assert isinstance(mod, nn.Linear) if name == "Linear" else isinstance(mod, nn.Identity)


def test_index_gaps_and_the_shorter_list(inventory):
    assert [k for k, _ in inventory["wide"]["params"]] == ["_net.0.weight", "_net.0.bias", "_net.2.weight", "_net.2.bias", "_net.4.weight", "_net.4.bias"]
    assert inventory["wide"]["members"] == ["Linear", "ReLU", "Linear", "ReLU", "Linear"]          # act "none": no slot after the last Linear
    assert inventory["wide_push"]["num_slots"] == 3 + 2 and inventory["wide"]["num_slots"] == 4 + 1
    short = inventory["short_acts"]                            # dims [8, 12, 16], acts [none, relu]: two layers, rep_dim still dims[-1]
    assert [k for k, _ in short["params"]] == ["_net.0.weight", "_net.0.bias", "_net.1.weight", "_net.1.bias"] and short["rep_dim"] == 16
    m = ocrs.GT_Module(*MK.configs("short_acts"))
    assert m._acts == ("none", "relu") and len(m._param_list()) == 4
    m.load_state_dict({k: torch.from_numpy(np.load(MK.FIXTURE)[f"short_acts:w:{k}"]) for k, _ in short["params"]})


# ---------------------------------------------------------------------------------------------------------------- 2. arithmetic
@pytest.mark.parametrize("tag", [t for t in MK.CASES if MK.CASES[t][0]])
def test_restatement_against_the_fixture_layer_by_layer(fx, inventory, tag):
    dims, acts = MK.CASES[tag][:2]
    n = min(len(dims), len(acts))
    keys = [k for k, _ in inventory[tag]["params"]]
    members = inventory[tag]["members"]
    x, member = fx[f"{tag}:state"], 0
    assert np.array_equal(x, MK.state(tag, inventory[tag]["num_slots"]).numpy())
    for l in range(n):
        W, b = fx[f"{tag}:w:{keys[2 * l]}"], fx[f"{tag}:w:{keys[2 * l + 1]}"]
        member += 1 + (acts[l] == "relu")                       # the layer's last member: the ReLU where there is one
        assert members[member - 1] == ("ReLU" if acts[l] == "relu" else "Linear")
        y = fx[f"{tag}:member:{member - 1}"]
        hs, _ = G.gt_mlp(x, [W, b], [acts[l]])
        K = W.shape[1]
        bound = (K + 2) * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b))
        assert (np.abs(y - hs[0]) <= bound).all(), f"{tag} layer {l}: {np.abs(y - hs[0]).max():.3e}"
        x = y
    assert np.array_equal(x, fx[f"{tag}:out"])


def test_gradient_formulas_against_the_fixture(fx, inventory):
    """the fp64 gradients by formula against the reference's fp32 autograd ones: 1e-5 of each tensor's largest entry is two orders
    above fp32 accumulation over these 15 rows and three orders below a wrong term"""
    tag = "wide"
    keys = [k for k, _ in inventory[tag]["params"]]
    params = [fx[f"{tag}:w:{k}"] for k in keys]
    x = fx[f"{tag}:state"]
    dx, gs = G.gt_mlp_grads(x, params, MK.CASES[tag][1], MK.cotangent(tag, fx[f"{tag}:out"].shape).numpy())
    for got, ref in [(dx, fx[f"{tag}:dstate"])] + [(g, fx[f"{tag}:g:{k}"]) for g, k in zip(gs, keys)]:
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------------- 3. state_obs
def test_state_obs_on_hand_made_rows():
    rows = np.array([[[1, 2, F(0.15), 0.25, 0.75],             # an object of the first scale
                      [3, 0, F(0.22), 0.5, 0.125],             # ... of the second: index 1
                      [-1, 1, F(0.22), 0.375, 0.625],          # colour -1: ids -1, the position NOT copied
                      [3, 3, F(0.15), 0.5, 0.5],               # the agent row (red circle)
                      [0, 0, 0, 0, 0],                         # lo < hi: the padding stays zero
                      [0, 0, 0, 0, 0]],
                     [[0, 0, F(0.15), 0.0, 0.0],               # blue square at the origin: not an empty row
                      [6, 3, F(0.22), 1.0, 1.0],
                      [2, 1, F(0.3), 0.5, 0.5],                # a scale outside the list: -1 (the Python side refuses such configs)
                      [3, 3, F(0.22), 0.1, 0.9],
                      [0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0]]], dtype=F)
    want = np.array([[[1, 2, 0, 0.25, 0.75], [3, 0, 1, 0.5, 0.125], [-1, -1, -1, 0, 0], [3, 3, 0, 0.5, 0.5], [0] * 5, [0] * 5],
                     [[0, 0, 0, 0, 0], [6, 3, 1, 1, 1], [2, 1, -1, 0.5, 0.5], [3, 3, 1, F(0.1), F(0.9)], [0] * 5, [0] * 5]], dtype=F)
    got = G.state_obs(rows)
    assert got.dtype == F and got.shape == rows.shape and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- 4. C ABI
def test_symbols_and_refusals():
    L = _lib.lib()
    for name in ("ocrl_sprite_state_obs", "ocrl_gt_mlp_ws_floats", "ocrl_gt_mlp_fwd", "ocrl_gt_mlp_bwd"):
        assert hasattr(L, name)
    ints = lambda v: (ctypes.c_int * max(1, len(v)))(*v)
    ws = lambda M, D, dims: L.ocrl_gt_mlp_ws_floats(M, D, len(dims), ints(dims))
    assert ws(15, 5, [64, 64, 128]) > 0
    for D, dims, reason in ((5, [6], "multiple of 4"), (5, [8, 260], "multiple of 4"), (5, [8] * 5, "len\\(dims\\)"), (0, [8], "input width"),
                            (65, [8], "input width")):
        assert ws(15, D, dims) == 0
        assert re.search(reason, L.ocrl_last_error().decode()), L.ocrl_last_error().decode()
    sizes = [ws(M, 5, [64, 64, 128]) for M in list(range(1, 1100)) + [1280, 5000, 100000]]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    # null arguments are refused before any launch (no GPU is touched: the calls return before the stream is used)
    one, acts = ctypes.c_void_p(64), ints([1])
    ptrs = (ctypes.c_void_p * 2)(64, 64)
    assert L.ocrl_gt_mlp_fwd(None, ptrs, one, 5, 5, 1, ints([8]), acts, one, 1 << 20, None) != 0
    assert "null argument" in L.ocrl_last_error().decode()
    assert L.ocrl_gt_mlp_fwd(one, (ctypes.c_void_p * 2)(64, None), one, 5, 5, 1, ints([8]), acts, one, 1 << 20, None) != 0
    assert "null parameter" in L.ocrl_last_error().decode()
    assert L.ocrl_gt_mlp_fwd(one, ptrs, one, 5, 5, 1, ints([8]), acts, one, 8, None) != 0
    assert "workspace too small" in L.ocrl_last_error().decode()
    assert L.ocrl_gt_mlp_bwd(one, None, ptrs, None, ptrs, 5, 5, 1, ints([8]), acts, one, 1 << 20, None) != 0
    assert "null argument" in L.ocrl_last_error().decode()
    assert L.ocrl_gt_mlp_bwd(one, one, ptrs, None, (ctypes.c_void_p * 2)(None, 64), 5, 5, 1, ints([8]), acts, one, 1 << 20, None) != 0
    assert "null parameter or gradient" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_state_obs(None, 1, 5, one, None) != 0 and "null argument" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_state_obs(one, 1, 5, None, None) != 0 and "null argument" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_state_obs(one, 1, 17, one, None) != 0 and "rows <= 16" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_state_obs(one, 0, 5, one, None) != 0


# ---------------------------------------------------------------------------------------------------------------- 5. train_sb3.build
class _Stop(Exception):
    pass


@pytest.mark.parametrize("env,task", [("target-N4C4S3S1", "TargetEnv"), ("odd-one-out-N4C2S2S1", "OddOneOutEnv")])
def test_build_hands_the_environment_state_mode(monkeypatch, env, task):
    seen = []

    def fake(config_env, *a):
        seen.append(config_env.render_mode)
        raise _Stop()                                          # what follows (the policy on the device) needs a GPU

    monkeypatch.setitem(envs._ENVS, task, fake)
    c = compose(CFG, "train_sb3", BASE[:-1] + [f"env={env}"])
    assert c.env.render_mode == "image"
    with pytest.raises(_Stop):
        train_sb3.build(c)
    assert seen == ["state"] and c.env.render_mode == "state"
    seen.clear()
    c = compose(CFG, "train_sb3", ["ocr=slate"] + BASE[1:-1] + [f"env={env}"])    # every other encoder keeps its frames
    with pytest.raises(_Stop):
        train_sb3.build(c)
    assert seen == ["image"]


def test_test_sb3_evaluates_in_state_mode_too(monkeypatch, tmp_path):
    """test_sb3.py builds its environment with train_sb3.build, so ocr=gt reaches it without a line of its own"""
    import test_sb3
    seen = []

    def fake(config_env, *a):
        seen.append(config_env.render_mode)
        raise _Stop()

    monkeypatch.setitem(envs._ENVS, "TargetEnv", fake)
    agent = tmp_path / "agent.pth"
    agent.write_bytes(b"")
    with pytest.raises(_Stop):
        test_sb3.main(BASE + [f"agent_checkpoint.local_file={agent}", "n_eval_episodes=2", f"run_dir={tmp_path / 'run'}"])
    assert seen == ["state"]


# ---------------------------------------------------------------------------------------------------------------- 6. scales
@pytest.mark.parametrize("over,key", [({"env.SCALES": "[0.15,0.3]"}, "SCALES"), ({"env.AGENT": "[red,circle,0.2]"}, "AGENT"),
                                      ({"env.target": "[blue,square,0.3]", "env.SCALES": "[0.15,0.22]"}, "target")])
def test_state_mode_refuses_scales_without_an_index(monkeypatch, over, key):
    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_library)
    c = compose(CFG, "train_sb3", BASE + ["env.render_mode=state"] + [f"{k}={v}" for k, v in over.items()])
    with pytest.raises(ValueError, match=key):
        envs.TargetEnv(c.env, 4)
    assert envs.env_desc(c.env, 4).E == 4                      # the config is sound otherwise: frames can show any scale
