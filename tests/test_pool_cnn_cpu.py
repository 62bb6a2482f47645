"""CPU checks of the NatureCNN pooling heads CNN_Linear and CNN_Transformer: the names, the parameter inventories against the
reference-made fixture, the restatement of tests/pool_cnn_ref.py against that fixture (fp32 and fp64), the C entry points and their
workspace contract, how the RL extractor constructs each head, and the two config files."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import pool_cnn_ref as R
from tests.golden import make_golden_pooling_cnn as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inventory(tag):
    return json.loads(str(np.load(G.FIXTURE)["inventory"]))[tag]


def _module(tag):
    from ocrl_amd import poolings
    head, S, D, _, _ = G.CASES[tag]
    return getattr(poolings, head + "_Module")(D, S * S, G.config(tag))


def test_names_import():
    from ocrl_amd import poolings
    for n in ("CNN_Linear", "CNN_Linear_Module", "CNN_Transformer", "CNN_Transformer_Module"):
        assert n in poolings.__all__ and hasattr(poolings, n)
    assert issubclass(poolings.CNN_Linear, poolings.Base) and issubclass(poolings.CNN_Transformer, poolings.Base)


@pytest.mark.parametrize("tag", list(G.CASES))
def test_state_dict_and_rep_dim_match_the_reference(tag):
    m = _module(tag)
    inv = _inventory(tag)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == inv["params"]
    assert m.rep_dim == inv["rep_dim"]


def test_stacked_observations_widen_cnn_linear_only():
    from ocrl_amd import poolings
    m = poolings.CNN_Linear_Module(67, 4096, G.config("linear64"), num_stacked_obss=2)
    assert tuple(m._net._net[0].weight.shape) == (32, 134, 8, 8) and tuple(m._net._net[7].weight.shape) == (512, 1024)
    m = poolings.CNN_Transformer_Module(67, 4096, G.config("trans64"), num_stacked_obss=2)
    assert tuple(m._cnn._net[0].weight.shape) == (32, 67, 8, 8) and tuple(m._trans._pos.pe.shape) == (4097, 1, 128)
    none = types.SimpleNamespace(**{**G.CASES["trans64"][4], "pos_emb": "None"})
    assert "_trans._pos.pe" not in poolings.CNN_Transformer_Module(67, 4096, none).state_dict()


@pytest.mark.parametrize("tag", list(G.CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_restatement_reproduces_the_reference_fixture(tag, dtype):
    fx = np.load(G.FIXTURE)
    head = G.CASES[tag][0]
    m = _module(tag)
    P = G.weights(m, tag)
    x = G.tokens(tag)
    cot = G.cotangent(tag, fx[tag + ":out"].shape)
    out, g, dt = R.loss_and_grads(P, x, head, G.config(tag), cot, dtype=dtype)
    linear = head == "CNN_Linear"
    tol_out, tol_g = (1e-5, 5e-5) if linear else (2e-5, 3e-4)
    want = fx[tag + ":out"]
    assert np.abs(out.numpy() - want).max() <= tol_out * np.abs(want).max()
    keys = [k for k in fx.files if k.startswith(tag + ":g:")]
    assert sorted(k.split(":g:")[1] for k in keys) == sorted(g)
    gmax = max(np.abs(fx[k] if fx[k].ndim > 1 or fx[k].shape == tuple(g[k.split(":g:")[1]].shape) else fx[k][3:]).max() for k in keys)
    for k in keys + [tag + ":dtokens"]:
        t = dt if k.endswith(":dtokens") else g[k.split(":g:")[1]]
        w = fx[k]
        if w.shape == tuple(t.shape):
            got = t.numpy()
        else:
            got, w = G.sample(t)[3:], w[3:]
        floor = 0.0 if linear or k.endswith(":dtokens") else 1e-3 * gmax      # the floors of tests/test_gpu_pooling_long.py's fixture check
        assert np.abs(got - w).max() <= tol_g * max(np.abs(w).max(), floor), k


def test_c_entry_points_and_workspace_contract():
    from ocrl_amd import _lib
    L = _lib.lib()
    for n in ("ocrl_pool_cnn_ws_floats", "ocrl_pool_cnn_fwd", "ocrl_pool_cnn_bwd"):
        assert hasattr(L, n)
    for D in (1, 3, 64, 67, 134):
        for S in (36, 38, 64, 84, 128):
            for B in (1, 4, 32, 33, 256):
                for rep in (0, 512):
                    assert L.ocrl_pool_cnn_ws_floats(B, S, S, D, rep) > 0, (B, S, D, rep)
    assert L.ocrl_pool_cnn_ws_floats(4, 64, 84, 67, 0) > 0
    for args, msg in [((0, 64, 64, 67, 512), "batch >= 1"), ((2, 64, 64, 0, 512), "token width >= 1"), ((2, 35, 64, 67, 0), "at least 36 x 36"),
                      ((2, 64, 35, 67, 0), "at least 36 x 36"), ((2, 64, 64, 67, 6), "multiple of 4"), ((2, 64, 64, 67, -4), "multiple of 4"),
                      ((40000, 128, 128, 67, 0), "int32"), ((1 << 20, 36, 36, 1, 0), "int32")]:
        assert L.ocrl_pool_cnn_ws_floats(*args) == 0, args
        assert msg in L.ocrl_last_error().decode(), (args, L.ocrl_last_error().decode())


def test_modules_reject_what_they_cannot_run():
    m = _module("linear64")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 4096, 67))
    with pytest.raises(ValueError, match="square"):
        m(torch.zeros(2, 4000, 67))
    with pytest.raises(ValueError, match="1024"):
        m(torch.zeros(2, 84 * 84, 67))
    with pytest.raises(ValueError, match="expected tokens"):
        m(torch.zeros(2, 4096, 3))
    with pytest.raises(ValueError, match="unknown pos_emb"):
        from ocrl_amd import poolings
        poolings.CNN_Transformer_Module(67, 4096, types.SimpleNamespace(**{**G.CASES["trans64"][4], "pos_emb": "rope"}))


@pytest.mark.parametrize("head,rep", [("CNN_Linear", 512), ("CNN_Transformer", 128)])
def test_extractor_builds_the_heads_as_the_reference_does(head, rep):
    from ocrl_amd.sb3s.ocr_extractor import make_pooling_module
    tag = "linear64" if head == "CNN_Linear" else "trans64"
    cfg = types.SimpleNamespace(pooling=G.config(tag), env=types.SimpleNamespace(obs_size=64, obs_channels=3))
    m = make_pooling_module(cfg, 67, 4096)
    assert type(m).__name__ == head + "_Module" and m.rep_dim == rep
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == _inventory(tag)["params"]


def test_config_files_compose_to_the_reference_keys():
    from ocrl_amd.utils.config import Config, _compose_file
    base = dict(learn_aux_loss=False, learn_downstream_loss=False)
    want = {"cnn_linear": dict(name="CNN_Linear", rep_dim=512, **base),
            "cnn_transformer": dict(name="CNN_Transformer", d_model=128, rep_dim=128, nhead=8, num_layers=1, pos_emb="ape", **base)}
    for f, kv in want.items():
        p = Config(_compose_file(os.path.join(ROOT, "configs"), "pooling/" + f, {}, False))
        for k, v in kv.items():
            assert getattr(p, k) == v, (f, k)
        assert p.learning.lr == pytest.approx(1e-4)
        assert set(p.ocr_checkpoint.keys()) == {"entity", "project", "run_id", "file", "local_file", "finetuning"}
        assert set(p.keys()) == set(kv) | {"ocr_checkpoint", "learning"}
        assert getattr(__import__("ocrl_amd.poolings", fromlist=["x"]), p.name + "_Module")(67, 4096, p).rep_dim == kv["rep_dim" if f == "cnn_linear" else "d_model"]
