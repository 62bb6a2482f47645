"""CPU checks of the RN, MLP and Identity pooling heads: parameter inventories against the reference fixtures, RN's limits and its
workspace contract (ocrl_pool_rn_ws_floats), Identity on the CPU, and how the RL extractor constructs each head."""
import ctypes
import json
import types

import numpy as np
import pytest
import torch

from ocrl_amd import poolings
from tests.golden.make_golden_pooling_heads import CASES, config, fixture_path, slots

RN_DEFAULT = dict(g_dims=[256, 256, 256, 256], f_dims=[256, 128, 64, 64])


def _inventory(tag):
    return json.loads(str(np.load(fixture_path(tag))["inventory"]))[tag]


def _module(tag):
    head, D, K, _, _, _ = CASES[tag]
    if head == "RN":
        return poolings.RN_Module(D, K, 1, config(tag))
    return getattr(poolings, head + "_Module")(D, K, config(tag))


@pytest.mark.parametrize("tag", list(CASES))
def test_state_dict_and_rep_dim_match_the_reference(tag):
    m = _module(tag)
    inv = _inventory(tag)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == inv["params"]
    assert m.rep_dim == inv["rep_dim"]


def test_rn_limits():
    cfg = types.SimpleNamespace(**RN_DEFAULT)
    with pytest.raises(NotImplementedError):
        poolings.RN_Module(192, 6, 2, cfg)
    with pytest.raises(ValueError):
        poolings.RN_Module(192, 1, 1, cfg)
    m = poolings.RN_Module(192, 6, 1, cfg)
    with pytest.raises(RuntimeError, match="GPU"):          # no CPU fallback
        m(torch.zeros(2, 6, 192))


def _ws(B, K=6, D=192, g=RN_DEFAULT["g_dims"], f=RN_DEFAULT["f_dims"]):
    from ocrl_amd import _lib
    arr = lambda v: (ctypes.c_int * len(v))(*v)
    return _lib.lib().ocrl_pool_rn_ws_floats(B, K, D, len(g), arr(g), len(f), arr(f))


def test_rn_workspace_contract():
    a, b = _ws(16), _ws(256)
    assert 0 < a < b < _ws(2048)
    assert _ws(16, D=67) > 0                                 # any rep_dim: padded inside the workspace
    assert _ws(16, K=1) == 0 and _ws(16, K=0) == 0
    assert _ws(0) == 0
    assert _ws(16, g=[256, 254]) == 0 and _ws(16, f=[64, 30]) == 0
    assert _ws(16, g=[]) == 0 and _ws(16, f=[]) == 0
    assert _ws(1, K=4096, D=67) == 0                         # SLATE use_cnn_feat at 64x64: 16.8 M pairs per image
    from ocrl_amd import _lib
    assert b"int32" in _lib.lib().ocrl_last_error()


def test_identity_on_cpu_is_flatten():
    s = slots("identity")
    m = poolings.Identity_Module(192, 6, types.SimpleNamespace(name="Identity"))
    assert m.rep_dim == 1152 and list(m.parameters()) == []
    assert torch.equal(m(s), s.flatten(1))
    fx = np.load(fixture_path("identity"))
    assert np.array_equal(m(s).numpy(), fx["identity:out"])
    assert torch.equal(m(s.flatten(1)), s.flatten(1))


def test_extractor_builds_rn_with_its_own_argument_order():
    from ocrl_amd.sb3s.ocr_extractor import make_pooling_module
    cfg = types.SimpleNamespace(pooling=types.SimpleNamespace(name="RN", **RN_DEFAULT), env=types.SimpleNamespace(num_stacked_obss=1))
    m = make_pooling_module(cfg, 192, 6)
    assert isinstance(m, poolings.RN_Module) and m.rep_dim == 64
    assert m._g[0].in_features == 384
    cfg.env.num_stacked_obss = 2                             # reaches RN_Module's num_stacked_obss argument, not its config
    with pytest.raises(NotImplementedError):
        make_pooling_module(cfg, 192, 6)
    del cfg.env                                              # no env section: one observation
    assert make_pooling_module(cfg, 192, 6).rep_dim == 64


@pytest.mark.parametrize("name,over", [("MLP", dict(dims=[128, 128], acts=["relu", "relu"])), ("Identity", dict()),
                                       ("Transformer", dict(d_model=128, nhead=8, num_layers=1, pos_emb="None"))])
def test_extractor_builds_other_heads_as_the_reference(name, over):
    from ocrl_amd.sb3s.ocr_extractor import make_pooling_module
    pc = types.SimpleNamespace(name=name, **over)
    torch.manual_seed(3)
    m = make_pooling_module(types.SimpleNamespace(pooling=pc, env=types.SimpleNamespace(num_stacked_obss=1)), 192, 6)
    torch.manual_seed(3)
    ref = getattr(poolings, name + "_Module")(192, 6, pc)
    assert type(m) is type(ref) and m.rep_dim == ref.rep_dim
    a, b = m.state_dict(), ref.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
