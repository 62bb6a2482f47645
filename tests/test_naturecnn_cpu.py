"""CPU checks of the NatureCNN and MultipleCNN encoders: exported names and C symbols, parameter inventories against the reference
fixtures, the workspace contract (ocrl_naturecnn_ws_floats, 0 for rejected shapes), the no-CPU-fallback rule, MultipleCNN leaving the
caller's config alone, and the extractor / pooling gates admitting these encoders."""
import json
import types

import numpy as np
import pytest
import torch

from ocrl_amd import ocrs, poolings
from tests.golden.make_golden_naturecnn import CASES, config, env_config, fixture_path


def _inventory(tag):
    return json.loads(str(np.load(fixture_path(tag))["inventory"]))[tag]


def test_exported():
    for name in ("NatureCNN", "NatureCNN_Module", "MultipleCNN", "MultipleCNN_Module"):
        assert name in ocrs.__all__ and hasattr(ocrs, name)
    from ocrl_amd import _lib
    L = _lib.lib()
    for sym in ("ocrl_naturecnn_ws_floats", "ocrl_naturecnn_fwd", "ocrl_naturecnn_bwd"):
        assert hasattr(L, sym)
    assert L.ocrl_abi_version() == 5


@pytest.mark.parametrize("tag", list(CASES))
def test_state_dict_rep_dim_and_num_slots_match_the_reference(tag):
    m = getattr(ocrs, CASES[tag][0] + "_Module")(config(tag), env_config(tag))
    inv = _inventory(tag)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == inv["params"]
    assert (m.rep_dim, m.num_slots) == (inv["rep_dim"], inv["num_slots"])


def test_wrapper_has_the_reference_optimiser_and_loads_its_checkpoint():
    cfg = types.SimpleNamespace(name="NatureCNN", rep_dim=512, use_cnn_feat=False, cnn_feat_size=4, learning=types.SimpleNamespace(lr=1e-4))
    env = types.SimpleNamespace(obs_size=64, obs_channels=3)
    w = ocrs.NatureCNN(cfg, env)
    assert isinstance(w._opt, torch.optim.Adam) and w._opt.param_groups[0]["lr"] == 1e-4
    assert (w.rep_dim, w.num_slots) == (512, 1) and w.get_samples(None) == {}
    ck = w.save()
    w2 = ocrs.NatureCNN(cfg, env)
    w2.load(ck)
    for (k, a), (_, b) in zip(w._module.state_dict().items(), w2._module.state_dict().items()):
        assert torch.equal(a, b), k


def _ws(B=32, S=64, C=3, G=1, feat=4, use_feat=0, rep=512):
    from ocrl_amd import _lib
    return _lib.lib().ocrl_naturecnn_ws_floats(B, S, S, C, G, feat, use_feat, rep)


def test_workspace_contract():
    a, b = _ws(4), _ws(32)
    assert 0 < a < b < _ws(256)
    assert _ws(32, G=5) > _ws(32)
    assert _ws(32, S=36) > 0 and _ws(32, S=35) == 0               # 36 x 36 is the smallest non-empty map
    assert _ws(32, S=52, feat=2) > 0 and _ws(32, S=51, feat=2) == 0
    assert _ws(0) == 0 and _ws(32, C=0) == 0
    assert _ws(32, rep=30) == 0 and _ws(32, rep=0) == 0
    assert _ws(32, use_feat=1, rep=0) > 0 and _ws(32, use_feat=1, feat=3) == 0
    assert _ws(32, G=2, use_feat=1) == 0 and _ws(32, G=0) == 0 and _ws(32, G=17) == 0
    from ocrl_amd import _lib
    _ws(32, S=35)
    assert "at least 36 x 36" in _lib.lib().ocrl_last_error().decode()         # the reason is left for ocrl_last_error()


def test_rejected_configs():
    env = types.SimpleNamespace(obs_size=32, obs_channels=3)
    with pytest.raises(ValueError):
        ocrs.NatureCNN_Module(types.SimpleNamespace(rep_dim=512, use_cnn_feat=False, cnn_feat_size=4), env)
    with pytest.raises(ValueError):
        ocrs.NatureCNN_Module(types.SimpleNamespace(rep_dim=512, use_cnn_feat=True, cnn_feat_size=3),
                              types.SimpleNamespace(obs_size=64, obs_channels=3))


def test_cpu_tensors_raise():
    m = ocrs.NatureCNN_Module(config("default"), env_config("default"))
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(2, 3, 64, 64))
    mm = ocrs.MultipleCNN_Module(config("multi2"), env_config("multi2"))
    with pytest.raises(RuntimeError, match="GPU"):
        mm(torch.zeros(2, 3, 64, 64))


def test_multiple_cnn_leaves_the_callers_config_alone():
    cfg = types.SimpleNamespace(name="MultipleCNN", rep_dim=16, num_modules=2, cnn_feat_size=2, use_cnn_feat=True)
    m = ocrs.MultipleCNN_Module(cfg, types.SimpleNamespace(obs_size=64, obs_channels=3))
    assert (cfg.cnn_feat_size, cfg.use_cnn_feat) == (2, True)
    assert len(m._cnns) == 2 and all(not c._use_cnn_feat and c._cnn_feat_size == 4 for c in m._cnns)
    assert (m.rep_dim, m.num_slots) == (16, 2)


def _rl_config(ocr, pooling, checkpoint=""):
    return types.SimpleNamespace(
        ocr=ocr, env=types.SimpleNamespace(obs_size=64, obs_channels=3), num_envs=1, device="cpu",
        pooling=types.SimpleNamespace(name=pooling, ocr_checkpoint=types.SimpleNamespace(local_file=checkpoint, run_id="", finetuning=False),
                                      learn_aux_loss=False, learn_downstream_loss=False))


def test_extractor_trains_these_encoders_without_a_checkpoint():
    from ocrl_amd.sb3s.ocr_extractor import OCRExtractor
    cfg = _rl_config(types.SimpleNamespace(name="NatureCNN", rep_dim=512, use_cnn_feat=False, cnn_feat_size=4), "Identity")
    ex = OCRExtractor(None, cfg)
    assert ex._trainable and isinstance(ex._ocr, ocrs.NatureCNN_Module)
    assert any(n.startswith("_ocr._cnn.0.") for n, _ in ex.named_parameters())
    assert ex.features_dim == 512
    cfg = _rl_config(types.SimpleNamespace(name="MultipleCNN", rep_dim=64, num_modules=5), "MLP")
    cfg.pooling.dims, cfg.pooling.acts = [32], ["relu"]
    ex = OCRExtractor(None, cfg)
    assert ex._trainable and isinstance(ex._ocr, ocrs.MultipleCNN_Module)


def test_extractor_freezes_them_from_a_checkpoint(tmp_path):
    from ocrl_amd.sb3s.ocr_extractor import OCRExtractor
    ocr_cfg = types.SimpleNamespace(name="NatureCNN", rep_dim=512, use_cnn_feat=False, cnn_feat_size=4)
    w = ocrs.NatureCNN(ocr_cfg, types.SimpleNamespace(obs_size=64, obs_channels=3))
    path = str(tmp_path / "ocr.pt")
    torch.save(w.save(), path)
    ex = OCRExtractor(None, _rl_config(ocr_cfg, "Identity", path))
    assert not ex._trainable and not any(n.startswith("_ocr") for n, _ in ex.named_parameters())


def test_pooling_learn_downstream_loss_admits_them():
    w = ocrs.NatureCNN(config("default"), env_config("default"))
    pcfg = types.SimpleNamespace(name="MLP", dims=[32], acts=["relu"], learn_aux_loss=False, learn_downstream_loss=True,
                                 learning=types.SimpleNamespace(lr=1e-3))
    p = poolings.MLP(w, pcfg)
    assert p._learn_downstream_loss and not hasattr(w._module, "finetune_through_slots")
