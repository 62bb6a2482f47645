"""CPU checks of the VAE module: exported names and C symbols, state_dict names and shapes against the reference fixture, the fp64
restatement of the reference's loss (tests/golden/make_golden_vae.py: ref_loss) against the fixture's metrics, mu, rep, recon and
gradients, the workspace contract, the no-CPU-fallback rule, and the ocr=vae config."""
import json
import os
import types

import numpy as np
import pytest
import torch

from ocrl_amd import ocrs
from tests.golden import make_golden_vae as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_and_symbols():
    assert "VAE" in ocrs.__all__ and "VAE_Module" in ocrs.__all__
    from ocrl_amd import _lib
    L = _lib.lib()
    for sym in ("ocrl_vae_ws_floats", "ocrl_vae_fwd", "ocrl_vae_bwd"):
        assert hasattr(L, sym)
    assert L.ocrl_abi_version() == 5


@pytest.mark.parametrize("tag", list(G.CASES))
def test_state_dict_matches_the_reference(tag):
    inv = json.loads(str(np.load(G.fixture_path())["inventory"]))[tag]
    m = ocrs.VAE_Module(G.config(tag), G.env_config(G.CASES[tag][0]))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == inv["params"]
    assert (m.rep_dim, m.num_slots) == (inv["rep_dim"], inv["num_slots"])
    assert sum(1 for k in m.state_dict() if k.endswith(".m.weight")) == 8 * G.stages(tag) + 1


@pytest.mark.parametrize("tag", list(G.CASES))
def test_fp64_restatement_reproduces_the_fixture(tag):
    S, B, c = G.CASES[tag]
    seed = list(G.CASES).index(tag)
    fx = np.load(G.fixture_path())
    m = ocrs.VAE_Module(G.config(tag), G.env_config(S)).double()
    G.load_closed_form(m)
    ps = list(m.parameters())
    r = G.ref_loss(G.observations(B, S, seed), ps, G.noise(B, c["latent_dim"], seed), G.stages(tag), c["cnn_feat_size"], c["kld_weight"],
                   c["use_cnn_feat"])
    (r["loss"] + (r["rep"] * G.cotangent(tuple(r["rep"].shape), seed)).sum()).backward()
    assert np.allclose([r["loss"].item(), r["mse"].item(), -r["kld"].item()], fx[tag + "/loss"], rtol=1e-10)
    assert np.allclose(r["mu"].detach().numpy(), fx[tag + "/mu"], rtol=1e-9, atol=1e-12)
    rep = r["rep"].detach().numpy().ravel()
    assert np.allclose(rep[G.sample_idx(rep.size)], fx[tag + "/rep_sample"], rtol=1e-9, atol=1e-12)
    rc = r["recon"].detach().numpy().ravel()
    assert np.allclose(G.moments(rc), fx[tag + "/recon_moments"], rtol=1e-9)
    for n, p in m.named_parameters():
        g = p.grad.numpy().ravel()
        if tag + "/grad/" + n in fx:
            assert np.allclose(g, fx[tag + "/grad/" + n], rtol=1e-8, atol=1e-14), n
        else:
            assert np.allclose(g[G.sample_idx(g.size)], fx[tag + "/grads/" + n], rtol=1e-8, atol=1e-14), n


def _ws(B=24, S=64, C=3, f=4, L=256, cnn=0, full=1):
    from ocrl_amd import _lib
    return _lib.lib().ocrl_vae_ws_floats(B, S, C, f, L, cnn, full)


def test_workspace_contract():
    assert 0 < _ws(4) < _ws(24) < _ws(256)
    assert 0 < _ws(full=0) < _ws(full=1)
    assert _ws(S=32) > 0 and _ws(S=48) == 0 and _ws(S=4) == 0      # obs_size / cnn_feat_size must be a power of two >= 2
    assert _ws(C=5) == 0 and _ws(L=30) == 0 and _ws(B=0) == 0


def test_cpu_tensors_raise_and_bad_ratio_rejected():
    m = ocrs.VAE_Module(G.config("default"), G.env_config(64))
    with pytest.raises(RuntimeError):
        m(torch.rand(2, 3, 64, 64))
    with pytest.raises(RuntimeError):
        m.get_loss(torch.rand(2, 3, 64, 64))
    with pytest.raises(ValueError):
        ocrs.VAE_Module(G.config("default"), G.env_config(48))


def test_parameter_shapes_come_from_the_config():
    from ocrl_amd.ocrs.vae import param_shapes
    for tag in G.CASES:
        m = ocrs.VAE_Module(G.config(tag), G.env_config(G.CASES[tag][0]))
        assert [tuple(p.shape) for p in m.parameters()] == param_shapes(3, G.stages(tag), 4, G.CASES[tag][2]["latent_dim"])
    m = ocrs.VAE_Module(G.config("default"), G.env_config(64))
    m._mu.weight = torch.nn.Parameter(torch.zeros(128, 1024))                      # reassigned with another shape
    with pytest.raises(ValueError):
        m(torch.rand(2, 3, 64, 64))                                                   # before the device check, before any launch
    with pytest.raises(ValueError):
        m.get_loss(torch.rand(2, 3, 64, 64))
    m = ocrs.VAE_Module(G.config("default"), G.env_config(64))
    m._var.weight = torch.nn.Parameter(torch.zeros(256, 512))
    with pytest.raises(ValueError):
        m.get_loss(torch.rand(2, 3, 64, 64))


def test_wrapper_optimiser_and_checkpoint_round_trip():
    w = ocrs.VAE(G.config("default"), G.env_config(64))
    assert isinstance(w._opt, torch.optim.Adam) and w._opt.param_groups[0]["lr"] == 1e-4
    assert (w.rep_dim, w.num_slots) == (256, 1)
    w2 = ocrs.VAE(G.config("default"), G.env_config(64))
    w2.load(w.save())
    for (k, a), (_, b) in zip(w._module.state_dict().items(), w2._module.state_dict().items()):
        assert torch.equal(a, b), k


def test_compose_ocr_vae():
    from ocrl_amd.utils.config import compose
    cfg = compose(os.path.join(ROOT, "configs"), "train_ocr", ["ocr=vae", "dataset=random-N5C4S4S2"])
    assert cfg.ocr.name == "VAE" and cfg.ocr.latent_dim == 256 and cfg.ocr.use_cnn_feat is False and cfg.ocr.cnn_feat_size == 4
    assert cfg.ocr.learning.lr == 1e-4 and cfg.ocr.learning.kld_weight == 1e-4
    m = getattr(ocrs, cfg.ocr.name)(cfg.ocr, cfg.dataset)
    assert m.rep_dim == 256
