"""CPU checks of the MAE module: the sin-cos position table against the reference's fixture, exported names and C symbols, state_dict
names and shapes, rep_dim / num_slots, the ocr=mae config, the workspace contract (rejected shapes) and the restatement's two
embedding orders (tests/mae_ref.py)."""
import os
import types

import numpy as np
import pytest
import torch

from ocrl_amd import ocrs
from ocrl_amd.ocrs import mae as M
from tests import mae_ref as R
from tests.golden import make_golden_mae as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(**kw):
    c = dict(name="MAE", vit_size="base", patch_size=8, return_cls=False, masking_ratio=0.75,
             learning=types.SimpleNamespace(lr=1e-3, weight_decay=0.05))
    c.update(kw)
    return types.SimpleNamespace(**c)


def env_config(obs_size=64):
    return types.SimpleNamespace(obs_size=obs_size, obs_channels=3)


def block_names(prefix, d):
    return [(prefix + n, sh) for n, sh in [
        ("norm1.weight", [d]), ("norm1.bias", [d]), ("attn.qkv.weight", [3 * d, d]), ("attn.qkv.bias", [3 * d]), ("attn.proj.weight", [d, d]),
        ("attn.proj.bias", [d]), ("norm2.weight", [d]), ("norm2.bias", [d]), ("mlp.fc1.weight", [4 * d, d]), ("mlp.fc1.bias", [4 * d]),
        ("mlp.fc2.weight", [d, 4 * d]), ("mlp.fc2.bias", [d])]]


def expected_state_dict(D, depth, Dd, ddepth, L, p):
    names = [("cls_token", [1, 1, D]), ("pos_embed", [1, L + 1, D]), ("mask_token", [1, 1, Dd]), ("decoder_pos_embed", [1, L + 1, Dd]),
             ("patch_embed.proj.weight", [D, 3, p, p]), ("patch_embed.proj.bias", [D])]
    for i in range(depth):
        names += block_names(f"blocks.{i}.", D)
    names += [("norm.weight", [D]), ("norm.bias", [D]), ("decoder_embed.weight", [Dd, D]), ("decoder_embed.bias", [Dd])]
    for i in range(ddepth):
        names += block_names(f"decoder_blocks.{i}.", Dd)
    names += [("decoder_norm.weight", [Dd]), ("decoder_norm.bias", [Dd]), ("decoder_pred.weight", [3 * p * p, Dd]), ("decoder_pred.bias", [3 * p * p])]
    return [["_mae." + n, sh] for n, sh in names]


@pytest.mark.parametrize("dim,grid", G.CASES)
def test_position_table_matches_the_reference_bit_for_bit(dim, grid):
    fx = np.load(G.fixture_path())[G.key(dim, grid)]
    ours = M.sincos_2d(dim, grid)
    assert ours.shape == fx.shape == (grid * grid + 1, dim)
    assert np.array_equal(ours.astype(np.float32), fx.astype(np.float32))


def test_exported_and_symbols():
    assert "MAE" in ocrs.__all__ and "MAE_Module" in ocrs.__all__
    from ocrl_amd import _lib
    L = _lib.lib()
    for sym in ("ocrl_mae_ws_floats", "ocrl_mae_fwd", "ocrl_mae_bwd", "ocrl_mae_rank"):
        assert hasattr(L, sym)


def test_state_dict_names_shapes_and_attributes():
    m = ocrs.MAE_Module(config(), env_config(64))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == expected_state_dict(768, 12, 512, 8, 64, 8)
    assert [tuple(p.shape) for p in m.parameters()] == M.param_shapes(64, 8, M.VIT["base"], M.DECODER)
    assert (m.rep_dim, m.num_slots, m.trains_through_autograd, m.len_keep) == (768, 64, True, 16)
    assert not m._mae.pos_embed.requires_grad and not m._mae.decoder_pos_embed.requires_grad
    assert torch.equal(m._mae.pos_embed[0], torch.from_numpy(M.sincos_2d(768, 8)).float())
    m = ocrs.MAE_Module(config(return_cls=True), env_config(64))
    assert (m.rep_dim, m.num_slots) == (768, 1)


def test_large_and_initialisation():
    m = ocrs.MAE_Module(config(vit_size="large", patch_size=16, _test_dims=((1024, 1, 16), (512, 1, 16))), env_config(64))
    assert (m.rep_dim, m.num_slots) == (1024, 16)
    sd = m.state_dict()
    # every Linear / LayerNorm bias is zero; the patch projection is a Conv2d, whose bias the reference leaves at torch's default
    assert all(float(v.abs().max()) == 0 for k, v in sd.items() if k.endswith(".bias") and "patch_embed" not in k)
    assert all(bool((v == 1).all()) for k, v in sd.items() if "norm" in k and k.endswith(".weight"))
    w = sd["_mae.blocks.0.mlp.fc1.weight"]
    bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5                 # xavier-uniform
    assert float(w.abs().max()) <= bound * (1 + 1e-6) and float(w.abs().max()) > 0.9 * bound
    assert 0.01 < float(sd["_mae.cls_token"].std()) < 0.03
    with pytest.raises(ValueError):
        ocrs.MAE_Module(config(), env_config(60))
    with pytest.raises(ValueError):
        ocrs.MAE_Module(config(vit_size="huge"), env_config(64))


def _ws(B=2, S=16, p=4, D=64, depth=2, h=2, Dd=32, ddepth=1, dh=2, keep=4, full=1):
    from ocrl_amd import _lib
    return _lib.lib().ocrl_mae_ws_floats(B, S, p, D, depth, h, Dd, ddepth, dh, keep, full)


def test_workspace_contract():
    assert 0 < _ws(B=1) < _ws(B=4)
    assert _ws(full=0) > 0 and _ws(full=0, keep=16) < _ws(full=1, keep=16)      # the decoder's buffers come on top at the same token count
    assert _ws(S=18) == 0                                              # obs_size % patch != 0
    assert _ws(h=1, D=96) == 0 and _ws(dh=1, Dd=128) == 0 and _ws(h=8) == 0      # head sizes 96, 128, 8
    assert _ws(S=9, p=3) == 0                                          # 3 p^2 = 27 is no multiple of 4
    assert _ws(D=66, h=1) == 0 and _ws(Dd=34, dh=1) == 0               # widths that are no multiple of 4
    assert _ws(S=132, p=4, keep=4) == 0 and _ws(S=128, p=4, keep=4) > 0      # L = 1089 > 1024; L = 1024 is accepted
    assert _ws(keep=0) == 0 and _ws(keep=17) == 0 and _ws(keep=16) > 0 and _ws(keep=0, full=0) > 0
    assert _ws(B=0) == 0
    from ocrl_amd import _lib
    assert _ws(keep=0) == 0 and b"len_keep" in _lib.lib().ocrl_last_error()


def test_cpu_tensors_raise():
    m = ocrs.MAE_Module(config(_test_dims=((64, 1, 2), (32, 1, 2))), env_config(16))
    with pytest.raises(RuntimeError):
        m(torch.rand(2, 3, 16, 16))
    with pytest.raises(RuntimeError):
        m.get_loss(torch.rand(2, 3, 16, 16))
    with pytest.raises(ValueError):
        m(torch.rand(2, 3, 32, 32))


def test_wrapper_optimiser():
    w = ocrs.MAE(config(_test_dims=((64, 1, 2), (32, 1, 2))), env_config(16))
    assert isinstance(w._opt, torch.optim.AdamW)
    g = w._opt.param_groups
    assert len(g) == 1 and g[0]["lr"] == 1e-3 and tuple(g[0]["betas"]) == (0.9, 0.95) and g[0]["weight_decay"] == 1e-2
    assert (w.rep_dim, w.num_slots) == (64, 4)
    from ocrl_amd.ocrs.base import AutogradUpdate
    assert isinstance(w, AutogradUpdate) and issubclass(ocrs.VAE, AutogradUpdate)


def test_compose_ocr_mae():
    from ocrl_amd.utils.config import compose
    cfg = compose(os.path.join(ROOT, "configs"), "train_ocr", ["ocr=mae", "dataset=random-N5C4S4S2"])
    assert cfg.ocr.name == "MAE" and cfg.ocr.vit_size == "base" and cfg.ocr.patch_size == 8 and cfg.ocr.return_cls is False
    assert cfg.ocr.masking_ratio == 0.75 and cfg.ocr.learning.lr == 1e-3 and cfg.ocr.learning.weight_decay == 0.05
    assert hasattr(ocrs, cfg.ocr.name)


@pytest.mark.parametrize("S,p,keep", [(16, 4, 4), (24, 8, 2)])
def test_restatement_embedding_orders_agree(S, p, keep):
    enc, dec = (64, 2, 2), (32, 1, 2)
    L = (S // p) ** 2
    w = R.make_params(L, p, enc, dec, seed=3)
    g = torch.Generator().manual_seed(5)
    obs = torch.rand(2, 3, S, S, generator=g, dtype=torch.float64)
    noise = torch.stack([torch.randperm(L, generator=g).double() / L for _ in range(2)])
    a = R.loss_terms(obs, w, noise, p, enc, dec, keep)
    b = R.loss_terms(obs, w, noise, p, enc, dec, keep, gather_first=True)
    assert torch.equal(a["mask"], b["mask"]) and a["mask"].sum() == 2 * (L - keep)
    for k in ("loss", "pred", "rep"):
        assert torch.allclose(a[k], b[k], rtol=1e-12, atol=1e-13), k
    # the full-patch encoder equals the masked encoder when nothing is masked and the noise is sorted
    full = R.encode_full(obs, w, p, enc[1], enc[2])
    ident = torch.arange(L, dtype=torch.float64).expand(2, L) / L
    assert torch.allclose(R.loss_terms(obs, w, ident, p, enc, dec, L)["rep"], full, rtol=1e-12, atol=1e-13)
    # ties break by index
    keep_ids, mask, restore = R.masking(torch.zeros(2, L, dtype=torch.float64), keep)
    assert torch.equal(restore, torch.arange(L).expand(2, L)) and torch.equal(keep_ids, torch.arange(keep).expand(2, keep))
