"""The first layer of both spatial-broadcast decoders (csrc/bcast_l1.hip: position term + per-slot tap sums by border class) on
its own, against the plain convolution in float64 on the engine's own slots.  Compared once over the whole map and once over the
border ring alone, where every pixel takes a border class other than the interior's.  Tolerance: tensors 1e-4, as in
test_gpu_slate.py and test_gpu_iodine.py (the same layer in float32 on the CPU is 6.3e-7 / 2.7e-7 off float64 at these shapes)."""
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import dims_from_cfg, load_params, log, relerr
from tests.test_gpu_iodine import TINY, dims as iodine_dims
from tests.test_gpu_slate import BC
from oracle import iodine_oracle as IO
from oracle import slate_oracle as O

pytestmark = pytest.mark.gpu


def check_layer1(tag, c1, pre, act, ring):
    """c1: the engine's activation [BK,S,S,64]; pre: the reference pre-activation [BK,64,S,S] (float64); ring: the border's width"""
    pos = (pre > 0).double().mean().item()
    assert 0.2 < pos < 0.8, (tag, pos)          # a degenerate reference (all closed / all open units) would compare nothing
    got, ref = c1.permute(0, 3, 1, 2).double().cpu(), act(pre)
    S = pre.shape[-1]
    edge = torch.ones(S, S, dtype=torch.bool)
    edge[ring:S - ring, ring:S - ring] = False
    e_all, e_ring = relerr(got, ref), relerr(got[..., edge], ref[..., edge])
    log(f"[{tag}] first layer: whole map {e_all:.2e} border ring {e_ring:.2e} ({pos:.0%} of the pre-activations positive)")
    assert e_all < 1e-4 and e_ring < 1e-4, (tag, e_all, e_ring)


def test_slate_broadcast_first_layer():
    """5x5 / ReLU at 16x16, B*K = 12: all 25 border classes, 12 interior rows (strided row walk and row reduce over several terms)"""
    from ocrl_amd.engine import SlateEngine
    cfg, B = O.default_cfg(**BC), 2
    P = O.formula_params(cfg)
    eng = SlateEngine(dims_from_cfg(cfg), max_batch=B + 1)
    load_params(eng, P)
    S, K, D = cfg.obs_size, cfg.num_slots, cfg.slot_size
    obs = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(21))
    noise = O.make_noise(cfg, B, 30)
    eng.forward(obs.cuda(), O.schedules(cfg, 0)[0], train=False, seed=0, noise=dict(slots=noise["slots"].cuda()))
    torch.cuda.synchronize()
    slots = eng.tensor("slots", (B, K, D)).double().cpu()
    P64 = {n: P[n].double() for n in ("_dec._pos_emb.channels_map.weight", "_dec._pos_emb.channels_map.bias", "_dec._decoder.0.m.weight", "_dec._decoder.0.m.bias")}
    # the first layer of slate_oracle.broadcast_decoder
    x = slots.reshape(B * K, D, 1, 1).expand(B * K, D, S, S)
    x = x + F.conv2d(O.position_grid(S).double(), P64["_dec._pos_emb.channels_map.weight"], P64["_dec._pos_emb.channels_map.bias"])
    pre = F.conv2d(x, P64["_dec._decoder.0.m.weight"], P64["_dec._decoder.0.m.bias"], padding=2)
    check_layer1("slate bcdec16", eng.tensor("bc_c1", (B * K, S, S, 64)), pre, F.relu, 2)


def test_iodine_broadcast_first_layer():
    """3x3 / ELU at 16x16, 3 slots, the last of 3 iterations: all 9 border classes, 14 interior rows"""
    from ocrl_amd.engine import IodineEngine
    cfg, B = IO.default_cfg(**TINY), 2
    P = IO.formula_params(cfg)
    eng = IodineEngine(iodine_dims(cfg), max_batch=B)
    load_params(eng, P)
    S, K, L = cfg.obs_size, cfg.num_slots, cfg.slot_size
    obs = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(100))
    eng.forward(obs.cuda(), seed=1, noise=IO.make_noise(cfg, B, 7).cuda())
    torch.cuda.synchronize()
    slots = eng.tensor("slots", (B, K, L)).double().cpu()
    # the first layer of iodine_oracle.decoder
    x = slots.reshape(B * K, L)[:, :, None, None].expand(B * K, L, S, S)
    x = torch.cat((x, IO.coords(S, torch.float64)[None].expand(B * K, 2, S, S)), dim=1)
    pre = F.conv2d(x, P["decoder.mlc.layers.0.weight"].double(), P["decoder.mlc.layers.0.bias"].double(), padding=1)
    check_layer1("iodine tiny", eng.tensor("dec_c1", (B * K, S, S, 64)), pre, F.elu, 1)
