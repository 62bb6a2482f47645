"""GPU parity of the Transformer pooling head over long token sequences (ocrl_pool_transformer_long_*: a CNN feature map as tokens,
SLATE with use_cnn_feat) against oracle/pooling_oracle.py, the reference fixture, the short path, and through the Python surface."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from oracle import pooling_oracle as PO
from tests.golden.make_golden_pooling_long import CASES as GOLD_CASES, cotangent, sample, tokens
from tests.gpu_util import log, relerr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def run_hip(cfg, P, slots, cot, p_drop=0.0, seed=0, want_dslots=True, long=True):
    lib, L = _lib()
    B, K, Din = slots.shape
    d, h, ff, nl = cfg.d_model, cfg.nhead, cfg.dim_feedforward, cfg.num_layers
    names = [n for n, _ in PO.param_shapes(cfg)]
    w = [P[n].cuda().contiguous() for n in names]
    g = [torch.full_like(t, float("nan")) for t in w]
    pe = PO.pos_table(cfg)
    pos = None if pe is None else pe.cuda().contiguous()
    xs, dc = slots.cuda().contiguous(), cot.cuda().contiguous()
    out = torch.empty(B, d, device="cuda")
    ds = torch.full_like(xs, float("nan")) if want_dslots else None
    if long:
        n = L.ocrl_pool_transformer_long_ws_floats(B, K, Din, d, h, ff, nl)
        fwd, bwd = L.ocrl_pool_transformer_long_fwd, L.ocrl_pool_transformer_long_bwd
    else:
        n = L.ocrl_pool_transformer_ws_floats(B, K, d, h, ff, nl)
        fwd, bwd = L.ocrl_pool_transformer_fwd, L.ocrl_pool_transformer_bwd
    ws = torch.empty(n, device="cuda")
    arr = (ctypes.c_void_p * len(w))(*[t.data_ptr() for t in w])
    garr = (ctypes.c_void_p * len(g))(*[t.data_ptr() for t in g])
    lib.check(fwd(lib.ptr(xs), arr, lib.ptr(pos), lib.ptr(out), B, K, Din, d, h, ff, nl, p_drop, seed, lib.ptr(ws), n, None))
    lib.check(bwd(lib.ptr(xs), lib.ptr(dc), arr, lib.ptr(ds), garr, B, K, Din, d, h, ff, nl, p_drop, seed, lib.ptr(ws), n, None))
    torch.cuda.synchronize()
    return out.cpu(), dict(zip(names, [t.cpu() for t in g])), None if ds is None else ds.cpu()


def hip_masks(cfg, B, p_drop, seed):
    lib, L = _lib()
    S, d, ff, h = cfg.num_slots + 1, cfg.d_model, cfg.dim_feedforward, cfg.nhead
    masks = {}
    for l in range(cfg.num_layers):
        for which, (key, shape) in enumerate((("attn", (B, h, S, S)), ("drop1", (B, S, d)), ("ffn", (B, S, ff)), ("drop2", (B, S, d)))):
            m = torch.empty(shape, device="cuda")
            lib.check(L.ocrl_pool_transformer_dropout_mask(l, which, m.numel(), p_drop, seed, lib.ptr(m), None))
            masks[f"l{l}.{key}"] = m.cpu()
    return masks


def compare(tag, got, ref, tol_out=2e-5, tol_g=3e-4):
    out, g, ds = got
    r_out, r_g, r_ds = ref
    e_out = relerr(out, r_out)
    gmax = max(v.abs().max().item() for v in r_g.values())
    rows = sorted(((relerr(g[n], r_g[n], floor=1e-4 * gmax), n) for n in r_g), reverse=True)
    e_ds = relerr(ds, r_ds) if ds is not None else 0.0
    log(f"[pool long {tag}] out {e_out:.2e} dslots {e_ds:.2e} grads worst {rows[0][0]:.2e} ({rows[0][1]})")
    assert e_out < tol_out, e_out
    assert e_ds < tol_g, e_ds
    assert rows[0][0] < tol_g, rows[:4]


def oracle_out(P, x, cfg):
    """eval-mode oracle one sample at a time (the [h, S, S] weights of a 64x64 map are 0.5 GB per sample)"""
    with torch.no_grad():
        return torch.cat([PO.forward(P, x[b:b + 1], cfg) for b in range(x.shape[0])])


def _inputs(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, cfg.num_slots, cfg.rep_dim, generator=g), torch.randn(B, cfg.d_model, generator=g)


# (S, Din, L, pos, B): every value of each axis appears; d_model 128 / 8 heads / ff 512 unless given
EVAL = [(33, 67, 1, "None", 1), (33, 64, 2, "ape", 5), (257, 67, 1, "ape", 2), (257, 192, 2, "None", 1), (257, 64, 1, "None", 5),
        (1025, 67, 2, "ape", 2), (1025, 192, 1, "ape", 1), (1025, 64, 1, "None", 2), (33, 192, 1, "ape", 2), (4097, 67, 1, "ape", 1)]


@pytest.mark.parametrize("S,Din,L,pos,B", EVAL)
def test_eval_matches_oracle(S, Din, L, pos, B):
    cfg = PO.default_cfg(rep_dim=Din, num_slots=S - 1, num_layers=L, pos_emb=pos, dim_feedforward=512)
    P = PO.formula_params(cfg)
    slots, cot = _inputs(cfg, B, 11)
    ref = PO.loss_and_grads(P, slots, cfg, cot, dtype=torch.float64 if S < 4097 else torch.float32)     # fp64 scores of 4097^2: too large
    compare(f"S{S} Din{Din} L{L} {pos} B{B}", run_hip(cfg, P, slots, cot), ref)


@pytest.mark.parametrize("over", [dict(d_model=256, nhead=16, num_layers=2), dict(d_model=192, nhead=4, num_layers=2),
                                  dict(d_model=64, nhead=2, num_layers=2), dict(d_model=128, nhead=4, num_layers=1)],
                         ids=["hd16_d256", "hd48", "hd32_d64", "hd32"])
def test_head_sizes_match_oracle(over):
    cfg = PO.default_cfg(rep_dim=67, num_slots=100, dim_feedforward=256, pos_emb="ape", **over)
    P = PO.formula_params(cfg)
    slots, cot = _inputs(cfg, 2, 12)
    compare(str(over), run_hip(cfg, P, slots, cot), PO.loss_and_grads(P, slots, cfg, cot, dtype=torch.float64))


@pytest.mark.parametrize("tag,K,L,B", GOLD_CASES)
def test_matches_reference_fixture(tag, K, L, B):
    """straight against the numbers the reference module produced (tests/golden/make_golden_pooling_long.py)"""
    fx = np.load(os.path.join(GOLD, "pooling_cnnfeat.npz"))
    rep, _, d, nhead, _, ff, _, _ = [int(v) for v in fx[tag + ":cfg"]]
    cfg = PO.default_cfg(rep_dim=rep, num_slots=K, d_model=d, nhead=nhead, num_layers=L, dim_feedforward=ff, pos_emb="ape")
    out, g, ds = run_hip(cfg, PO.formula_params(cfg), tokens(B, K, rep), cotangent(B, d))
    ref = torch.from_numpy(fx[tag + ":out"])
    e_out = relerr(out, ref)
    gmax = max(np.abs(fx[tag + ":g:" + n][3:]).max() for n in g)
    worst = 0.0
    for n, t in list(g.items()) + [("dslots", ds)]:
        r = fx[tag + (":dslots" if n == "dslots" else ":g:" + n)][3:]
        worst = max(worst, np.abs(sample(t)[3:] - r).max() / max(np.abs(r).max(), 1e-3 * gmax))
    log(f"[pool long fixture {tag}] out {e_out:.2e} grads worst {worst:.2e}")
    assert e_out < 2e-5 and worst < 3e-4


@pytest.mark.parametrize("L,K,over", [(1, 256, {}), (2, 256, {}), (2, 31, dict(d_model=192, nhead=4))], ids=["S257_l1", "S257_l2", "rows64_d192"])
def test_train_mode_dropout_parity(L, K, over):
    """train mode: the oracle consumes the keep-masks ocrl_pool_transformer_dropout_mask exports for the same (seed, layer, site).  The last
    case has B*S = 64 rows of width 192 (the dX products there run as two halves)"""
    cfg = PO.default_cfg(rep_dim=67, num_slots=K, num_layers=L, pos_emb="ape", dim_feedforward=512, **over)
    P = PO.formula_params(cfg)
    B = 2
    slots, cot = _inputs(cfg, B, 5)
    p, seed = cfg.dropout, 0x1234567800000009
    masks = hip_masks(cfg, B, p, seed)
    keep = np.mean([m.mean().item() for m in masks.values()])
    assert abs(keep - (1 - p)) < 0.02, keep
    compare(f"train L{L} K{K}", run_hip(cfg, P, slots, cot, p, seed), PO.loss_and_grads(P, slots, cfg, cot, masks, p, dtype=torch.float64))


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_long_path_agrees_with_short_path(p):
    """K = 6 slots of width 192 through both C entry points: the same maths and the same dropout decisions"""
    cfg = PO.default_cfg(num_layers=2)
    P = PO.formula_params(cfg)
    slots, cot = _inputs(cfg, 3, 7)
    a = run_hip(cfg, P, slots, cot, p, 99, long=True)
    b = run_hip(cfg, P, slots, cot, p, 99, long=False)
    compare(f"long vs short p={p}", a, b)


def test_large_map_deterministic_and_permutation_invariant():
    """S = 16385 (a 128x128 map), B = 1: two runs are bitwise equal; without positions, permuting the tokens permutes dslots only"""
    cfg = PO.default_cfg(rep_dim=67, num_slots=16384, dim_feedforward=512)
    P = PO.formula_params(cfg)
    slots, cot = _inputs(cfg, 1, 3)
    a = run_hip(cfg, P, slots, cot)
    b = run_hip(cfg, P, slots, cot)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])
    perm = torch.randperm(cfg.num_slots, generator=torch.Generator().manual_seed(1))
    c = run_hip(cfg, P, slots[:, perm], cot)
    gmax = max(v.abs().max().item() for v in a[1].values())
    e = dict(out=relerr(c[0], a[0]), dslots=relerr(c[2], a[2][:, perm]),
             grads=max(relerr(c[1][n], a[1][n], floor=1e-4 * gmax) for n in a[1]))
    log(f"[pool long S16385] permutation: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["out"] < 2e-5 and e["dslots"] < 3e-4 and e["grads"] < 3e-4, e


def test_bad_arguments():
    lib, L = _lib()
    x = torch.zeros(64, device="cuda")
    arr = (ctypes.c_void_p * 15)(*[x.data_ptr()] * 15)
    f = L.ocrl_pool_transformer_long_fwd
    assert f(None, None, None, None, 2, 4096, 67, 128, 8, 2048, 1, 0.0, 0, None, 0, None) != 0
    assert b"null" in L.ocrl_last_error()
    assert f(lib.ptr(x), arr, None, lib.ptr(x), 2, 4096, 67, 128, 8, 2048, 1, 0.0, 0, lib.ptr(x), 64, None) != 0
    assert b"workspace" in L.ocrl_last_error()
    assert f(lib.ptr(x), arr, None, lib.ptr(x), 2, 4096, 67, 128, 16 * 8, 2048, 1, 0.0, 0, lib.ptr(x), 64, None) != 0
    assert b"head size" in L.ocrl_last_error()
    assert f(lib.ptr(x), arr, None, lib.ptr(x), 2, 4096, 67, 96, 8, 2048, 1, 0.0, 0, lib.ptr(x), 64, None) != 0
    assert b"d_model" in L.ocrl_last_error()
    assert f(lib.ptr(x), arr, None, lib.ptr(x), 2, 0, 67, 128, 8, 2048, 1, 0.0, 0, lib.ptr(x), 64, None) != 0
    assert f(lib.ptr(x), arr, None, lib.ptr(x), 2, 4096, 67, 128, 8, 2048, 9, 0.0, 0, lib.ptr(x), 64, None) != 0
    assert b"num_layers" in L.ocrl_last_error()
    # the short path keeps its contract
    assert L.ocrl_pool_transformer_fwd(lib.ptr(x), arr, None, lib.ptr(x), 2, 40, 192, 128, 8, 2048, 1, 0.0, 0, lib.ptr(x), 8, None) != 0
    assert b"num_slots" in L.ocrl_last_error()


def _pool_cfg(**over):
    c = types.SimpleNamespace(name="Transformer", rep_dim=128, d_model=128, nhead=8, num_layers=1, pos_emb="ape", norm_first=False, use_mlp1=False,
                              use_mlp2=False, cw_embedding=False, push_embedding=False, learn_aux_loss=False, learn_downstream_loss=False,
                              ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=""), learning=types.SimpleNamespace(lr=1e-3))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_python_surface_trains_with_a_torch_optimizer():
    """Transformer_Module(67, 4096): the reference's state_dict (pe [4097,1,128]), autograd through the long path, torch.optim.Adam"""
    from ocrl_amd.poolings import Transformer_Module
    cfg = PO.default_cfg(rep_dim=67, num_slots=4096, pos_emb="ape")
    m = Transformer_Module(67, 4096, _pool_cfg()).cuda()
    sd = m.state_dict()
    assert tuple(sd["_trans._pos.pe"].shape) == (4097, 1, 128)
    assert [k for k in sd if not k.endswith(".pe")] == [n for n, _ in PO.param_shapes(cfg)]
    P = PO.formula_params(cfg)
    m.load_state_dict({**sd, **P})
    g = torch.Generator().manual_seed(3)
    slots = torch.randn(2, 4096, 67, generator=g)
    target = torch.randn(2, 128, generator=g)
    m.eval()
    assert relerr(m(slots.cuda()), oracle_out(P, slots, cfg)) < 2e-5
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = ((m(slots.cuda()) - target.cuda()) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    log(f"[pool long surface] losses {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < 0.8 * losses[0], losses
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_python_surface_ragged_width_with_few_tokens():
    """Transformer_Module(67, 6): 7 tokens fit the short path, the width 67 does not -- the module takes the long path"""
    from ocrl_amd.poolings import Transformer_Module
    cfg = PO.default_cfg(rep_dim=67, num_slots=6)
    m = Transformer_Module(67, 6, _pool_cfg(pos_emb="None")).cuda().eval()
    P = PO.formula_params(cfg)
    m.load_state_dict(P)
    g = torch.Generator().manual_seed(6)
    slots, cot = torch.randn(3, 6, 67, generator=g), torch.randn(3, 128, generator=g)
    x = slots.cuda().requires_grad_(True)
    out = m(x)
    (out * cot.cuda()).sum().backward()
    r_out, r_g, r_ds = PO.loss_and_grads(P, slots, cfg, cot, dtype=torch.float64)
    named = dict(m.named_parameters())
    compare("module K6 Din67", (out.detach().cpu(), {n: named[n].grad.cpu() for n in r_g}, x.grad.cpu()), (r_out, r_g, r_ds))


def test_slate_cnn_extractor_matches_oracle(tmp_path):
    """SLATE-CNN: ocr=slate ocr.use_cnn_feat=True pooling=transformer pooling.pos_emb=ape with a pre-trained (frozen) encoder at 64x64"""
    from ocrl_amd import ocrs, poolings
    from ocrl_amd.sb3s import OCRExtractor
    from ocrl_amd.utils.config import compose
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ocr_cfg = compose(os.path.join(root, "configs"), "train_ocr", ["ocr=slate", "ocr.use_cnn_feat=True", "ocr.slotattr.num_slots=5",
                                                                     "ocr.dvae.vocab_size=256", "ocr.tfdec.num_dec_blocks=1", "dataset=random-N5C4S4S2",
                                                                     "dataset.obs_size=64"])
    ocr = ocrs.SLATE(ocr_cfg.ocr, ocr_cfg.dataset)
    assert (ocr.num_slots, ocr.rep_dim) == (4096, 67)
    ck = tmp_path / "slate.pth"
    torch.save(ocr.save(), ck)
    pcfg = _pool_cfg(ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=str(ck), finetuning=False))
    full = types.SimpleNamespace(ocr=ocr_cfg.ocr, env=ocr_cfg.dataset, pooling=pcfg, num_envs=4, device="cuda:0")
    ex = OCRExtractor(None, full).to("cuda:0")
    ex.eval()
    obs = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)).cuda()
    f = ex(obs)
    assert f.shape == (2, ex.features_dim) and torch.isfinite(f).all()
    feat = ex._ocr(obs)
    assert feat.shape == (2, 4096, 67)
    P = {k: t.detach().cpu() for k, t in ex._pooling.state_dict().items() if not k.endswith(".pe")}
    cfg = PO.default_cfg(rep_dim=67, num_slots=4096, pos_emb="ape")
    e = relerr(f, oracle_out(P, feat.cpu(), cfg))
    log(f"[pool long SLATE-CNN extractor] out {e:.2e}")
    assert e < 2e-5
    # the wrapper: poolings.Transformer over the same frozen encoder; a gradient into the conv encoder stays unsupported
    pool = poolings.Transformer(ocr, pcfg)
    pool.to("cuda:0")
    pool.eval()
    assert pool(obs).shape == (2, 128)
    with pytest.raises(NotImplementedError):
        poolings.Transformer(ocr, _pool_cfg(learn_downstream_loss=True))
