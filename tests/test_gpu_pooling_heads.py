"""GPU checks of the RN, MLP and Identity pooling heads: ocrl_pool_rn_fwd/_bwd against an fp64 autograd restatement written here and
against the reference fixtures, the ABI contract (coverage of every output, detached slots, independent images, reproducibility), and the
Python surface (poolings.RN / MLP / Identity over the SLATE encoder, a torch optimiser step, OCRExtractor with each head)."""
import ctypes
import itertools
import os
import types

import numpy as np
import pytest
import torch

from tests.golden.make_golden_pooling_heads import CASES, cotangent, fixture_path, load_closed_form, sample, slots as gold_slots
from tests.gpu_util import log, relerr

pytestmark = pytest.mark.gpu
RN_DEFAULT = dict(g_dims=[256, 256, 256, 256], f_dims=[256, 128, 64, 64])


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def rn_params(D, g_dims, f_dims, seed, grid=False):
    """weights [out, in] and biases in the ABI's (state_dict) order.  Gaussian: weights scaled by 1/sqrt(fan_in), small biases.
    grid: about four +-1 entries per weight row and half-integer biases; with integer slots every pre-activation is a half-integer that
    fp32 holds exactly, so no ReLU input sits within rounding of zero and the fp32 and fp64 masks agree"""
    gen = torch.Generator().manual_seed(seed)
    ps, i = [], 2 * D
    for o in list(g_dims) + list(f_dims):
        if grid:
            keep = torch.rand(o, i, generator=gen) < min(1.0, 4.0 / i)
            w = torch.where(keep, torch.randint(0, 2, (o, i), generator=gen).float() * 2 - 1, torch.zeros(()))
            ps += [w, torch.randint(-2, 2, (o,), generator=gen).float() + 0.5]
        else:
            ps += [torch.randn(o, i, generator=gen) * (1.4 / i ** 0.5), torch.randn(o, generator=gen) * 0.05]
        i = o
    return ps


def rn_ref64(slots, ps, ng):
    """RN_Module.forward restated in fp64: pair rows cat(s_i, s_j) in permutations order, g, the pair sum, f"""
    B, K, D = slots.shape
    pairs = list(itertools.permutations(range(K), 2))
    I = torch.tensor([i for i, _ in pairs], device=slots.device)
    J = torch.tensor([j for _, j in pairs], device=slots.device)
    x = torch.cat([slots.index_select(1, I), slots.index_select(1, J)], dim=-1)
    for l in range(len(ps) // 2):
        if l == ng:
            x = x.sum(1)
        x = torch.relu(x @ ps[2 * l].T + ps[2 * l + 1])
    return x


def run_abi(slots, ps, g_dims, f_dims, cot, want_dslots=True):
    """one forward and backward through the C ABI; out, dslots and every dw are NaN-prefilled"""
    lib, L = _lib()
    B, K, D = slots.shape
    gd, fd = (ctypes.c_int * len(g_dims))(*g_dims), (ctypes.c_int * len(f_dims))(*f_dims)
    w = [p.cuda().float().contiguous() for p in ps]
    dw = [torch.full_like(t, float("nan")) for t in w]
    xs, dc = slots.cuda().float().contiguous(), cot.cuda().float().contiguous()
    out = torch.full((B, f_dims[-1]), float("nan"), device="cuda")
    ds = torch.full_like(xs, float("nan")) if want_dslots else None
    n = L.ocrl_pool_rn_ws_floats(B, K, D, len(g_dims), gd, len(f_dims), fd)
    assert n > 0, L.ocrl_last_error()
    ws = torch.full((n,), float("nan"), device="cuda")
    arr = (ctypes.c_void_p * len(w))(*[t.data_ptr() for t in w])
    darr = (ctypes.c_void_p * len(dw))(*[t.data_ptr() for t in dw])
    lib.check(L.ocrl_pool_rn_fwd(lib.ptr(xs), arr, lib.ptr(out), B, K, D, len(g_dims), gd, len(f_dims), fd, lib.ptr(ws), n, None))
    lib.check(L.ocrl_pool_rn_bwd(lib.ptr(xs), lib.ptr(dc), arr, lib.ptr(ds), darr, B, K, D, len(g_dims), gd, len(f_dims), fd, lib.ptr(ws), n, None))
    torch.cuda.synchronize()
    return out.cpu(), None if ds is None else ds.cpu(), [t.cpu() for t in dw]


def ref_grads(slots, ps, ng, cot):
    s = slots.double().cuda().requires_grad_(True)
    p64 = [p.double().cuda().requires_grad_(True) for p in ps]
    out = rn_ref64(s, p64, ng)
    (out * cot.double().cuda()).sum().backward()
    return out.detach().cpu(), s.grad.cpu(), [p.grad.cpu() for p in p64]


# (B, K, D, g_dims, f_dims): K in {2, 3, 6, 10, 16}, D in {64, 67, 192}, 1-4 layers in g and f, widths 64-256, B in {1, 3, 37, 256}
PARITY = [
    (1, 2, 64, [64], [64]),
    (3, 3, 67, [128, 64], [64, 128, 64]),
    (37, 6, 192, RN_DEFAULT["g_dims"], RN_DEFAULT["f_dims"]),
    (256, 6, 192, RN_DEFAULT["g_dims"], RN_DEFAULT["f_dims"]),
    (256, 10, 64, [64, 128, 64], [128]),
    (3, 16, 67, [256, 256], [64, 64, 64, 64]),
    (37, 16, 192, [128, 128, 128, 128], [256, 64]),
    (1, 10, 67, [192, 64, 256], [256, 128]),
]


# grid data for every case; Gaussian data only where the pair rows are few (see test_rn_matches_fp64)
PARITY_RUNS = [(*c, True) for c in PARITY] + [(*c, False) for c in PARITY if c[0] * c[1] * (c[1] - 1) <= 1200]


@pytest.mark.parametrize("B,K,D,g_dims,f_dims,grid", PARITY_RUNS)
def test_rn_matches_fp64(B, K, D, g_dims, f_dims, grid):
    """grid data: the forward exact and the gradients within fp32 rounding of their sums.  Gaussian data: only where the pair rows
    are few (B K (K-1) <= 1200).  With 10^6 and more ReLU inputs a handful lands within fp32 rounding of zero, its fp32 and fp64 masks
    differ, and a whole pair row's contribution moves (observed: 2e-3..1e-2 of the largest gradient at B = 256)."""
    gen = torch.Generator().manual_seed(B * 1000 + K * 10 + D)
    if grid:
        slots = torch.randint(-2, 3, (B, K, D), generator=gen).float()
        cot = torch.randint(-2, 3, (B, f_dims[-1]), generator=gen).float()
    else:
        slots = torch.randn(B, K, D, generator=gen)
        cot = torch.randn(B, f_dims[-1], generator=gen)
    ps = rn_params(D, g_dims, f_dims, seed=K + D, grid=grid)
    out, ds, dw = run_abi(slots, ps, g_dims, f_dims, cot)
    r_out, r_ds, r_dw = ref_grads(slots, ps, len(g_dims), cot)
    gmax = max(t.abs().max().item() for t in r_dw)
    e_out, e_ds = relerr(out, r_out), relerr(ds, r_ds)
    e_dw = max(relerr(a, b, floor=1e-3 * gmax) for a, b in zip(dw, r_dw))
    log(f"[rn {'grid' if grid else 'gauss'} B={B} K={K} D={D} g={g_dims} f={f_dims}] out {e_out:.2e} dslots {e_ds:.2e} worst dw {e_dw:.2e}")
    if grid:
        assert r_out.abs().max().item() < 2 ** 21 and r_out.abs().max().item() > 0      # the half-integer grid is exact in fp32
        assert e_out < 1e-6 and e_ds < 1e-5 and e_dw < 1e-5
    else:
        assert e_out < 1e-4 and e_ds < 3e-4 and e_dw < 3e-4


def test_rn_matches_reference_fixtures():
    from ocrl_amd import poolings
    fx = np.load(fixture_path("rn_small"))
    for tag in ("rn_small", "rn_default"):
        _, D, K, B, c, full = CASES[tag]
        m = poolings.RN_Module(D, K, 1, types.SimpleNamespace(**c))
        load_closed_form(m)
        m.cuda()
        s = gold_slots(tag).cuda().requires_grad_(True)
        out = m(s)
        (out * cotangent(tag, out.shape[1]).cuda()).sum().backward()
        assert relerr(out, torch.from_numpy(fx[tag + ":out"])) < 2e-5, tag
        grads = [("dslots", s.grad)] + [("g:" + n, p.grad) for n, p in m.named_parameters()]
        floor = 1e-3 * max(np.abs(fx[f"{tag}:{n}"][0 if full else 3:]).max() for n, _ in grads)   # tensors whose sampled rows are dead
        for n, g in grads:
            ref = fx[f"{tag}:{n}"]
            if full:
                assert relerr(g, torch.from_numpy(ref), floor=floor) < 2e-4, (tag, n)
            else:
                got = sample(g)
                assert np.abs(got[3:] - ref[3:]).max() <= 2e-4 * max(np.abs(ref[3:]).max(), floor), (tag, n)
                assert abs(got[2] - ref[2]) <= 1e-3 * ref[2] + floor ** 2, (tag, n)           # sum of squares of the whole tensor


def test_mlp_and_identity_match_reference_fixtures():
    from ocrl_amd import poolings
    for tag in ("mlp_default", "mlp_linear", "identity"):
        head, D, K, B, c, full = CASES[tag]
        fx = np.load(fixture_path(tag))
        m = getattr(poolings, head + "_Module")(D, K, types.SimpleNamespace(**c))
        load_closed_form(m)
        m.cuda()
        s = gold_slots(tag).cuda().requires_grad_(True)
        out = m(s)
        (out * cotangent(tag, out.shape[1]).cuda()).sum().backward()
        assert relerr(out, torch.from_numpy(fx[tag + ":out"])) < 2e-5, tag
        for n, g in [("dslots", s.grad)] + [("g:" + n, p.grad) for n, p in m.named_parameters()]:
            ref = fx[f"{tag}:{n}"]
            if full:
                assert relerr(g, torch.from_numpy(ref)) < 2e-4, (tag, n)
            else:
                assert np.abs(sample(g)[3:] - ref[3:]).max() < 2e-4 * np.abs(ref[3:]).max(), (tag, n)


def test_rn_outputs_covered_detached_and_reproducible():
    B, K, D = 256, 6, 192
    gen = torch.Generator().manual_seed(5)
    slots, cot = torch.randn(B, K, D, generator=gen), torch.randn(B, 64, generator=gen)
    ps = rn_params(D, RN_DEFAULT["g_dims"], RN_DEFAULT["f_dims"], seed=7)
    a = run_abi(slots, ps, RN_DEFAULT["g_dims"], RN_DEFAULT["f_dims"], cot)
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all() and all(torch.isfinite(t).all() for t in a[2])
    b = run_abi(slots, ps, RN_DEFAULT["g_dims"], RN_DEFAULT["f_dims"], cot)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    c = run_abi(slots, ps, RN_DEFAULT["g_dims"], RN_DEFAULT["f_dims"], cot, want_dslots=False)
    assert torch.equal(a[0], c[0]) and all(torch.equal(x, y) for x, y in zip(a[2], c[2]))


def test_rn_images_are_independent():
    """a batch of different images pools as each image on its own (identical copies would hide cross-image indexing)"""
    B, K, D = 256, 6, 67
    g_dims, f_dims = [128, 64], [64, 32]
    gen = torch.Generator().manual_seed(9)
    slots, cot = torch.randn(B, K, D, generator=gen), torch.randn(B, 32, generator=gen)
    ps = rn_params(D, g_dims, f_dims, seed=3)
    out, ds, _ = run_abi(slots, ps, g_dims, f_dims, cot)
    worst = 0.0
    for b in range(B):
        o1, d1, _ = run_abi(slots[b:b + 1], ps, g_dims, f_dims, cot[b:b + 1])
        worst = max(worst, relerr(out[b], o1[0], floor=1e-6), relerr(ds[b], d1[0], floor=1e-6))
    log(f"[rn images independent] worst {worst:.2e}")
    assert worst < 1e-5


def test_rn_rejects_bad_shapes():
    lib, L = _lib()
    x = torch.zeros(64, device="cuda")
    gd, fd = (ctypes.c_int * 1)(64), (ctypes.c_int * 1)(64)
    arr = (ctypes.c_void_p * 4)(*[x.data_ptr()] * 4)
    assert L.ocrl_pool_rn_fwd(lib.ptr(x), arr, lib.ptr(x), 1, 1, 4, 1, gd, 1, fd, lib.ptr(x), 64, None) != 0
    assert b"num_slots" in L.ocrl_last_error()
    assert L.ocrl_pool_rn_fwd(lib.ptr(x), arr, lib.ptr(x), 1, 2, 4, 1, gd, 1, fd, lib.ptr(x), 8, None) != 0
    assert b"workspace" in L.ocrl_last_error()


def test_rn_module_adam_step_matches_fp64():
    from ocrl_amd import poolings
    B, K, D = 32, 6, 192
    m = poolings.RN_Module(D, K, 1, types.SimpleNamespace(**RN_DEFAULT)).cuda()
    gen = torch.Generator().manual_seed(4)
    slots, cot = torch.randn(B, K, D, generator=gen), torch.randn(B, 64, generator=gen)
    before = [p.detach().cpu().clone() for p in m._param_list()]
    _, _, r_dw = ref_grads(slots, before, len(RN_DEFAULT["g_dims"]), cot)
    lr = 1e-3
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    opt.zero_grad()
    (m(slots.cuda()) * cot.cuda()).sum().backward()
    opt.step()
    p64 = [p.double().requires_grad_(True) for p in before]
    opt64 = torch.optim.Adam(p64, lr=lr)
    for p, g in zip(p64, r_dw):
        p.grad = g
    opt64.step()
    gmax = max(g.abs().max().item() for g in r_dw)
    for p, want, g in zip(m._param_list(), p64, r_dw):
        got = p.detach().cpu().double()
        big = g.abs() > 1e-3 * gmax                               # gradients whose sign is not rounding noise
        assert (got - want.detach())[big].abs().max() <= 1e-3 * lr
        assert (got - want.detach()).abs().max() <= 2.001 * lr


def _pool_cfg(name, **over):
    c = types.SimpleNamespace(name=name, learn_aux_loss=False, learn_downstream_loss=False,
                              ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=""))
    if name == "RN":
        c.g_dims, c.f_dims, c.learning = RN_DEFAULT["g_dims"], RN_DEFAULT["f_dims"], types.SimpleNamespace(lr=1e-4)
    elif name == "MLP":
        c.dims, c.acts, c.learning = [128, 128], ["relu", "relu"], types.SimpleNamespace(lr=1e-4)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _ocr_cfg():
    from ocrl_amd.utils.config import compose
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return compose(os.path.join(root, "configs"), "train_ocr", ["ocr=slate", "ocr.slotattr.num_slots=5", "ocr.dvae.vocab_size=256",
                                                                "ocr.tfdec.num_dec_blocks=1", "dataset=random-N5C4S4S2", "dataset.obs_size=32"])


@pytest.mark.parametrize("name", ["RN", "MLP", "Identity"])
def test_heads_over_the_encoder_and_in_the_extractor(name):
    """poolings.<name>(ocr, config) in eval mode, learn_downstream_loss through the head into the encoder, and OCRExtractor"""
    from ocrl_amd import ocrs, poolings
    from ocrl_amd.sb3s import OCRExtractor
    ocr_cfg = _ocr_cfg()
    torch.manual_seed(11)
    ocr = ocrs.SLATE(ocr_cfg.ocr, ocr_cfg.dataset)
    ocr.to("cuda:0")
    pool = poolings.RN(ocr, 1, _pool_cfg(name)) if name == "RN" else getattr(poolings, name)(ocr, _pool_cfg(name))
    pool.to("cuda:0")
    pool.eval()
    want_dim = {"RN": 64, "MLP": 128, "Identity": 5 * ocr.rep_dim}[name]
    obs = torch.rand(4, 3, 32, 32, device="cuda")
    v = pool(obs)
    assert pool.rep_dim == want_dim and v.shape == (4, want_dim) and torch.isfinite(v).all()
    slots = ocr(obs)                                                # fresh slot noise per call: pool the same slots on both sides
    v = pool._module(slots)
    assert torch.equal(v, pool._module(slots))
    if name == "RN":
        assert relerr(v, rn_ref64(slots.double(), [p.detach().double() for p in pool._module._param_list()], 4)) < 1e-4
    elif name == "Identity":
        assert torch.equal(v, slots.flatten(1))
    # learn_downstream_loss: d loss / d slots reaches ocrl_slate_encode_backward
    ocr2 = ocrs.SLATE(ocr_cfg.ocr, ocr_cfg.dataset)
    ocr2.to("cuda:0")
    cfg = _pool_cfg(name, learn_downstream_loss=True)
    pool2 = poolings.RN(ocr2, 1, cfg) if name == "RN" else getattr(poolings, name)(ocr2, cfg)
    pool2.to("cuda:0")
    pool2.eval()
    pool2.set_zero_grad()
    v2 = pool2(obs)
    assert v2.requires_grad
    v2.square().sum().backward()
    torch.cuda.synchronize()
    eng = ocr2._module.engine
    enc = [p for p in eng.params if p.name.startswith(("_enc.", "_enc_pos.", "_slotattn."))]
    g = torch.cat([eng.view(eng.flat_g, p).flatten() for p in enc])
    assert torch.isfinite(g).all() and g.abs().max().item() > 0
    # the extractor owns the encoder module (no checkpoint): the RL loss trains it through the head
    full = types.SimpleNamespace(ocr=ocr_cfg.ocr, env=ocr_cfg.dataset, pooling=_pool_cfg(name), num_envs=4, device="cuda:0")
    ex = OCRExtractor(None, full).to("cuda:0")
    ex.train()
    assert ex.features_dim == want_dim
    f = ex(obs)
    assert f.shape == (4, want_dim) and f.requires_grad
    f.square().sum().backward()
    grads = [p.grad for n, p in ex.named_parameters() if n.startswith("_ocr._enc.") and p.grad is not None]
    assert grads and all(torch.isfinite(t).all() for t in grads) and max(t.abs().max().item() for t in grads) > 0
    ex.eval()
    with torch.no_grad():
        assert torch.isfinite(ex(obs)).all()
