"""GPU checks of the NatureCNN pooling heads: ocrl_pool_cnn_fwd/_bwd against the fp64 restatement of tests/pool_cnn_ref.py (with and
without the token gradient), the channels-last first layer against the generic ocrl_naturecnn_fwd on the NCHW permute, the ABI contract
(every output written, uncovered border pixels get a zero gradient, reproducibility, a NULL dtokens leaves dw unchanged, independent
images, argument messages), the reference fixtures straight against the HIP path, and the Python surface (modules train with Adam, a
leaf token tensor gets its gradient, OCRExtractor and the poolings.CNN_Linear wrapper over a frozen SLATE use_cnn_feat checkpoint).
Tolerances: the CNN stack's from tests/test_gpu_naturecnn.py (1e-5 / 5e-5), the transformer head's from tests/test_gpu_pooling_long.py
(2e-5 / 3e-4 with its floors)."""
import os
import types

import numpy as np
import pytest
import torch

from tests import pool_cnn_ref as R
from tests.golden import make_golden_pooling_cnn as G
from tests.gpu_util import log, relerr

pytestmark = pytest.mark.gpu


def _map(s):
    for k, st in ((8, 4), (4, 2), (3, 1)):
        s = (s - k) // st + 1
    return s


def grid_weights(D, S, rep, seed):
    """about a quarter of every weight's entries +-1/4, the rest 0; biases in {-1/8, 0, 1/8} (tests/test_gpu_naturecnn.py grid_params).
    With tokens in {0, 1/2, 1} each layer's pre-activations sit on a grid of 2^-3 times the previous one, so fp32 computes the
    forward exactly as long as the sums stay below 2^24 grid steps -- which test_abi_against_fp64 asserts instead of assuming (K = 64 D here)"""
    g = torch.Generator().manual_seed(seed)
    shapes, c = [], D
    for cout, k in ((32, 8), (64, 4), (64, 3)):
        shapes += [(cout, c, k, k), (cout,)]
        c = cout
    if rep:
        o = _map(S)
        shapes += [(rep, 64 * o * o), (rep,)]
    ws = []
    for sh in shapes:
        if len(sh) > 1:
            ws.append(torch.randint(-1, 2, sh, generator=g).float() * (torch.rand(sh, generator=g) < 0.25).float() * 0.25)
        else:
            ws.append(torch.randint(-1, 2, sh, generator=g).float() * 0.125)
    return ws


def grid_tokens(B, S, D, seed):
    return torch.randint(0, 3, (B, S * S, D), generator=torch.Generator().manual_seed(seed)).float() * 0.5


def raw(tokens, S, rep, ps, dout, want_dt=True, fill=float("nan")):
    """one saving ocrl_pool_cnn_fwd + _bwd with every output, the workspace and every gradient buffer prefilled with `fill`"""
    from ocrl_amd import _lib as lib
    L = lib.lib()
    B, _, D = tokens.shape
    n = L.ocrl_pool_cnn_ws_floats(B, S, S, D, rep)
    assert n > 0, L.ocrl_last_error().decode()
    ws = torch.full((n,), fill, device="cuda")
    o = _map(S)
    out = torch.full((B, rep) if rep else (B, o * o, 64), fill, device="cuda")
    gs = [torch.full_like(p, fill) for p in ps]
    dt = torch.full_like(tokens, fill) if want_dt else None
    st = lib.stream()
    lib.check(L.ocrl_pool_cnn_fwd(lib.ptr(tokens), lib.ptrs(ps), lib.ptr(out), B, S, S, D, rep, 1, lib.ptr(ws), n, st))
    if dout is not None:
        lib.check(L.ocrl_pool_cnn_bwd(lib.ptr(tokens), lib.ptr(dout), lib.ptrs(ps), lib.ptr(dt), lib.ptrs(gs), B, S, S, D, rep, lib.ptr(ws), n, st))
    torch.cuda.synchronize()
    return out, gs, dt


def ref64(tokens, ws, rep, cot):
    leaves = [w.double().requires_grad_(True) for w in ws]
    x = tokens.double().requires_grad_(True)
    out = R.cnn(x, leaves, rep)
    (out * cot.double()).sum().backward()
    return out.detach(), [l.grad for l in leaves], x.grad


# (D, map side, batch, rep_dim): every D in {3, 64, 67, 134}, every map in {36, 64, 84, 128} with rep_dim 0 and 512, every batch in
# {1, 4, 32, 33}; 38 adds a map whose last two rows and columns no window covers, and whose rows are not 16-byte aligned at D = 67
PARITY = [(67, 64, 32, 512), (67, 64, 33, 0), (67, 64, 1, 0), (67, 64, 4, 512), (3, 36, 4, 512), (3, 36, 33, 0), (64, 36, 33, 512),
          (134, 36, 32, 0), (64, 84, 4, 0), (64, 84, 1, 512), (3, 84, 32, 512), (134, 64, 4, 512), (134, 64, 1, 0), (3, 64, 32, 0),
          (64, 64, 33, 512), (67, 128, 4, 0), (67, 128, 1, 512), (3, 128, 32, 0), (134, 128, 1, 512), (64, 128, 4, 512), (67, 38, 4, 0),
          (3, 38, 1, 512)]


@pytest.mark.parametrize("D,S,B,rep", PARITY)
def test_abi_against_fp64(D, S, B, rep):
    seed = D * 1000 + S * 10 + B
    ws = grid_weights(D, S, rep, seed)
    tokens = grid_tokens(B, S, D, seed + 1)
    with torch.no_grad():
        f32 = R.cnn(tokens, ws, rep)
        f64 = R.cnn(tokens.double(), [w.double() for w in ws], rep)
    # the precondition of the comparison, as a condition: fp32 computes this forward exactly, so the fp32 and fp64 ReLU masks agree
    assert torch.equal(f32.double(), f64), "grid inputs do not give an exact fp32 forward; choose another scale or seed"
    cot = torch.randn(f64.shape, generator=torch.Generator().manual_seed(seed + 2))
    want, wg, wdt = ref64(tokens, ws, rep, cot)
    ps = [w.cuda() for w in ws]
    out, gs, dt = raw(tokens.cuda(), S, rep, ps, cot.cuda(), want_dt=True)
    assert torch.equal(out.cpu().double(), want), "the HIP forward is exact on grid inputs"
    e_out = relerr(out, want)
    errs = [relerr(g, w) for g, w in zip(gs, wg)]
    e_dt = relerr(dt, wdt)
    log(f"[pool cnn D{D} S{S} B{B} rep{rep}] out {e_out:.2e} grads worst {max(errs):.2e} dtokens {e_dt:.2e}")
    assert e_out <= 1e-5
    for e, w in zip(errs, wg):
        assert w.abs().max() > 0 and e <= 5e-5, errs
    assert wdt.abs().max() > 0 and e_dt <= 5e-5
    # detached tokens: the same weight gradients, bit for bit
    out2, gs2, _ = raw(tokens.cuda(), S, rep, ps, cot.cuda(), want_dt=False)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(gs, gs2))


def _generic(tokens, S, ps):
    """the generic NatureCNN path over the NCHW permute of the same tokens (cin = D, use_cnn_feat): the map as tokens"""
    from ocrl_amd import _lib as lib
    L = lib.lib()
    B, _, D = tokens.shape
    obs = tokens.reshape(B, S, S, D).permute(0, 3, 1, 2).contiguous()
    n = L.ocrl_naturecnn_ws_floats(B, S, S, D, 1, 4, 1, 0)
    assert n > 0
    ws = torch.empty(n, device="cuda")
    o = _map(S)
    out = torch.empty(B, o * o, 64, device="cuda")
    lib.check(L.ocrl_naturecnn_fwd(lib.ptr(obs), lib.ptrs(ps), lib.ptr(out), B, S, S, D, 1, 4, 1, 0, 0, lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D,S,B", [(67, 64, 4), (3, 36, 5), (134, 84, 2), (64, 128, 1), (67, 38, 3)])
def test_first_layer_agrees_with_generic_path(D, S, B):
    ws = grid_weights(D, S, 0, 7 + D)
    tokens = grid_tokens(B, S, D, 8 + D).cuda()
    ps = [w.cuda() for w in ws]
    assert torch.equal(raw(tokens, S, 0, ps, None)[0], _generic(tokens, S, ps)), "grid inputs: bit for bit"
    g = torch.Generator().manual_seed(9 + D)
    ps = [(torch.randn(w.shape, generator=g) * (1.0 / np.sqrt(max(1, w[0].numel())))).cuda() for w in ws]
    tokens = torch.randn(B, S * S, D, generator=g).cuda()
    a, b = raw(tokens, S, 0, ps, None)[0], _generic(tokens, S, ps)
    assert b.abs().max() > 0 and relerr(a, b) <= 1e-5


@pytest.mark.parametrize("D,S,rep", [(67, 64, 512), (67, 38, 0), (3, 84, 0), (134, 36, 512)])
def test_contract_nan_prefill_border_repeat_and_null_dtokens(D, S, rep):
    B = 3
    ws = grid_weights(D, S, rep, 21)
    ps = [w.cuda() for w in ws]
    tokens = grid_tokens(B, S, D, 22).cuda()
    o = _map(S)
    dout = torch.randn((B, rep) if rep else (B, o * o, 64), generator=torch.Generator().manual_seed(23)).cuda()
    out, gs, dt = raw(tokens, S, rep, ps, dout)
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in gs) and torch.isfinite(dt).all()
    covered = 4 * ((S - 8) // 4) + 8                     # rows / columns below this are inside some window
    img = dt.reshape(B, S, S, D)
    if covered < S:
        assert (img[:, covered:] == 0).all() and (img[:, :, covered:] == 0).all()
    assert img[:, :covered, :covered].abs().max() > 0
    out2, gs2, dt2 = raw(tokens, S, rep, ps, dout, fill=0.0)
    assert torch.equal(out, out2) and torch.equal(dt, dt2) and all(torch.equal(a, b) for a, b in zip(gs, gs2))
    out3, gs3, _ = raw(tokens, S, rep, ps, dout, want_dt=False)
    assert torch.equal(out, out3) and all(torch.equal(a, b) for a, b in zip(gs, gs3))


def test_images_are_independent():
    D, S, B = 67, 64, 6
    ps = [w.cuda() for w in grid_weights(D, S, 512, 31)]
    tokens = grid_tokens(B, S, D, 32).cuda()
    dout = torch.randn(B, 512, generator=torch.Generator().manual_seed(33)).cuda()
    a, _, da = raw(tokens, S, 512, ps, dout)
    t2 = tokens.clone()
    t2[3] = 1.0 - t2[3]
    b, _, db = raw(t2, S, 512, ps, dout)
    keep = [i for i in range(B) if i != 3]
    assert torch.equal(a[keep], b[keep]) and not torch.equal(a[3], b[3])
    assert torch.equal(da[keep], db[keep])


def test_bad_arguments():
    from ocrl_amd import _lib as lib
    L = lib.lib()
    x = torch.zeros(8, device="cuda")
    arr = lib.ptrs([x] * 8)
    for args, msg in [((0, 64, 64, 67, 512), "batch >= 1"), ((2, 64, 64, 0, 512), "token width >= 1"), ((2, 35, 64, 67, 0), "at least 36 x 36"),
                      ((2, 64, 32, 67, 0), "at least 36 x 36"), ((2, 64, 64, 67, 6), "multiple of 4"), ((2, 64, 64, 67, -4), "multiple of 4"),
                      ((40000, 128, 128, 67, 0), "int32")]:
        assert L.ocrl_pool_cnn_ws_floats(*args) == 0
        assert L.ocrl_pool_cnn_fwd(lib.ptr(x), arr, lib.ptr(x), *args, 1, lib.ptr(x), 8, lib.stream()) != 0
        assert msg in L.ocrl_last_error().decode(), (args, L.ocrl_last_error().decode())
        assert L.ocrl_pool_cnn_bwd(lib.ptr(x), lib.ptr(x), arr, None, arr, *args, lib.ptr(x), 8, lib.stream()) != 0
        assert msg in L.ocrl_last_error().decode()
    assert L.ocrl_pool_cnn_fwd(lib.ptr(x), arr, lib.ptr(x), 2, 64, 64, 67, 512, 1, lib.ptr(x), 8, lib.stream()) != 0
    assert "workspace too small" in L.ocrl_last_error().decode()
    assert L.ocrl_pool_cnn_fwd(None, arr, lib.ptr(x), 2, 64, 64, 67, 512, 1, lib.ptr(x), 8, lib.stream()) != 0
    assert "null argument" in L.ocrl_last_error().decode()


def _module(tag):
    from ocrl_amd import poolings
    head, S, D, _, _ = G.CASES[tag]
    m = getattr(poolings, head + "_Module")(D, S * S, G.config(tag))
    m.load_state_dict(G.weights(m, tag))
    return m.cuda().eval()


@pytest.mark.parametrize("tag", list(G.CASES))
def test_reference_fixtures(tag):
    fx = np.load(G.FIXTURE)
    m = _module(tag)
    x = G.tokens(tag).cuda().requires_grad_(True)
    out = m(x)
    want = fx[tag + ":out"]
    (out * G.cotangent(tag, out.shape).cuda()).sum().backward()
    linear = G.CASES[tag][0] == "CNN_Linear"
    tol_out, tol_g = (1e-5, 5e-5) if linear else (2e-5, 3e-4)
    e_out = np.abs(out.detach().cpu().numpy() - want).max() / np.abs(want).max()
    named = dict(m.named_parameters())
    keys = [k for k in fx.files if k.startswith(tag + ":g:")]
    assert len(keys) == len(named)
    gmax = max(np.abs(fx[k] if fx[k].shape == tuple(named[k.split(":g:")[1]].shape) else fx[k][3:]).max() for k in keys)
    worst = 0.0
    for k in keys + [tag + ":dtokens"]:
        t = x.grad if k.endswith(":dtokens") else named[k.split(":g:")[1]].grad
        w = fx[k]
        if w.shape == tuple(t.shape):
            got = t.detach().cpu().numpy()
        else:
            got, w = G.sample(t)[3:], w[3:]
        floor = 0.0 if linear or k.endswith(":dtokens") else 1e-3 * gmax
        worst = max(worst, np.abs(got - w).max() / max(np.abs(w).max(), floor, 1e-30))
    log(f"[pool cnn fixture {tag}] out {e_out:.2e} grads worst {worst:.2e}")
    assert e_out <= tol_out and worst <= tol_g


@pytest.mark.parametrize("tag", list(G.CASES))
def test_modules_against_fp64_with_a_leaf_token_gradient(tag):
    head, S, D, B, _ = G.CASES[tag]
    m = _module(tag)
    x = G.tokens(tag)
    if head == "CNN_Linear":
        # the CNN stack's fp64 bound (1e-5 of the output's maximum) is set for inputs on which fp32 is exact, as in test_abi_against_fp64:
        # on the fixture's continuous inputs the K = 4288 fp32 sums alone round by about that much (measured: 1.2e-5)
        with torch.no_grad():
            for p, w in zip(m._net.param_list(), grid_weights(D, S, m.rep_dim, 51)):
                p.copy_(w)
        x = grid_tokens(B, S, D, 52)
        P = {k: v.cpu() for k, v in m.state_dict().items()}
        with torch.no_grad():
            assert torch.equal(R.forward(P, x, head, G.config(tag)).double(),
                               R.forward({k: v.double() for k, v in P.items()}, x.double(), head, G.config(tag)))
    x = x.cuda().requires_grad_(True)
    out = m(x)
    cot = G.cotangent(tag, out.shape)
    (out * cot.cuda()).sum().backward()
    r_out, r_g, r_dt = R.loss_and_grads(m.state_dict(), x, head, G.config(tag), cot)
    named = dict(m.named_parameters())
    linear = head == "CNN_Linear"
    tol_out, tol_g = (1e-5, 5e-5) if linear else (2e-5, 3e-4)
    gmax = max(v.abs().max().item() for v in r_g.values())
    e_out = relerr(out, r_out)
    e_g = max(relerr(named[n].grad, r_g[n], floor=0.0 if linear else 1e-4 * gmax) for n in r_g)
    e_dt = relerr(x.grad, r_dt)
    log(f"[pool cnn module {tag}] out {e_out:.2e} grads worst {e_g:.2e} dtokens {e_dt:.2e}")
    assert e_out <= tol_out and e_g <= tol_g and e_dt <= tol_g


@pytest.mark.parametrize("head", ["CNN_Linear", "CNN_Transformer"])
def test_modules_train_with_adam(head):
    from ocrl_amd import poolings
    tag = "linear64" if head == "CNN_Linear" else "trans64"
    torch.manual_seed(0)
    m = getattr(poolings, head + "_Module")(67, 4096, G.config(tag)).cuda().train()
    g = torch.Generator().manual_seed(41)
    tokens, target = torch.rand(8, 4096, 67, generator=g).cuda(), torch.randn(8, m.rep_dim, generator=g).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        loss = (m(tokens) - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    log(f"[pool cnn surface {head}] losses {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0], losses
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    with torch.no_grad():
        assert not m(tokens).requires_grad
    with pytest.raises(ValueError, match="square"):
        m(torch.zeros(2, 4095, 67, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 4096, 67))
    if head == "CNN_Linear":
        with pytest.raises(ValueError, match="1024"):
            m(torch.zeros(2, 128 * 128, 67, device="cuda"))


def _pool_cfg(head, **over):
    base = dict(G.CASES["linear64" if head == "CNN_Linear" else "trans64"][4])
    c = types.SimpleNamespace(name=head, learn_aux_loss=False, learn_downstream_loss=False,
                              ocr_checkpoint=types.SimpleNamespace(run_id="", local_file="", finetuning=False), **base)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_slate_cnn_extractor_and_wrapper(tmp_path):
    """SLATE-CNN: ocr=slate ocr.use_cnn_feat=True pooling=cnn_linear / cnn_transformer with a pre-trained (frozen) encoder at 64 x 64"""
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
    obs = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)).cuda()
    for head in ("CNN_Linear", "CNN_Transformer"):
        pcfg = _pool_cfg(head, ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=str(ck), finetuning=False))
        full = types.SimpleNamespace(ocr=ocr_cfg.ocr, env=ocr_cfg.dataset, pooling=pcfg, num_envs=4, device="cuda:0")
        ex = OCRExtractor(None, full).to("cuda:0")
        ex.eval()
        f = ex(obs)
        assert f.shape == (2, ex.features_dim) and torch.isfinite(f).all()
        feat = ex._ocr(obs)
        assert feat.shape == (2, 4096, 67)
        with torch.no_grad():
            want = R.forward({k: t.detach().cpu().double() for k, t in ex._pooling.state_dict().items()}, feat.cpu().double(), head, pcfg)
        e = relerr(f, want)
        log(f"[pool cnn SLATE-CNN extractor {head}] out {e:.2e}")
        assert e <= (1e-5 if head == "CNN_Linear" else 2e-5)
    # the wrapper: save / load round trip; a gradient into the conv encoder stays unsupported
    pcfg = _pool_cfg("CNN_Linear", learning=types.SimpleNamespace(lr=1e-4))
    pool = poolings.CNN_Linear(ocr, pcfg)
    pool.to("cuda:0")
    pool.eval()
    a = pool(obs)
    assert a.shape == (2, 512)
    ckpt = pool.save()
    assert "pooling_module_state_dict" in ckpt and "pooling_opt_state_dict" in ckpt
    other = poolings.CNN_Linear(ocr, pcfg)
    other.to("cuda:0")
    other.load(ckpt)
    other.eval()
    assert torch.equal(other(obs), a)
    for head in ("CNN_Linear", "CNN_Transformer"):
        with pytest.raises(NotImplementedError):
            getattr(poolings, head)(ocr, _pool_cfg(head, learn_downstream_loss=True))
