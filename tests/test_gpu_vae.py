"""GPU checks of the VAE module (ocrl_vae_*): forward outputs, metrics and every parameter gradient against the fp64 restatement of the
reference's loss (tests/golden/make_golden_vae.py: ref_loss) and its fixtures, at 64 x 64 (n = 4), 32 x 32 (n = 3), use_cnn_feat and
kld_weight 5, up to B = 256; both cotangents (loss and rep); the encoder-only path; bitwise repeatability and NaN-prefilled buffers;
accumulation; an Adam step; the extractor with the MLP and Transformer heads; train_ocr.py ocr=vae; rejection before any launch."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.golden import make_golden_vae as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ocrs():
    from ocrl_amd import ocrs
    return ocrs


def _module(tag, S=None, **kw):
    S = S or G.CASES[tag][0]
    m = _ocrs().VAE_Module(G.config(tag, **kw), G.env_config(S))
    G.load_closed_form(m)
    return m.to(DEV)


def _inputs(m, B, seed):
    obs = G.observations(B, m._obs_size, seed)
    eps = G.noise(B, m._latent_dim, seed)
    return obs, eps


def _ref(m, obs, eps):
    ps = [p.detach().double().cpu().requires_grad_(True) for p in m.parameters()]
    r = G.ref_loss(obs, ps, eps, m._n, m._cnn_feat_size, m._kld_weight, m._use_cnn_feat)
    return r, ps


def _relerr(a, b, floor):
    return ((a.double().cpu() - b.double()).abs().max() / max(b.abs().max().item(), floor)).item()


def _normerr(a, b):
    """norm-wise relative error: the latent-side gradients are sums of many cancelling terms, so single entries carry fp32 noise"""
    b = b.double()
    return ((a.double().cpu() - b).norm() / max(b.norm().item(), 1e-30)).item()


# Fixed bounds on the norm-wise gradient error against fp64, per case: about twice the worst parameter measured once on an MI355X
# (the HIP path is bitwise deterministic, so one code state always gives the same verdict).  With the closed-form weights the
# reconstruction error is large (mse ~ 4400 at 64 x 64), so the gradients upstream of the latent (_in_dec, _dec._decoder.0/1) are
# small differences of large decoder terms and their fp32 error grows with B: worst measured 6.4e-3 at B = 64 and 8.9e-3 at B = 256
# (plain torch fp32 is 1.7e-3 off fp64 on _in_dec.weight at B = 64).  Small batches stay below 2.4e-5.  A layout or missing-term
# error is O(1).
GRAD_TOL = {("default", 5): 1e-4, ("default", 64): 1.5e-2, ("s32", 24): 1e-4, ("cnnfeat_kld5", 7): 2e-3, ("s32", 256): 4e-3,
            ("default", 256): 2e-2}


def _check(m, B, seed, with_rep_cot=True, tol=2e-4, gtol=1e-3):
    obs, eps = _inputs(m, B, seed)
    r, ps = _ref(m, obs, eps)
    cot = G.cotangent(tuple(r["rep"].shape), seed)
    (r["loss"] + ((r["rep"] * cot).sum() if with_rep_cot else 0)).backward()
    m.zero_grad(set_to_none=True)
    loss, mse, kld, rep = m.loss_terms(obs.float().to(DEV), eps.float().to(DEV))
    (loss + ((rep * cot.float().to(DEV)).sum() if with_rep_cot else 0)).backward()
    for got, want in ((loss, r["loss"]), (mse, r["mse"]), (kld, r["kld"])):
        assert abs(got.item() - want.item()) <= tol * max(abs(want.item()), 1e-3), (got.item(), want.item())
    assert _relerr(rep, r["rep"].detach(), 1e-3) < tol
    for (n, p), q in zip(m.named_parameters(), ps):
        assert p.grad is not None, n
        assert _normerr(p.grad, q.grad) < gtol, (n, _normerr(p.grad, q.grad))
    return r


@pytest.mark.parametrize("tag", list(G.CASES))
def test_reference_fixtures(tag):
    S, B, c = G.CASES[tag]
    seed = list(G.CASES).index(tag)
    fx = np.load(G.fixture_path())
    m = _module(tag)
    obs, eps = _inputs(m, B, seed)
    loss, mse, kld, rep = m.loss_terms(obs.float().to(DEV), eps.float().to(DEV))
    cot = G.cotangent(tuple(rep.shape), seed)
    (loss + (rep * cot.float().to(DEV)).sum()).backward()
    want = fx[tag + "/loss"]
    got = np.array([loss.item(), mse.item(), -kld.item()])
    assert np.allclose(got, want, rtol=2e-4, atol=1e-5), (got, want)
    if not c["use_cnn_feat"]:
        assert np.abs(rep.detach().cpu().numpy() - fx[tag + "/mu"]).max() <= 2e-4 * max(np.abs(fx[tag + "/mu"]).max(), 1e-3)
    r = rep.detach().cpu().double().numpy().ravel()
    rs = fx[tag + "/rep_sample"]
    assert np.abs(r[G.sample_idx(r.size)] - rs).max() <= 2e-4 * np.abs(rs).max()
    recon = m.reconstruct(obs.float().to(DEV), eps.float().to(DEV)).cpu().double().numpy().ravel()
    assert np.allclose(G.moments(recon)[:3], fx[tag + "/recon_moments"][:3], rtol=1e-4)
    for n, p in m.named_parameters():
        g = p.grad.detach().cpu().double().numpy().ravel()
        if tag + "/grad/" + n in fx:
            w = fx[tag + "/grad/" + n]
            assert np.abs(g - w).max() <= 2e-3 * max(np.abs(w).max(), 1e-6), n
        else:
            w = fx[tag + "/grads/" + n]
            gm = G.moments(g)
            assert np.abs(g[G.sample_idx(g.size)] - w).max() <= 2e-3 * max(np.abs(w).max(), 1e-6), n
            assert abs(gm[2] - fx[tag + "/gradm/" + n][2]) <= 4e-3 * fx[tag + "/gradm/" + n][2], n


@pytest.mark.parametrize("tag,B", [("default", 5), ("default", 64), ("s32", 24), ("cnnfeat_kld5", 7), ("s32", 256)])
def test_against_fp64(tag, B):
    _check(_module(tag), B, 10 + B, gtol=GRAD_TOL[tag, B])


def test_b256_at_64x64_against_fp64():
    _check(_module("default"), 256, 3, tol=5e-4, gtol=GRAD_TOL["default", 256])


def test_loss_cotangent_only_and_scaled_loss():
    m = _module("default")
    _check(m, 4, 21, with_rep_cot=False)
    obs, eps = _inputs(m, 4, 22)
    o, e = obs.float().to(DEV), eps.float().to(DEV)
    m.zero_grad(set_to_none=True)
    m.loss_terms(o, e)[0].backward()
    g1 = [p.grad.clone() for p in m.parameters()]
    m.zero_grad(set_to_none=True)
    (2.0 * m.loss_terms(o, e)[0]).backward()
    for a, p in zip(g1, m.parameters()):
        assert torch.allclose(2 * a, p.grad, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("cnn", [False, True])
def test_encoder_path_equals_get_loss_rep(cnn):
    m = _module("default", use_cnn_feat=cnn)
    obs, eps = _inputs(m, 6, 30)
    o = obs.float().to(DEV)
    _, rep = m.get_loss(o, with_rep=True, eps=eps.float().to(DEV))
    enc = m(o)
    assert torch.equal(enc, rep)
    r, ps = _ref(m, obs, eps)
    assert _relerr(enc, r["rep"].detach(), 1e-3) < 2e-4
    if cnn:
        assert enc.shape == (6, 16, 64)
        e = r["rep"].detach()
        # img_to_slot: token t = (h, w) of the [B, 64, f, f] map
        assert _relerr(enc[:, 5], e[:, 5], 1e-3) < 2e-4
    # backward of the encoder path from d rep alone
    cot = G.cotangent(tuple(enc.shape), 31)
    m.zero_grad(set_to_none=True)
    (m(o) * cot.float().to(DEV)).sum().backward()
    (r["rep"] * cot).sum().backward()
    for (n, p), q in zip(m.named_parameters(), ps):
        if q.grad is None or q.grad.abs().max() == 0:
            assert p.grad is None or p.grad.abs().max() == 0, n
            continue
        assert _normerr(p.grad, q.grad) < 1e-3, n


@pytest.mark.parametrize("cnn", [False, True])
def test_rep_cotangent_alone_through_get_loss(cnn):
    """backward from rep alone: the loss's cotangent is absent and counts as zero (no decoder or KL gradient)"""
    m = _module("cnnfeat_kld5", use_cnn_feat=cnn)
    obs, eps = _inputs(m, 5, 35)
    r, ps = _ref(m, obs, eps)
    cot = G.cotangent(tuple(r["rep"].shape), 35)
    (r["rep"] * cot).sum().backward()
    m.zero_grad(set_to_none=True)
    _, rep = m.get_loss(obs.float().to(DEV), with_rep=True, eps=eps.float().to(DEV))
    (rep * cot.float().to(DEV)).sum().backward()
    for (n, p), q in zip(m.named_parameters(), ps):
        if q.grad is None:
            assert p.grad is None or torch.count_nonzero(p.grad) == 0, n
        else:
            assert _normerr(p.grad, q.grad) < 1e-4, (n, _normerr(p.grad, q.grad))
    # a second backward from rep after the loss was backpropagated adds d rep's share only
    m.zero_grad(set_to_none=True)
    loss, _, _, rep = m.loss_terms(obs.float().to(DEV), eps.float().to(DEV))
    loss.backward(retain_graph=True)
    g_loss = [p.grad.clone() for p in m.parameters()]
    (rep * cot.float().to(DEV)).sum().backward()
    for (n, p), a, q in zip(m.named_parameters(), g_loss, ps):
        d = (p.grad - a)
        if q.grad is None:
            assert torch.count_nonzero(d) == 0, n
        else:
            assert _normerr(d, q.grad) < 1e-3, (n, _normerr(d, q.grad))


def _raw_full(m, obs, eps, fill):
    """one forward + backward through the C entry points with every output and the workspace prefilled"""
    from ocrl_amd.ocrs import vae as V
    ps = [p.detach().contiguous() for p in m.parameters()]
    dims = m._dims()
    ws = V._ws(obs, dims, True).fill_(fill)
    rep = V._rep_like(obs, dims).fill_(fill)
    met = torch.full((3,), fill, device=DEV)
    from ocrl_amd import _lib
    _lib.check(_lib.lib().ocrl_vae_fwd(_lib.ptr(obs), V._ptrs(ps), _lib.ptr(eps), _lib.ptr(rep), _lib.ptr(met), None, obs.shape[0], *dims[:5],
                                       float(dims[5]), 1, _lib.ptr(ws), ws.numel(), _lib.stream()))
    gs = [torch.full_like(p, fill) for p in ps]
    drep = torch.ones_like(rep) * 0.01
    dloss = torch.ones(1, device=DEV)
    _lib.check(_lib.lib().ocrl_vae_bwd(_lib.ptr(obs), _lib.ptr(eps), V._ptrs(ps), _lib.ptr(dloss), _lib.ptr(drep), V._ptrs(gs), obs.shape[0], *dims[:5],
                                       float(dims[5]), 1, _lib.ptr(ws), ws.numel(), _lib.stream()))
    torch.cuda.synchronize()
    return [met, rep] + gs


def test_bitwise_repeatable_and_nan_prefill():
    m = _module("default")
    obs, eps = _inputs(m, 9, 40)
    o, e = obs.float().to(DEV), eps.float().to(DEV)
    a = _raw_full(m, o, e, 0.0)
    b = _raw_full(m, o, e, float("nan"))
    c = _raw_full(m, o, e, 0.0)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.isfinite(x).all()


def test_backward_accumulates_and_no_grad_matches():
    m = _module("s32")
    obs, eps = _inputs(m, 4, 50)
    o, e = obs.float().to(DEV), eps.float().to(DEV)
    m.zero_grad(set_to_none=True)
    m.loss_terms(o, e)[0].backward()
    g1 = [p.grad.clone() for p in m.parameters()]
    m.loss_terms(o, e)[0].backward()
    for a, p in zip(g1, m.parameters()):
        assert torch.equal(p.grad, 2 * a) or torch.allclose(p.grad, 2 * a, rtol=1e-6, atol=0)
    with torch.no_grad():
        l0 = m.loss_terms(o, e)
        r0 = m(o)
    l1 = m.loss_terms(o, e)
    assert torch.equal(l0[0], l1[0].detach()) and torch.equal(r0, m(o).detach())


def test_observation_gradient_and_bad_inputs_raise():
    m = _module("default")
    obs = torch.rand(2, 3, 64, 64, device=DEV)
    with pytest.raises(RuntimeError):
        m(obs.clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        m(obs.cpu())
    with pytest.raises(ValueError):
        m(torch.rand(2, 4, 64, 64, device=DEV))
    with pytest.raises(ValueError):
        m(torch.rand(2, 3, 32, 32, device=DEV))
    with pytest.raises(ValueError):
        m.loss_terms(obs, torch.zeros(2, 7, device=DEV))
    m2 = _module("default")
    m2._mu.weight = torch.nn.Parameter(torch.zeros(128, 1024, device=DEV))       # a wrong shape never reaches the kernels
    with pytest.raises(ValueError):
        m2(obs)
    with pytest.raises(ValueError):
        m2.loss_terms(obs)
    m2 = _module("default")
    m2._dec._decoder[1].m.weight = torch.nn.Parameter(torch.zeros(64, 64, 1, 1, device=DEV))
    with pytest.raises(ValueError):
        m2.loss_terms(obs)
    with torch.no_grad():
        m._mu.weight.data = m._mu.weight.data.double()
    with pytest.raises(RuntimeError):
        m(obs)
    with pytest.raises(ValueError):
        _ocrs().VAE_Module(G.config("default"), G.env_config(48))
    from ocrl_amd import _lib
    assert _lib.lib().ocrl_vae_ws_floats(2, 48, 3, 4, 256, 0, 1) == 0


def test_update_matches_fp64_adam():
    ocfg = G.config("default")
    ocfg.learning.lr = 1e-3
    w = _ocrs().VAE(ocfg, G.env_config(64))
    G.load_closed_form(w._module)
    w.to(DEV)
    obs, eps = _inputs(w._module, 4, 60)
    before = [p.detach().double().cpu().clone() for p in w._module.parameters()]
    r, ps = _ref(w._module, obs, eps)
    r["loss"].backward()
    w._module.draw_eps = lambda o: eps.float().to(DEV)
    metrics = w.update(obs.float().to(DEV), None, 0)
    assert abs(metrics["loss"].item() - r["loss"].item()) <= 2e-4 * r["loss"].item()
    assert abs(metrics["kld"].item() + r["kld"].item()) <= 2e-4 * abs(r["kld"].item()) + 1e-6
    lr = 1e-3
    for (n, p), b, q in zip(w._module.named_parameters(), before, ps):
        g = q.grad
        want = b - lr * g / (g.abs() + 1e-8)                    # Adam's first step: m_hat / (sqrt(v_hat) + eps) = g / (|g| + eps)
        ok = (g.abs() > 1e-4 * g.abs().max()).double()             # tiny gradients: sign is fp32-noise
        err = ((p.detach().double().cpu() - want).abs() * ok).max().item()
        assert err <= 1e-2 * lr, (n, err)


def _rl_config(ocr, pooling, checkpoint="", finetuning=False):
    p = types.SimpleNamespace(name=pooling, learn_aux_loss=False, learn_downstream_loss=False,
                              ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=checkpoint, finetuning=finetuning))
    if pooling == "Transformer":
        for k, v in dict(rep_dim=128, d_model=128, nhead=8, num_layers=1, pos_emb="None", norm_first=False, use_mlp1=False, use_mlp2=False,
                         cw_embedding=False, push_embedding=False).items():
            setattr(p, k, v)
    else:
        p.dims, p.acts = [64], ["relu"]
    return types.SimpleNamespace(ocr=ocr, env=types.SimpleNamespace(obs_size=64, obs_channels=3), pooling=p, num_envs=4, device=DEV)


@pytest.mark.parametrize("pooling,cnn", [("MLP", False), ("Transformer", True)])
@pytest.mark.parametrize("finetune", [False, True])
def test_extractor_with_vae(tmp_path, pooling, cnn, finetune):
    from ocrl_amd.sb3s import OCRExtractor
    ocfg = G.config("cnnfeat_kld5" if cnn else "default")
    w = _ocrs().VAE(ocfg, G.env_config(64))
    path = str(tmp_path / "vae.pth")
    torch.save(w.save(), path)
    ex = OCRExtractor(None, _rl_config(ocfg, pooling, path, finetune)).to(DEV)
    obs = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(70)).to(DEV)
    out = ex(obs)
    assert torch.isfinite(out).all()
    out.square().sum().backward()
    enc = ex._ocr._module if hasattr(ex._ocr, "_module") else ex._ocr
    g = enc._enc._encoder[0].m.weight.grad
    if finetune:
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    else:
        assert g is None
        w.to(DEV)
        with torch.no_grad():
            rep = w(obs)
        assert rep.shape == ((8, 16, 64) if cnn else (8, 256))


def test_learn_aux_and_downstream_loss_through_mlp():
    from ocrl_amd import poolings
    w = _ocrs().VAE(G.config("default"), G.env_config(64))
    pcfg = types.SimpleNamespace(name="MLP", dims=[64], acts=["relu"], learn_aux_loss=True, learn_downstream_loss=True,
                                 ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=""), learning=types.SimpleNamespace(lr=1e-3))
    p = poolings.MLP(w, pcfg)
    p.to(DEV)
    p.set_zero_grad()
    obs = torch.rand(6, 3, 64, 64, generator=torch.Generator().manual_seed(71)).to(DEV)
    metrics, state = w.get_loss(obs, with_rep=True)
    (metrics["loss"] + state.square().sum()).backward()
    g = w._module._dec._decoder[1].m.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    g = w._module._enc._encoder[0].m.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0


def test_train_ocr_vae_runs(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "train_ocr.py"), "ocr=vae", "dataset=random-N5C4S4S2", f"run_dir={tmp_path}", "max_steps=3",
           "log_interval=1", "batch_size=8", "num_workers=0", "eval_interval=2", "dataset.synthetic_train=64", "dataset.synthetic_val=8"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "checkpoints" / "model_latest.pth").exists() or any(tmp_path.rglob("model_latest.pth"))
