"""GPU checks of the NatureCNN and MultipleCNN encoders: ocrl_naturecnn_fwd/_bwd against an fp64 restatement (F.conv2d / F.linear in
double on the CPU) and against the reference fixtures, the ABI contract (every output written, reproducibility, independent images,
no_grad == grad mode, accumulation), a torch Adam step, MultipleCNN against separately run NatureCNN modules, and the RL surface
(OCRExtractor trainable and frozen, MultipleCNN + Transformer, learn_downstream_loss through poolings.MLP)."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden.make_golden_naturecnn import CASES, config, cotangent, env_config, fixture_path, load_closed_form, observations, sample

pytestmark = pytest.mark.gpu
CONVS = ((32, 8, 4), (64, 4, 2), (64, 3, 1), (128, 3, 1))
MODES = {                                    # (cnn_feat_size, use_cnn_feat, rep_dim)
    "default": (4, False, 512),
    "feat4": (4, True, 512),
    "feat2": (2, True, 512),
    "size2_flat": (2, False, 64),
}


def _ocrs():
    from ocrl_amd import ocrs
    return ocrs


def _module(mode, S=64, G=None, rep=None):
    feat, use, r = MODES[mode]
    env = types.SimpleNamespace(obs_size=S, obs_channels=3)
    if G is not None:
        return _ocrs().MultipleCNN_Module(types.SimpleNamespace(rep_dim=rep or r, num_modules=G), env).cuda()
    return _ocrs().NatureCNN_Module(types.SimpleNamespace(rep_dim=rep or r, use_cnn_feat=use, cnn_feat_size=feat), env).cuda()


def grid_params(m, seed):
    """every weight: about a quarter of its entries +-1/4, the rest 0; biases in {-1/8, 0, 1/8}.  With observations in {0, 1/2, 1}
    each layer's pre-activations sit on a grid of 2^-3 times the previous one and stay below 2^7 in magnitude, so fp32 computes the whole
    forward exactly: the fp32 and fp64 ReLU masks agree, and the gradients differ by rounding alone"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                v = torch.randint(-1, 2, p.shape, generator=g).float() * (torch.rand(p.shape, generator=g) < 0.25).float() * 0.25
            else:
                v = torch.randint(-1, 2, p.shape, generator=g).float() * 0.125
            p.copy_(v)


def grid_obs(B, S, seed):
    return torch.randint(0, 3, (B, 3, S, S), generator=torch.Generator().manual_seed(seed)).float() * 0.5


def ref64(obs, params, n_conv, use_feat, G=1):
    """fp64 CPU restatement of G modules (params module-major in state_dict order); returns the output with autograd leaves"""
    leaves = [p.detach().cpu().double().requires_grad_(True) for p in params]
    x0 = obs.detach().cpu().double()
    per = 2 * n_conv + (0 if use_feat else 2)
    outs = []
    for g in range(G):
        w = leaves[g * per:(g + 1) * per]
        x = x0
        for l in range(n_conv):
            x = F.relu(F.conv2d(x, w[2 * l], w[2 * l + 1], stride=CONVS[l][2]))
        if use_feat:
            outs.append(x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]))
        else:
            outs.append(F.relu(F.linear(x.flatten(1), w[2 * n_conv], w[2 * n_conv + 1])))
    out = outs[0] if G == 1 else torch.stack(outs, 1)
    return out, leaves


def _check(m, obs, n_conv, use_feat, G=1, seed=0):
    params = m._param_list()
    out = m(obs.cuda())
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    for p in params:
        p.grad = None
    (out * cot.cuda()).sum().backward()
    want, leaves = ref64(obs, params, n_conv, use_feat, G)
    (want * cot.double()).sum().backward()
    assert out.shape == want.shape
    o = out.detach().cpu().double()
    assert (o - want.detach()).abs().max() <= 1e-5 * want.abs().max() + 1e-30
    for p, leaf in zip(params, leaves):
        g = p.grad.detach().cpu().double()
        scale = leaf.grad.abs().max().item()
        assert scale > 0
        assert (g - leaf.grad).abs().max().item() <= 5e-5 * scale


@pytest.mark.parametrize("B", [1, 4, 32, 33, 256])
def test_default_against_fp64(B):
    m = _module("default")
    grid_params(m, 1)
    _check(m, grid_obs(B, 64, B), 3, False, seed=B)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [4, 33])
def test_every_mode_against_fp64(mode, B):
    m = _module(mode)
    grid_params(m, 2)
    feat, use, _ = MODES[mode]
    _check(m, grid_obs(B, 64, 10 + B), 4 if feat == 2 else 3, use, seed=B)


@pytest.mark.parametrize("B", [2, 32])
def test_84x84_against_fp64(B):
    m = _module("default", S=84)
    grid_params(m, 3)
    _check(m, grid_obs(B, 84, 20 + B), 3, False, seed=B)


@pytest.mark.parametrize("B", [4, 32])
def test_multiple_cnn_against_fp64(B):
    m = _module("default", G=5)
    grid_params(m, 4)
    _check(m, grid_obs(B, 64, 30 + B), 3, False, G=5, seed=B)


@pytest.mark.parametrize("tag", list(CASES))
def test_reference_fixtures(tag):
    ocrs = _ocrs()
    m = getattr(ocrs, CASES[tag][0] + "_Module")(config(tag), env_config(tag)).cuda()
    load_closed_form(m)
    fx = np.load(fixture_path(tag))
    out = m(observations(tag).cuda())
    want = fx[tag + ":out"]
    assert out.shape == want.shape
    assert np.abs(out.detach().cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    (out * cotangent(tag, out.shape).cuda()).sum().backward()
    for k, p in m.named_parameters():
        w = fx[tag + ":g:" + k]
        got = p.grad.detach().cpu().numpy() if w.shape == tuple(p.shape) else sample(p.grad)
        if w.shape == tuple(p.shape):
            assert np.abs(got - w).max() <= 5e-5 * np.abs(w).max(), k
        else:                                # moments (sum, sum |.|, sum of squares), then the strided sample
            assert np.abs(got[3:] - w[3:]).max() <= 5e-5 * np.abs(w[3:]).max(), k
            assert abs(got[1] - w[1]) <= 1e-4 * w[1] and abs(got[2] - w[2]) <= 1e-4 * w[2], k


def _raw(m, obs, dout, fill=float("nan")):
    """one ocrl_naturecnn_fwd (saving) + _bwd with every output, workspace and gradient buffer prefilled with `fill`"""
    from ocrl_amd import _lib as lib
    L = lib.lib()
    G = len(m._cnns) if hasattr(m, "_cnns") else 1
    feat, use, rep = (4, 0, m.rep_dim) if G > 1 else (m._cnn_feat_size, int(m._use_cnn_feat), 0 if m._use_cnn_feat else m.rep_dim)
    ps = [p.detach() for p in m._param_list()]
    B, C, H, W = obs.shape
    n = L.ocrl_naturecnn_ws_floats(B, H, W, C, G, feat, use, rep)
    ws = torch.full((n,), fill, device="cuda")
    out = torch.full(dout.shape, fill, device="cuda")
    gs = [torch.full_like(p, fill) for p in ps]
    arr = (ctypes.c_void_p * len(ps))(*[p.data_ptr() for p in ps])
    garr = (ctypes.c_void_p * len(gs))(*[g.data_ptr() for g in gs])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.ocrl_naturecnn_fwd(lib.ptr(obs), arr, lib.ptr(out), B, H, W, C, G, feat, use, rep, 1, lib.ptr(ws), n, st))
    lib.check(L.ocrl_naturecnn_bwd(lib.ptr(obs), lib.ptr(dout), arr, garr, B, H, W, C, G, feat, use, rep, lib.ptr(ws), n, st))
    torch.cuda.synchronize()
    return out, gs


@pytest.mark.parametrize("mode", list(MODES) + ["multi"])
def test_nan_prefill_is_overwritten_and_calls_repeat_bitwise(mode):
    m = _module("default", G=3, rep=32) if mode == "multi" else _module(mode)
    grid_params(m, 5)
    obs = grid_obs(5, 64, 5).cuda()
    shape = m(obs).shape
    dout = torch.randn(shape, generator=torch.Generator().manual_seed(6)).cuda()
    out, gs = _raw(m, obs, dout)
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in gs)
    out2, gs2 = _raw(m, obs, dout, fill=0.0)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(gs, gs2))


def test_images_are_independent():
    m = _module("default", G=2, rep=64)
    grid_params(m, 7)
    obs = grid_obs(6, 64, 7).cuda()
    a = m(obs)
    obs2 = obs.clone()
    obs2[3] = 1.0 - obs2[3]
    b = m(obs2)
    keep = [i for i in range(6) if i != 3]
    assert torch.equal(a[keep], b[keep]) and not torch.equal(a[3], b[3])


def test_no_grad_equals_grad_mode_and_backward_accumulates():
    m = _module("default")
    grid_params(m, 8)
    obs = grid_obs(32, 64, 8).cuda()
    with torch.no_grad():
        a = m(obs)
    b = m(obs)
    assert not a.requires_grad and b.requires_grad and torch.equal(a, b)
    cot = torch.randn(b.shape, generator=torch.Generator().manual_seed(9)).cuda()
    (b * cot).sum().backward()
    one = [p.grad.clone() for p in m.parameters()]
    for p in m.parameters():
        p.grad = None
    (m(obs) * cot).sum().backward()
    (m(obs) * cot).sum().backward()
    assert all(torch.equal(p.grad, 2 * g) for p, g in zip(m.parameters(), one))


def test_observation_gradient_raises():
    m = _module("default")
    with pytest.raises(RuntimeError, match="no gradient"):
        m(torch.zeros(2, 3, 64, 64, device="cuda", requires_grad=True))


def test_wrapper_adam_step_matches_fp64():
    ocrs = _ocrs()
    cfg = types.SimpleNamespace(name="NatureCNN", rep_dim=512, use_cnn_feat=False, cnn_feat_size=4, learning=types.SimpleNamespace(lr=1e-4))
    w = ocrs.NatureCNN(cfg, types.SimpleNamespace(obs_size=64, obs_channels=3))
    w.to("cuda")
    grid_params(w._module, 10)
    before = [p.detach().cpu().double() for p in w._module.parameters()]
    obs = grid_obs(32, 64, 10)
    w.set_zero_grad()
    out = w(obs.cuda())
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(11))
    (out * cot.cuda()).sum().backward()
    want, leaves = ref64(obs, list(w._module.parameters()), 3, False)      # at the weights before the step
    (want * cot.double()).sum().backward()
    w.do_step()
    lr, eps = 1e-4, 1e-8
    for p, p0, leaf in zip(w._module.parameters(), before, leaves):
        step = p0 - lr * leaf.grad / (leaf.grad.abs() + eps)          # Adam's first step: m_hat = g, v_hat = g^2
        got = p.detach().cpu().double()
        big = leaf.grad.abs() > 1e-3 * leaf.grad.abs().max()
        assert (got - step)[big].abs().max() <= 1e-3 * lr
        assert (got - step).abs().max() <= 2.001 * lr


def test_multiple_cnn_equals_separate_modules_bitwise():
    """G = 5 in one call is bitwise equal to five NatureCNN modules run one by one: the fused first layer computes each module's
    channels with the same k order as a lone module, and every other sum depends on the shapes of one module alone"""
    ocrs = _ocrs()
    mm = _module("default", G=5)
    for i, c in enumerate(mm._cnns):
        load_closed_form(c)
        with torch.no_grad():
            for p in c.parameters():
                p.mul_(1.0 + 0.1 * i)
    obs = torch.rand(32, 3, 64, 64, generator=torch.Generator().manual_seed(12)).cuda()
    out = mm(obs)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(13)).cuda()
    (out * cot).sum().backward()
    for i, c in enumerate(mm._cnns):
        single = ocrs.NatureCNN_Module(types.SimpleNamespace(rep_dim=512, use_cnn_feat=False, cnn_feat_size=4),
                                       types.SimpleNamespace(obs_size=64, obs_channels=3)).cuda()
        single.load_state_dict(c.state_dict())
        o = single(obs)
        assert torch.equal(o, out[:, i])
        (o * cot[:, i]).sum().backward()
        for (k, a), b in zip(single.named_parameters(), c.parameters()):
            assert torch.equal(a.grad, b.grad), k


def _rl_config(ocr, pooling, checkpoint=""):
    p = types.SimpleNamespace(name=pooling, learn_aux_loss=False, learn_downstream_loss=False,
                              ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=checkpoint, finetuning=False))
    if pooling == "Transformer":
        for k, v in dict(rep_dim=128, d_model=128, nhead=8, num_layers=1, pos_emb="None", norm_first=False, use_mlp1=False, use_mlp2=False,
                         cw_embedding=False, push_embedding=False).items():
            setattr(p, k, v)
    return types.SimpleNamespace(ocr=ocr, env=types.SimpleNamespace(obs_size=64, obs_channels=3), pooling=p, num_envs=4, device="cuda:0")


NCNN = dict(name="NatureCNN", rep_dim=512, use_cnn_feat=False, cnn_feat_size=4)


def test_extractor_trains_naturecnn_end_to_end():
    from ocrl_amd.sb3s import OCRExtractor
    ex = OCRExtractor(None, _rl_config(types.SimpleNamespace(**NCNN), "Identity")).to("cuda:0")
    obs = torch.rand(32, 3, 64, 64, generator=torch.Generator().manual_seed(14)).cuda()
    out = ex(obs)
    assert out.shape == (32, 512)
    out.square().sum().backward()
    named = [(n, p) for n, p in ex.named_parameters() if n.startswith("_ocr._cnn.")]
    assert len(named) == 6
    for n, p in named:
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n


def test_extractor_freezes_naturecnn_from_a_checkpoint(tmp_path):
    from ocrl_amd.sb3s import OCRExtractor
    ocr_cfg = types.SimpleNamespace(**NCNN)
    w = _ocrs().NatureCNN(ocr_cfg, types.SimpleNamespace(obs_size=64, obs_channels=3))
    path = str(tmp_path / "ocr.pt")
    torch.save(w.save(), path)
    ex = OCRExtractor(None, _rl_config(ocr_cfg, "Identity", path)).to("cuda:0")
    obs = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(15)).cuda()
    out = ex(obs)
    assert not out.requires_grad
    w.to("cuda")
    with torch.no_grad():
        assert torch.equal(out, w(obs))
    assert all(p.grad is None for p in ex._ocr._module.parameters())


def test_multiple_cnn_with_transformer_in_the_extractor():
    from ocrl_amd.sb3s import OCRExtractor
    ex = OCRExtractor(None, _rl_config(types.SimpleNamespace(name="MultipleCNN", rep_dim=512, num_modules=5), "Transformer")).to("cuda:0")
    ex.eval()
    obs = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(16)).cuda()
    out = ex(obs)
    assert out.shape == (8, 128) and torch.isfinite(out).all()
    out.square().sum().backward()
    g = ex._ocr._cnns[4]._cnn[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0


def test_learn_downstream_loss_through_mlp():
    from ocrl_amd import poolings
    w = _ocrs().NatureCNN(types.SimpleNamespace(**NCNN, learning=types.SimpleNamespace(lr=1e-4)), types.SimpleNamespace(obs_size=64, obs_channels=3))
    pcfg = types.SimpleNamespace(name="MLP", dims=[64], acts=["relu"], learn_aux_loss=False, learn_downstream_loss=True,
                                 ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=""), learning=types.SimpleNamespace(lr=1e-3))
    p = poolings.MLP(w, pcfg)
    p.to("cuda")
    p.set_zero_grad()
    obs = torch.rand(16, 3, 64, 64, generator=torch.Generator().manual_seed(17)).cuda()
    out = p(obs)
    out.square().sum().backward()
    g = w._module._cnn[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    before = w._module._cnn[0].weight.detach().clone()
    p.do_step()
    assert not torch.equal(before, w._module._cnn[0].weight)
