"""What the IODINE / broadcast-decoder kernel tests rest on, without a GPU: the eighth header (include/ocrl_hip_iodine.h) parses, binds and
is exported while the older tables stay as they were; every refusal its entry points make before a launch; the references of
tests/iodine_ref.py against themselves (analytic against autograd, an operator against its transpose, torch's own LSTMCell) and against
oracle/iodine_oracle.py's first refinement step; and the conditioning figures the bars of tests/test_gpu_iodine_kernels.py rest on: what
the same formulas lose when torch evaluates them in fp32, per input set and channel group, against the table of floors kept there."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from ocrl_amd import _abi, _lib
from oracle import iodine_oracle as IO
from tests import iodine_ref as R
from tests import test_gpu_iodine_kernels as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is refused before any launch
EXACT = 1e-10                   # fp64 against fp64: the same operation written twice
FUNCTIONS = {"ocrl_iodine_elbo_ws_floats": 3, "ocrl_iodine_elbo": 18, "ocrl_iodine_elbo_bwd": 10, "ocrl_iodine_sample_ws_floats": 1,
             "ocrl_iodine_sample": 12, "ocrl_iodine_latent": 11, "ocrl_iodine_post_grad": 12, "ocrl_iodine_im2col": 9, "ocrl_iodine_col2im": 10,
             "ocrl_iodine_refw_pack": 6, "ocrl_iodine_pool": 6, "ocrl_iodine_elu2": 9, "ocrl_iodine_lstm": 13, "ocrl_bcdec_c4_ws_floats": 0,
             "ocrl_bcdec_c4": 13, "ocrl_bcdec_c4_wgrad_blocks": 2, "ocrl_bcdec_c4_wgrad": 8, "ocrl_bcdec_mix_ws_floats": 0, "ocrl_bcdec_mix": 12,
             "ocrl_bcdec_compose": 7, "ocrl_bcdec_compose_bwd": 10}


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-300)


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_iodine.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == FUNCTIONS and abi.consts == {} and abi.structs == {}
    assert set(_lib.ABI_IODINE.functions) == set(FUNCTIONS)
    L = _lib.lib()
    for n, k in FUNCTIONS.items():
        assert len(getattr(L, n).argtypes) == k, n                                         # the symbol is exported and bound
    assert all(getattr(L, n).restype is ctypes.c_size_t for n in FUNCTIONS if n.endswith("_ws_floats"))
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_IODINE_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                         # self-contained
    # the older tables are what they were: the additions are additive
    assert len(_lib.ABI.functions) == 146 and _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    older = (_lib.ABI, _lib.ABI_DQN, _lib.ABI_ROLLOUT, _lib.ABI_REPLAY, _lib.ABI_C51, _lib.ABI_NOISY, _lib.ABI_CLASSIFIER)
    assert [len(a.functions) for a in older] == [146, 9, 1, 8, 6, 5, 1]
    assert not any(set(FUNCTIONS) & set(a.functions) for a in older)


# ---- refusals before any launch
def refused(rc, *words):
    msg = _lib.lib().ocrl_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_arguments_are_checked_before_any_launch():
    L = _lib.lib()
    p, big = ctypes.c_void_p(FAKE), 1 << 40

    def elbo(B=2, K=3, S=16, sigma=0.35, out4=p, part=p, enc=p, st1=p, st2=p, ws=p, n=big, ln=1):
        return L.ocrl_iodine_elbo(out4, p, B, K, S, sigma, ln, enc, st1, st2, p, part, p, p, p, ws, n, None)
    for K in (0, 17):
        refused(elbo(K=K), "1 <= K <= 16")
        refused(L.ocrl_iodine_elbo_bwd(p, p, None, 2, K, 16, 0.35, -1.0, p, None), "1 <= K <= 16")
        assert L.ocrl_iodine_elbo_ws_floats(2, K, 16) == 0
    for S in (0, 8, 24, 40):                                    # S * S % 256 != 0, or smaller than a block
        refused(elbo(S=S), "S % 16 == 0")
        refused(L.ocrl_iodine_elbo_bwd(p, p, None, 2, 3, S, 0.35, -1.0, p, None), "S % 16 == 0")
    refused(elbo(B=0), "B >= 1")
    refused(elbo(sigma=0.0), "sigma")
    refused(elbo(out4=None), "null"), refused(elbo(part=None), "null"), refused(elbo(ws=None), "null")
    refused(elbo(st1=None), "st1"), refused(elbo(st2=None), "st2")
    assert L.ocrl_iodine_elbo_ws_floats(2, 3, 32) == max(2 * 4 * 66, 2 * 3 * 4 * 4)
    assert L.ocrl_iodine_elbo_ws_floats(1, 16, 16) == max(66, 16 * 4)
    refused(elbo(S=32, n=2 * 4 * 66 - 1), "workspace too small")
    refused(L.ocrl_iodine_elbo_bwd(None, p, None, 2, 3, 16, 0.35, -1.0, p, None), "null")
    refused(L.ocrl_iodine_elbo_bwd(p, p, None, 2, 3, 16, 0.35, -1.0, None, None), "null")
    refused(L.ocrl_iodine_sample(p, p, None, p, p, p, 100, 1, 300, p, 99, None), "workspace too small")
    refused(L.ocrl_iodine_sample(p, p, None, p, p, p, 0, 1, 300, p, big, None), "n")
    refused(L.ocrl_iodine_sample(p, p, None, None, p, p, 100, 1, 300, p, big, None), "null")
    for Lz in (0, 1):
        refused(L.ocrl_iodine_latent(p, p, p, p, p, 4, Lz, 1.0, 1, 64, None), "L - 1")
    refused(L.ocrl_iodine_latent(p, p, p, p, p, 4, 16, 1.0, 1, 63, None), "ld >= 4 L")
    refused(L.ocrl_iodine_latent(p, p, p, None, p, 4, 16, 1.0, 1, 64, None), "null")
    refused(L.ocrl_iodine_post_grad(p, p, p, p, p, 31, 1.0, p, p, 4, 16, None), "ldl >= 2 L")
    refused(L.ocrl_iodine_post_grad(p, p, p, p, None, 0, 1.0, None, p, 4, 16, None), "null")
    refused(L.ocrl_iodine_im2col(p, p, 2, 17, 16, 16, 152, 0, None), "ldc >= 9 C")
    refused(L.ocrl_iodine_col2im(p, None, p, 2, 17, 16, 16, 152, 1, None), "ldc >= 9 C")
    refused(L.ocrl_iodine_im2col(p, None, 2, 17, 16, 16, 156, 0, None), "null")
    refused(L.ocrl_iodine_col2im(p, None, p, 0, 17, 16, 16, 156, 0, None), "Bn")
    refused(L.ocrl_iodine_refw_pack(p, p, 17, 152, 0, None), "ldc")
    refused(L.ocrl_iodine_pool(p, None, p, 3, 0, None), "n >= 1")
    refused(L.ocrl_iodine_elu2(p, 64, p, 63, 5, 64, None, 0, None), "row stride")
    refused(L.ocrl_iodine_elu2(p, 64, p, 64, 5, 64, p, 63, None), "row stride")
    refused(L.ocrl_iodine_lstm(None, p, p, p, p, None, None, None, None, 4, 64, 0, None), "null")
    refused(L.ocrl_iodine_lstm(None, p, p, p, None, None, None, None, p, 4, 64, 1, None), "null")
    refused(L.ocrl_iodine_lstm(p, p, p, p, p, None, None, None, None, 4, 0, 0, None), "H")
    assert L.ocrl_bcdec_c4_ws_floats() == 2 * 9 * 64 * 4
    refused(L.ocrl_bcdec_c4(p, 5, p, p, None, p, 1, 16, 0, 0, p, big, None), "co_n")
    refused(L.ocrl_bcdec_c4(p, 4, p, p, None, p, 1, 16, 2, 0, p, big, None), "mode")
    refused(L.ocrl_bcdec_c4(p, 4, None, p, None, p, 1, 16, 0, 0, p, big, None), "bias")
    refused(L.ocrl_bcdec_c4(p, 4, None, p, None, p, 1, 16, 1, 0, p, big, None), "act")
    refused(L.ocrl_bcdec_c4(p, 4, p, p, None, p, 1, 16, 0, 0, p, 4607, None), "workspace too small")
    refused(L.ocrl_bcdec_c4(p, 4, p, ctypes.c_void_p(FAKE + 4), None, p, 1, 16, 0, 0, p, big, None), "aligned")
    assert L.ocrl_bcdec_c4_wgrad_blocks(1, 16) == 4 and L.ocrl_bcdec_c4_wgrad_blocks(3, 48) == 72
    assert L.ocrl_bcdec_c4_wgrad_blocks(33, 64) == 1024 and L.ocrl_bcdec_c4_wgrad_blocks(0, 64) == 0
    refused(L.ocrl_bcdec_c4_wgrad(p, p, p, 4 * 2304 - 1, 1, 16, 0, None), "part too small")
    refused(L.ocrl_bcdec_c4_wgrad(p, p, p, big, 1, 16, 3, None), "form")
    refused(L.ocrl_bcdec_c4_wgrad(p, None, p, big, 1, 16, 1, None), "null")
    for K in (0, 17):
        refused(L.ocrl_bcdec_mix(p, p, None, None, p, 2, K, 16, 3, p, 1024, None), "1 <= K <= 16")
    refused(L.ocrl_bcdec_mix(p, p, None, None, p, 2, 3, 16, 4, p, 1024, None), "C <= 3")
    refused(L.ocrl_bcdec_mix(p, p, None, None, p, 2, 3, 16, 3, p, 1023, None), "workspace too small")
    refused(L.ocrl_bcdec_mix(p, p, None, None, None, 2, 3, 16, 3, p, 1024, None), "null")
    refused(L.ocrl_bcdec_compose(p, p, p, p, None, 64, None), "null")
    refused(L.ocrl_bcdec_compose_bwd(p, p, p, p, p, p, p, p, 0, None), "D")


# ---- the references against themselves
@pytest.mark.parametrize("K,sigma,kind", [(1, 0.35, "well"), (3, 0.35, "well"), (9, 0.1, "spread"), (5, 0.35, "saturated")])
def test_elbo_gradients_analytic_against_autograd(K, sigma, kind):
    obs, rec, lg, denc = R.elbo_inputs(kind, K, 16, 2)
    for de in (None, denc):
        assert rel(R.elbo_bwd_analytic(obs, rec, lg, de, sigma, -0.4), R.elbo_bwd(obs, rec, lg, de, sigma, -0.4)) < EXACT
    # the in-forward gradient is the same expression with weight 1 and no encoding term
    assert rel(R.elbo_bwd_analytic(obs, rec, lg, None, sigma, 1.0), R.elbo_fwd(obs, rec, lg, sigma, True)["dout4"]) < EXACT
    # only channels 3-8 of the encoding carry gradient: whatever denc holds elsewhere changes nothing
    live = torch.zeros_like(denc)
    live[:, :, 3:9] = denc[:, :, 3:9]
    assert torch.equal(R.elbo_bwd(obs, rec, lg, denc, sigma, -0.4), R.elbo_bwd(obs, rec, lg, live, sigma, -0.4))
    dead = denc - live
    assert torch.equal(R.elbo_bwd(obs, rec, lg, dead, sigma, -0.4), R.elbo_bwd(obs, rec, lg, None, sigma, -0.4))


@pytest.mark.parametrize("ln", [True, False])
def test_elbo_reference_reproduces_the_oracles_first_step(ln):
    """trace[0] of iodine_forward on formula_params, in fp64: the encoding from the reference's own entry point on that step's decoder
    output, and the latent vector from d(B ll) / d slots of the same step"""
    cfg = IO.default_cfg(obs_size=16, num_slots=3, num_iterations=2, layer_norm=ln, beta=2.0)
    P = {k: v.double().requires_grad_(True) for k, v in IO.formula_params(cfg).items()}
    B = 2
    obs = torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(3)).double()
    eps = IO.make_noise(cfg, B, 4).double()
    t0 = IO.iodine_forward(P, obs, eps, cfg, return_all=True)["trace"][0]
    rec, lg = t0["recons"].detach(), t0["mask_logits"].detach()
    ref = R.elbo_fwd(obs, rec, lg, cfg.sigma, ln)
    assert rel(ref["enc"], R.nhwc(t0["enc"].detach())) < EXACT and rel(ref["masks"], t0["masks"][:, :, 0].detach()) < EXACT
    slots = t0["slots"].detach().clone().requires_grad_(True)
    r2, l2 = IO.decoder({k: v.detach() for k, v in P.items()}, slots, cfg)
    z = slots.new_zeros(B, cfg.num_slots, 1)
    (ds,) = torch.autograd.grad(IO.elbo_terms(obs, z, z, z, r2, l2, cfg)["pll"].sum(), slots)
    mu, ls = t0["means"].detach().reshape(B * 3, -1), t0["logsigs"].detach().reshape(B * 3, -1)
    lat = R.latent(mu, ls, eps[0].reshape(B * 3, -1), ds.reshape(B * 3, -1), cfg.beta, ln)
    assert rel(lat, t0["latent"].detach().reshape(B * 3, -1)) < EXACT


def test_posterior_references():
    mu, ls, eps, ds, dlat = G.posterior_inputs(5, 36, 2)
    for d in (None, dlat):
        for a, b in zip(R.post_grad_analytic(mu, ls, eps, ds, d, 1.3), R.post_grad(mu, ls, eps, ds, d, 1.3)):
            assert rel(a, b) < EXACT
    lat = R.latent(mu, ls, eps, ds, 4.0, True)
    g = ds.double() - 4.0 * mu.double()
    want = (g - g.mean(1, keepdim=True)) / ((((g - g.mean(1, keepdim=True)) ** 2).sum(1, keepdim=True) / 35).sqrt() + 1e-5)       # L - 1
    assert rel(lat[:, 72:108], want) < EXACT and torch.equal(lat[:, :36], mu.double()) and torch.equal(lat[:, 36:72], ls.double())
    slots, kl = R.sample(mu, ls, eps)
    q = torch.distributions.Normal(mu.double(), ls.double().exp())
    assert rel(kl, torch.distributions.kl_divergence(q, torch.distributions.Normal(0.0, 1.0)).sum()) < EXACT


@pytest.mark.parametrize("C,Hi", [(17, 16), (17, 3), (64, 6), (64, 2)])
def test_im2col_is_the_strided_convolution_and_col2im_its_transpose(C, Hi):
    g = torch.Generator().manual_seed(C + Hi)
    x, W = torch.randn(2, Hi, Hi, C, generator=g).double(), torch.randn(64, C, 3, 3, generator=g).double()
    ldc = G.model_ldc(C) + 8
    Ho = R.out_size(Hi)
    col, Wp = R.im2col(x, ldc), R.refw_pack(W, ldc)
    conv = F.conv2d(x.permute(0, 3, 1, 2), W, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, 64)
    assert col.shape == (2 * Ho * Ho, ldc) and rel(col @ Wp.t(), conv) < EXACT and bool((col[:, 9 * C:] == 0).all())
    dcol = torch.randn(2 * Ho * Ho, ldc, generator=g).double()
    dx = R.col2im(dcol, None, x.shape)
    assert abs((col[:, :9 * C] * dcol[:, :9 * C]).sum().item() - (x * dx).sum().item()) < EXACT * (x.abs() * dx.abs()).sum().item()
    act = F.elu(torch.randn(2, Hi, Hi, C, generator=g).double())
    pre = torch.where(act > 0, act, torch.log1p(act))                      # the pre-activation whose ELU is act
    gate = torch.autograd.functional.jvp(F.elu, pre, torch.ones_like(pre))[1]
    assert rel(R.col2im(dcol, act, x.shape), dx * gate) < EXACT


def test_lstm_reference_is_torchs_cell():
    g = torch.Generator().manual_seed(0)
    H, rows = 64, 7
    cell = torch.nn.LSTMCell(32, H).double()
    x, h0, c0 = (torch.randn(rows, n, generator=g).double() for n in (32, H, H))
    gates = F.linear(x, cell.weight_ih, cell.bias_ih) + F.linear(h0, cell.weight_hh, cell.bias_hh)
    acts, c1, h1, dgates, dc0 = R.lstm(gates.detach(), c0, torch.ones(rows, H), None)
    h_t, c_t = cell(x, (h0, c0.clone().requires_grad_(True)))
    assert rel(h1, h_t.detach()) < EXACT and rel(c1, c_t.detach()) < EXACT
    assert float(R.lstm(gates.detach(), c0, None, None)[3].abs().max()) == 0.0


def test_c4_mix_and_compose_references():
    X, W, bias, dY, act = G.c4_inputs(20, 1, 3, 1)
    Y, dX, dW = R.c4(X, W, bias, dY, act, 1)
    assert bool((Y[..., 3] == bias[3].double()).all())                                             # the missing output channel
    # <dY, conv(X)> is linear in X and in W
    lin = (Y - bias.double()) * dY.double()
    assert abs(lin.sum().item() - (dW[:3] * W.double()).sum().item()) < EXACT * lin.abs().sum().item()
    relu = R.c4(X, W, bias, dY, F.relu(act), 0)[1]
    assert bool((relu[F.relu(act) == 0] == 0).all())
    g = torch.Generator().manual_seed(1)
    out4 = torch.randn(2, 1, 16, 16, 4, generator=g)
    recon, loss, d = R.mix(out4, torch.rand(2, 3, 16, 16, generator=g))
    assert torch.equal(recon, out4[:, 0, ..., :3].double()) and float(d[..., 3].abs().max()) == 0.0   # one slot: the mask is 1
    W1, Wpos, bpos = torch.randn(64, 8, 5, 5, generator=g), torch.randn(8, 4, generator=g), torch.randn(8, generator=g)
    Wc, W1r = R.compose(W1, Wpos, bpos)
    pos = torch.randn(4, 9, 9, generator=g).double()
    direct = F.conv2d((torch.einsum("dj,jhw->dhw", Wpos.double(), pos) + bpos.double()[:, None, None])[None], W1.double())[0, :, 0, 0]
    patch = torch.cat((pos[:, :5, :5].reshape(4, 25), torch.ones(1, 25, dtype=torch.float64)))
    assert rel(torch.einsum("toj,jt->o", Wc, patch), direct) < EXACT and torch.equal(W1r[7, 3], W1[3, :, 1, 2].double())


# ---- the conditioning figures the GPU bars rest on
@pytest.mark.parametrize("kind,sigma,case", [pytest.param(k, s, c, id=f"{k}-s{s}-K{c[0]}-S{c[1]}-B{c[2]}") for k, s, cs in G.ELBO_SETS for c in cs])
def test_fp32_floors_of_the_reference_formulas(kind, sigma, case):
    """The reference's formulas in fp32 (torch, CPU) against fp64.  Where the GPU test applies TOL the formulas themselves must hold
    TOL / 4 in fp32, or TOL would not be a fair bar; where it applies max(TOL, 4 x floor) the floor in its table must be the one
    measured here.  A floor that widens a bar must lie within a factor 1.5 of this measurement either way, so the bar stays between 2.7
    and 6 times what this machine measures (the table's provenance is noted beside it; the maximum of rounding noise can move with the
    CPU's vector width); a floor that does not widen a bar only has to be confirmed as not widening it."""
    K, S, B = case
    obs, rec, lg, denc = R.elbo_inputs(kind, K, S, B)
    pairs = R.elbo_pairs(kind, sigma, case)
    fl = R.elbo_floors(pairs)
    for ln in (True, False):
        hi, lo = pairs[ln]
        assert all(bool(torch.isfinite(v).all()) for v in hi.values()) and all(bool(torch.isfinite(v).all()) for v in lo.values())
        for n in ("ll", "mse", "masks", "recon", "recons_masked"):
            assert R._rel(lo[n], hi[n]) <= G.TOL / 4, (n, ln)
        assert R._rel(lo["dout4"][..., :3], hi["dout4"][..., :3]) <= G.TOL / 4 and R._rel(lo["dout4"][..., 3], hi["dout4"][..., 3]) <= G.TOL / 4
        for g, sl in (R.ENC_GROUPS[0], R.ENC_GROUPS[5]):
            assert R._rel(lo["enc"][..., sl], hi["enc"][..., sl]) <= G.TOL / 4, (g, ln)
    for de in (None, denc):
        a, b = R.elbo_bwd(obs, rec, lg, de, sigma, -0.5, dtype=torch.float32), R.elbo_bwd(obs, rec, lg, de, sigma, -0.5)
        assert R._rel(a[..., :3], b[..., :3]) <= G.TOL / 4 and R._rel(a[..., 3], b[..., 3]) <= G.TOL / 4
    for ln in (True, False, None):
        if kind == "saturated" and ln is True:
            assert (kind, case, ln) not in G.FLOORS                     # not compared: the fp32 formulas are off by more than 1e-4 there
            assert max(fl[True].values()) > 1e-4
            continue
        for g, v in fl[ln].items():
            if kind == "well":
                if not (K == 1 and ln is not False and g in ("12", "st2:12")):          # the layer norm of a constant: graded as zeros
                    assert v <= G.TOL / 4, (ln, g, v)
                continue
            t = G.FLOORS[(kind, case, ln)][g]
            if 4 * t > G.TOL:
                assert t / 1.5 <= v <= 1.5 * t, (ln, g, v, t)
            else:
                assert 4 * v <= G.TOL, (ln, g, v, t)
            assert G.bar_of(kind, case, ln, g) == max(G.TOL, 4 * t)
    if kind != "well":
        assert set(k for k in G.FLOORS if k[:2] == (kind, case)) == {(kind, case, ln) for ln in ((False, None) if kind == "saturated" else (True, False, None))}
