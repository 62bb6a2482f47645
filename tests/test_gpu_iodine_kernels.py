"""The IODINE kernels (iodine.hip) and the broadcast decoder's own kernels (bcdec.hip) one by one through include/ocrl_hip_iodine.h against
the fp64 references of tests/iodine_ref.py, at the shapes IodineModel::bind accepts and tests/test_gpu_iodine.py does not reach: the
MAXK = 16 instantiations and the K = 8 / 9 boundary, K = 1, slot sizes 4 .. 256, S = 48, the stride loop of the 64 -> 4 weight gradient
beyond its 1024-block cap and its VALU form, the generic im2col / col2im kernels, the Slot-Attention mixture, the device-drawn noise.

Bar: TOL = 2e-5 of the reference tensor's maximum per output tensor (tests/test_gpu_kernels.py), per channel group for the encoding; a
reference that is exactly zero requires exact zeros.  The exceptions are tabulated below (FLOORS).  Outputs a kernel must write in full are
pre-filled with NaN and must come back finite; columns it must not touch hold a sentinel."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import iodine_oracle as IO
from tests import iodine_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu
TOL = 2e-5
NAN = float("nan")
SENTINEL = -777.0

# ------------------------------------------------------------------------------------------------------------------- ELBO inputs
# (K, S, B): both sides of the MAXK = 8 / 16 boundary, every register array full, one slot, nine blocks per image, several blocks
ELBO_CASES = [(1, 16, 2), (2, 16, 3), (7, 16, 2), (8, 16, 2), (9, 16, 2), (16, 16, 1), (3, 48, 1), (5, 32, 2)]
WIDE_CASES = [(5, 32, 2), (16, 16, 1)]
# (input set of iodine_ref.INPUT_SETS, sigma, cases).  "well" (mask logits ~ N(0, 1)): every output holds TOL.  "spread" (~ N(0, 4^2),
# sigma 0.1) and "saturated" (~ N(0, 8^2): the smallest mask is 1e-21, for log(m + 1e-12) and 1 / (m + 1e-12)): the gradient, likelihood
# and leave-one-out channels 9-14, and their sums st1 / st2, lose more than TOL in fp32 whoever computes them -- the leave-one-out term
# divides by 1 - m + 1e-5 where m rounds to 1 -- so their bar is max(TOL, 4 x floor), floor = what the reference's own formulas lose when
# torch evaluates them in fp32 on the CPU (tests/test_iodine_ref_cpu.py measures it and holds this table to it).  The factor 4 covers
# another summation order and expf / logf a few ulp apart; it cannot cover a wrong term.  Under the layer norm the saturated set's fp32
# channels 9-14 are off by up to 5e-3 of their maximum and are not compared; without it they are, under the same rule.  Every other
# output of these sets holds TOL.
ELBO_SETS = [("well", 0.35, ELBO_CASES), ("well", 0.1, ELBO_CASES), ("spread", 0.1, WIDE_CASES), ("saturated", 0.35, WIDE_CASES)]
# (set, (K, S, B), layer_norm or None for st1 / st2) -> floor per group (the fp32-torch-vs-fp64 error relative to the group's maximum),
# measured with torch 2.10 on an x86-64 CPU whose torch kernels are the AVX512 ones (torch.backends.cpu.get_cpu_capability()).
# What the table shows: only the leave-one-out term is above TOL / 4, so only its bars are wider than TOL.  That term is channel 14 of
# the encoding and, beyond the channels the rule was written for, its two sums: column 14 of st1 (the sum the layer norm's mean is taken
# from) and of st2 (its squared deviations), which inherit the same cancellation and are measured in the same way.  The bars: channel 14
# 7.6e-3 and 1.2e-2 of the channel's maximum at K = 5 (spread, with and without the layer norm), 1.9e-2 at K = 5 saturated, 3.2e-3 at
# K = 16 saturated, 2.2e-5 at K = 16 spread; st1:14 1.5e-3 / 1.5e-4 / 8e-5 and st2:14 6e-3 / 2.4e-4 / 7.6e-5 in the same order.
FLOORS = {
    ("spread", (5, 32, 2), True): {"9-11": 8.7e-07, "12": 5.8e-07, "13": 2.3e-07, "14": 1.9e-03},
    ("spread", (5, 32, 2), False): {"9-11": 7.7e-07, "12": 3.8e-07, "13": 4.0e-07, "14": 3.0e-03},
    ("spread", (5, 32, 2), None): {"st1:9-11": 3.3e-07, "st1:12": 4.8e-07, "st1:13": 1.2e-07, "st1:14": 3.8e-04,
                                   "st2:9-11": 1.3e-07, "st2:12": 4.2e-07, "st2:13": 5.0e-07, "st2:14": 1.5e-03},
    ("spread", (16, 16, 1), True): {"9-11": 4.1e-07, "12": 4.0e-07, "13": 1.7e-07, "14": 4.8e-06},
    ("spread", (16, 16, 1), False): {"9-11": 5.1e-07, "12": 7.6e-07, "13": 1.3e-07, "14": 5.4e-06},
    ("spread", (16, 16, 1), None): {"st1:9-11": 2.4e-07, "st1:12": 4.9e-07, "st1:13": 8.9e-08, "st1:14": 1.5e-06,
                                    "st2:9-11": 2.0e-07, "st2:12": 1.5e-06, "st2:13": 2.7e-07, "st2:14": 2.2e-06},
    ("saturated", (5, 32, 2), False): {"9-11": 3.4e-07, "12": 1.4e-06, "13": 3.2e-07, "14": 4.7e-03},
    ("saturated", (5, 32, 2), None): {"st1:9-11": 1.5e-07, "st1:12": 1.9e-07, "st1:13": 6.1e-08, "st1:14": 3.8e-05,
                                      "st2:9-11": 6.4e-08, "st2:12": 7.9e-07, "st2:13": 7.9e-08, "st2:14": 5.9e-05},
    ("saturated", (16, 16, 1), False): {"9-11": 2.2e-07, "12": 2.1e-06, "13": 5.0e-07, "14": 8.1e-04},
    ("saturated", (16, 16, 1), None): {"st1:9-11": 1.7e-07, "st1:12": 2.3e-07, "st1:13": 3.6e-08, "st1:14": 2.0e-05,
                                       "st2:9-11": 9.9e-08, "st2:12": 1.1e-06, "st2:13": 2.0e-07, "st2:14": 1.9e-05},
}


def bar_of(kind, case, ln, group):
    """the bar of an encoding group (or an "st1:" / "st2:" column) at an input set"""
    if kind == "well" or group in ("0-8", "15-16"):
        return TOL
    return max(TOL, 4 * FLOORS[(kind, case, ln)][group])


ELBO_PARAMS = [pytest.param(kind, sigma, case, ln, id=f"{kind}-s{sigma}-K{case[0]}-S{case[1]}-B{case[2]}-{'ln' if ln else 'raw'}")
               for kind, sigma, cases in ELBO_SETS for case in cases for ln in (True, False)]


# ------------------------------------------------------------------------------------------------------------------- helpers
def lib():
    from ocrl_amd import _lib
    return _lib.lib()


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def P(t):
    """device pointer of a tensor (None: null); the tensor is held until the test ends, so that a temporary's memory is not handed to the
    next allocation while a launch that reads it is still queued"""
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def stream():
    from ocrl_amd import _lib
    return _lib.stream()


def ok(rc):
    from ocrl_amd import _lib
    _lib.check(rc)


def dev(t):
    return t.detach().float().contiguous().cuda()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen)


def err(got, ref):
    """max |got - ref| / max |ref| against fp64; an exactly zero reference requires exact zeros (inf otherwise)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = ref.abs().max().item() if ref.numel() else 0.0
    d = (got - ref).abs().max().item() if ref.numel() else 0.0
    if den == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / den


def grade(tag, rows):
    """rows: (name, got, ref, bar); logs every error -- with its floor and bar where the bar is a floor-derived one, which is then
    4 x the floor (bar_of) -- then asserts finiteness and the bars"""
    out = []
    for name, got, ref, bar in rows:
        assert bool(torch.isfinite(got).all()), f"{tag}: {name} is not finite"
        out.append((name, err(got, ref), bar))
    log(f"[iok {tag}] " + " ".join(f"{n}={e:.1e}" + (f"(floor {b / 4:.1e} bar {b:.1e})" if b != TOL else "") for n, e, b in out))
    bad = [(n, e, b) for n, e, b in out if not e <= b]
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------------------------- ELBO
@functools.lru_cache(maxsize=None)
def elbo_case(kind, sigma, case, ln):
    K, S, B = case
    obs, rec, lg, denc = R.elbo_inputs(kind, K, S, B)
    return obs, rec, lg, denc, R.elbo_fwd(obs, rec, lg, sigma, ln)


ELBO_OUT = ("enc", "dout4", "masks", "recon", "recons_masked")


def run_elbo(out4, obs, case, sigma, ln, want, part):
    K, S, B = case
    shapes = dict(enc=(B, K, S, S, 17), dout4=(B, K, S, S, 4), masks=(B, K, S, S), recon=(B, 3, S, S), recons_masked=(B, K, 3, S, S))
    o = {n: (nans(*shapes[n]) if n in want else None) for n in ELBO_OUT}
    o["st1"] = nans(B, K, 4) if "enc" in want else None
    o["st2"] = nans(B, K, 4) if "enc" in want and ln else None
    n = lib().ocrl_iodine_elbo_ws_floats(B, K, S)
    assert n >= B * (S * S // 256) * 66
    ws = nans(n)
    ok(lib().ocrl_iodine_elbo(P(out4), P(obs), B, K, S, sigma, int(ln), P(o["enc"]), P(o["st1"]), P(o["st2"]), P(o["dout4"]), P(part), P(o["masks"]),
                              P(o["recon"]), P(o["recons_masked"]), P(ws), n, stream()))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("kind,sigma,case,ln", ELBO_PARAMS)
def test_elbo_forward(kind, sigma, case, ln):
    K, S, B = case
    obs, rec, lg, _, ref = elbo_case(kind, sigma, case, ln)
    out4, obs_d = dev(R.to_out4(rec, lg)), dev(obs)
    part = torch.zeros(2, device="cuda")
    o = run_elbo(out4, obs_d, case, sigma, ln, ELBO_OUT, part)
    first = part.clone()
    tag = f"elbo {kind} s{sigma} K{K} S{S} B{B} {'ln' if ln else 'raw'}"
    rows = [("ll", first[0], ref["ll"], TOL), ("mse", first[1], ref["mse"], TOL), ("masks", o["masks"], ref["masks"], TOL),
            ("recon", o["recon"], ref["recon"], TOL), ("recons_masked", o["recons_masked"], ref["recons_masked"], TOL),
            ("d_rgb", o["dout4"][..., :3], ref["dout4"][..., :3], TOL), ("d_logit", o["dout4"][..., 3], ref["dout4"][..., 3], TOL)]
    cols = ("9-11", "12", "13", "14")
    for j, g in enumerate(cols):
        rows.append((f"st1:{g}", o["st1"][..., j], ref["st1"][..., j], bar_of(kind, case, None, f"st1:{g}")))
        if ln:
            want = ref["st2"][..., j]
            if K == 1 and g == "12":                      # the squared deviations of a constant (see channel 12 below)
                assert want.abs().max().item() < 1e-20
                want = torch.zeros_like(want)
            rows.append((f"st2:{g}", o["st2"][..., j], want, bar_of(kind, case, None, f"st2:{g}")))
    for g, sl in R.ENC_GROUPS:
        want = ref["enc"][..., sl]
        if kind == "saturated" and ln and g in cols:
            assert bool(torch.isfinite(o["enc"][..., sl]).all()), (tag, g)
            continue
        if K == 1 and ln and g == "12":
            # one slot: the mask is 1 at every pixel, so d elbo / d mask = sum_c post / (1 + 1e-12) is one number and its layer norm is 0;
            # the fp64 reference holds rounding residue of that constant over 1e-5 instead (checked to be no more)
            assert want.abs().max().item() < 1e-9
            want = torch.zeros_like(want)
        rows.append((f"enc:{g}", o["enc"][..., sl], want, bar_of(kind, case, ln, g)))
    grade(tag, rows)
    # the properties that hold whatever the reference says
    assert (o["masks"].double().sum(dim=1) - 1).abs().max().item() <= (K + 2) * 2.0 ** -23        # K roundings of e_k / sum
    for n in ("recon", "recons_masked"):
        assert o[n].min().item() >= 0.0 and o[n].max().item() <= 1.0, n
    xy = IO.coords(S, dtype=torch.float64).permute(1, 2, 0)
    assert (o["enc"][..., 15:17].double().cpu() - xy).abs().max().item() <= 2.0 ** -23             # one ulp at 1
    # part accumulates: a second call adds the same two sums (fl(p + p) = 2 p), here with every optional output left out
    run_elbo(out4, obs_d, case, sigma, ln, (), part)
    assert torch.equal(part, 2 * first), (part, first)
    # each optional output alone is what it was with all of them
    for n in ELBO_OUT:
        p2 = torch.zeros(2, device="cuda")
        alone = run_elbo(out4, obs_d, case, sigma, ln, (n,), p2)
        assert torch.equal(p2, first), n
        for m in (n, "st1", "st2") if n == "enc" else (n,):
            if alone[m] is not None:
                assert torch.equal(alone[m], o[m]), (n, m)


@pytest.mark.parametrize("kind,sigma,case", [pytest.param(k, s, c, id=f"{k}-s{s}-K{c[0]}-S{c[1]}-B{c[2]}") for k, s, cs in ELBO_SETS for c in cs])
def test_elbo_backward(kind, sigma, case):
    K, S, B = case
    obs, rec, lg, denc = R.elbo_inputs(kind, K, S, B)
    out4, obs_d = dev(R.to_out4(rec, lg)), dev(obs)
    cw = -2.0 / (3.0 * B)                                   # iteration 2 of 3
    rows = []
    for name, de in (("plain", None), ("denc", denc)):
        ref = R.elbo_bwd(obs, rec, lg, de, sigma, cw)
        got = nans(B, K, S, S, 4)
        ok(lib().ocrl_iodine_elbo_bwd(P(out4), P(obs_d), P(None if de is None else dev(R.nhwc(de))), B, K, S, sigma, cw, P(got), stream()))
        torch.cuda.synchronize()
        rows += [(f"{name}:d_rgb", got[..., :3], ref[..., :3], TOL), (f"{name}:d_logit", got[..., 3], ref[..., 3], TOL)]
    grade(f"elbo_bwd {kind} s{sigma} K{K} S{S} B{B}", rows)


# ------------------------------------------------------------------------------------------------------------------- sampling
def run_sample(mu, ls, noise, seed=0, site=300):
    n = mu.numel()
    eps, slots, kl = nans(n), nans(n), nans(1)
    nws = lib().ocrl_iodine_sample_ws_floats(n)
    assert nws >= n
    ws = nans(nws)
    ok(lib().ocrl_iodine_sample(P(mu), P(ls), P(noise), P(eps), P(slots), P(kl), n, seed, site, P(ws), nws, stream()))
    torch.cuda.synchronize()
    return eps, slots, kl


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024 * 3 + 5])
def test_sample_injected_noise(n):
    g = torch.Generator().manual_seed(n)
    mu, ls, noise = rnd(g, n), 0.5 * rnd(g, n), rnd(g, n)
    slots, kl = R.sample(mu, ls, noise)
    eps_d, slots_d, kl_d = run_sample(dev(mu), dev(ls), dev(noise))
    assert torch.equal(eps_d.cpu(), noise)
    e_kl = abs(kl_d.item() - kl.item()) / abs(kl.item())
    log(f"[iok sample n={n}] slots={err(slots_d, slots):.1e} kl={e_kl:.1e}")
    assert math.isfinite(kl_d.item()) and err(slots_d, slots) <= TOL and e_kl <= TOL


def test_sample_device_noise():
    n = 1 << 20
    z = torch.zeros(n, device="cuda")
    a, slots, kl = run_sample(z, z, None, seed=11, site=300)
    b, _, _ = run_sample(z, z, None, seed=11, site=300)
    c, _, _ = run_sample(z, z, None, seed=12, site=300)
    d, _, _ = run_sample(z, z, None, seed=11, site=301)
    assert torch.equal(a, b) and torch.equal(slots, a)                  # mu = 0, ls = 0: slots = eps
    for other in (c, d):
        assert (other == a).float().mean().item() < 1e-3
    assert bool(torch.isfinite(a).all()) and a.abs().max().item() <= math.sqrt(2 * 25 * math.log(2)) * (1 + 1e-6)      # u01_24 >= 2^-25
    x = a.double()
    mean, var = x.mean().item(), x.var(unbiased=False).item()
    zs = (x - mean) / math.sqrt(var)
    skew, kurt = (zs ** 3).mean().item(), (zs ** 4).mean().item() - 3
    corr = (zs[1:] * zs[:-1]).mean().item()
    log(f"[iok sample device n={n}] mean={mean:.2e} var-1={var - 1:.2e} skew={skew:.2e} kurt={kurt:.2e} lag1={corr:.2e} max={a.abs().max().item():.3f}")
    # five standard errors of the moments of n independent N(0, 1) draws
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(skew) <= 5 * math.sqrt(6 / n) and abs(kurt) <= 5 * math.sqrt(24 / n) and abs(corr) <= 5 / math.sqrt(n)
    assert kl.item() == 0.0                                # -0 + (1 + 0) / 2 - 1/2 at every element: the KL of the prior from itself


# ------------------------------------------------------------------------------------------------------------------- latent, posterior
LS = [4, 36, 64, 100, 256]
BKS = [1, 3, 4, 5, 33]                  # four rows per workgroup


def posterior_inputs(BK, L, seed):
    g = torch.Generator().manual_seed(seed * 1000 + BK * 7 + L)
    return rnd(g, BK, L), 0.5 * rnd(g, BK, L), rnd(g, BK, L), rnd(g, BK, L), rnd(g, BK, 4 * L + 8)


@pytest.mark.parametrize("beta", [1.0, 4.0])
@pytest.mark.parametrize("ln", [True, False], ids=["ln", "raw"])
@pytest.mark.parametrize("L", LS)
def test_latent(L, ln, beta):
    rows = []
    for BK in BKS:
        mu, ls, eps, ds, _ = posterior_inputs(BK, L, 1)
        ref = R.latent(mu, ls, eps, ds, beta, ln)
        ld = 4 * L + 8                                    # as xin: the latent sits inside a wider row
        out = torch.full((BK, ld), SENTINEL, device="cuda")
        out[:, 4:4 + 4 * L] = NAN
        ok(lib().ocrl_iodine_latent(P(dev(mu)), P(dev(ls)), P(dev(eps)), P(dev(ds)), ctypes.c_void_p(out.data_ptr() + 16), BK, L, beta, int(ln), ld,
                                    stream()))
        torch.cuda.synchronize()
        assert bool((out[:, :4] == SENTINEL).all()) and bool((out[:, 4 + 4 * L:] == SENTINEL).all()), (BK, L)
        for j, n in enumerate(("mu", "ls", "gmu", "gls")):
            rows.append((f"BK{BK}:{n}", out[:, 4 + j * L:4 + (j + 1) * L], ref[:, j * L:(j + 1) * L], TOL))
    grade(f"latent L{L} {'ln' if ln else 'raw'} beta{beta}", rows)


@pytest.mark.parametrize("with_dlat", [False, True], ids=["plain", "dlat"])
@pytest.mark.parametrize("L", LS)
def test_post_grad(L, with_dlat):
    rows = []
    for BK in BKS:
        mu, ls, eps, ds, dlat = posterior_inputs(BK, L, 2)
        kw = 2.0 / 3.0 * 4.0 / 2.0
        a, b = R.post_grad(mu, ls, eps, ds, dlat if with_dlat else None, kw)
        g0 = posterior_inputs(BK, L, 3)
        gmu, gls = dev(g0[0]), dev(g0[1])
        dl = dev(dlat) if with_dlat else None
        for rep in (1, 2):                               # gmu and gls accumulate: the second call adds the same again
            ok(lib().ocrl_iodine_post_grad(P(dev(mu)), P(dev(ls)), P(dev(eps)), P(dev(ds)), P(dl), 4 * L + 8, kw, P(gmu), P(gls), BK, L, stream()))
            torch.cuda.synchronize()
            rows += [(f"BK{BK}x{rep}:gmu", gmu.clone(), g0[0].double() + rep * a, TOL), (f"BK{BK}x{rep}:gls", gls.clone(), g0[1].double() + rep * b, TOL)]
    grade(f"post_grad L{L} {'dlat' if with_dlat else 'plain'}", rows)


# ------------------------------------------------------------------------------------------------------------------- im2col, col2im, pack
def model_ldc(C):
    return (9 * C + 3) & ~3              # IodineModel's ldc_: 156 for the 17-channel encoding, 576 for 64 channels


@pytest.mark.parametrize("Hi", [16, 8, 6, 4, 3, 2])          # Ho = (Hi - 1) / 2 + 1: 3 arises at S = 48
@pytest.mark.parametrize("C", [17, 64])
def test_im2col_col2im(C, Hi):
    rows = []
    for Bn in (1, 5):
        for ldc in (model_ldc(C), model_ldc(C) + 8):
            g = torch.Generator().manual_seed(C * 100 + Hi * 10 + Bn)
            x = rnd(g, Bn, Hi, Hi, C)
            Ho = R.out_size(Hi)
            col_ref = R.im2col(x, ldc)
            dcol = rnd(g, Bn * Ho * Ho, ldc)               # the padding columns hold noise: nothing may read them
            act = F.elu(rnd(g, Bn, Hi, Hi, C))
            dx_ref = {a: R.col2im(dcol, act if a else None, x.shape) for a in (False, True)}
            for force in (0, 1):
                tag = f"B{Bn} ldc{ldc} {'generic' if force else 'dispatched'}"
                col = nans(Bn * Ho * Ho, ldc)
                ok(lib().ocrl_iodine_im2col(P(dev(x)), P(col), Bn, C, Hi, Hi, ldc, force, stream()))
                torch.cuda.synchronize()
                assert torch.equal(col.cpu(), col_ref), tag                                      # a copy: bit for bit
                assert bool((col[:, 9 * C:] == 0).all()), tag
                for a in (False, True):
                    dx = nans(Bn, Hi, Hi, C)
                    ok(lib().ocrl_iodine_col2im(P(dev(dcol)), P(dev(act)) if a else None, P(dx), Bn, C, Hi, Hi, ldc, force, stream()))
                    torch.cuda.synchronize()
                    rows.append((f"{tag} {'act' if a else 'noact'}", dx, dx_ref[a], TOL))
    grade(f"col2im C{C} H{Hi}", rows)


@pytest.mark.parametrize("C", [17, 64])
def test_refw_pack_unpack(C):
    g = torch.Generator().manual_seed(C)
    W = rnd(g, 64, C, 3, 3)
    for ldc in (model_ldc(C), model_ldc(C) + 8):
        Wp = nans(64, ldc)
        ok(lib().ocrl_iodine_refw_pack(P(dev(W)), P(Wp), C, ldc, 0, stream()))
        torch.cuda.synchronize()
        assert torch.equal(Wp.cpu(), R.refw_pack(W, ldc)) and bool((Wp[:, 9 * C:] == 0).all())
        Wp[:, 9 * C:] = NAN                              # the way back reads the 9 C live columns only
        back = nans(64, C, 3, 3)
        ok(lib().ocrl_iodine_refw_pack(P(Wp), P(back), C, ldc, 1, stream()))
        torch.cuda.synchronize()
        assert torch.equal(back.cpu(), W), ldc
    log(f"[iok refw_pack C{C}] pack == reference, unpack(pack(W)) == W, bit for bit")


# ------------------------------------------------------------------------------------------------------------------- pool, ELU, LSTM
@pytest.mark.parametrize("n", [1, 4, 9, 64])
def test_pool(n):
    BK = 3
    g = torch.Generator().manual_seed(n)
    pre, dpool = rnd(g, BK, n, 64), rnd(g, BK, 64)
    r, p_ref, dpre_ref = R.pool(pre, dpool)
    r_d, p, dpre = dev(r), nans(BK, 64), nans(BK, n, 64)
    ok(lib().ocrl_iodine_pool(P(r_d), None, P(p), BK, n, stream()))
    ok(lib().ocrl_iodine_pool(P(r_d), P(dev(dpool)), P(dpre), BK, n, stream()))
    torch.cuda.synchronize()
    grade(f"pool n{n}", [("pool", p, p_ref, TOL), ("dpre", dpre, dpre_ref, TOL)])


@pytest.mark.parametrize("Fd,L", [(64, 36), (256, 64)])
def test_elu2(Fd, L):
    rows_n, XW = 5, Fd + 4 * L                           # y is the head of an xin row; dy comes from a dxin row
    g = torch.Generator().manual_seed(Fd)
    a, dy = 1.5 * rnd(g, rows_n, Fd), rnd(g, rows_n, XW)
    assert bool((a > 0).any()) and bool((a < 0).any())
    y_ref, da_ref = R.elu2(a, dy[:, :Fd])
    y = torch.full((rows_n, XW), SENTINEL, device="cuda")
    y[:, :Fd] = NAN
    da = nans(rows_n, Fd)
    ok(lib().ocrl_iodine_elu2(P(dev(a)), Fd, P(y), XW, rows_n, Fd, None, 0, stream()))
    ok(lib().ocrl_iodine_elu2(P(dev(a)), Fd, P(da), Fd, rows_n, Fd, P(dev(dy)), XW, stream()))
    torch.cuda.synchronize()
    assert bool((y[:, Fd:] == SENTINEL).all())
    grade(f"elu2 F{Fd} XW{XW}", [("y", y[:, :Fd], y_ref, TOL), ("da", da, da_ref, TOL)])


@pytest.mark.parametrize("rows_n", [1, 7])
@pytest.mark.parametrize("H", [64, 256])
def test_lstm(H, rows_n):
    g = torch.Generator().manual_seed(H + rows_n)
    gates, c0, dh1, dc1 = 1.5 * rnd(g, rows_n, 4 * H), rnd(g, rows_n, H), rnd(g, rows_n, H), rnd(g, rows_n, H)
    acts, c1, h1 = nans(rows_n, 4 * H), nans(rows_n, H), nans(rows_n, H)
    ok(lib().ocrl_iodine_lstm(P(dev(gates)), P(dev(c0)), P(acts), P(c1), P(h1), None, None, None, None, rows_n, H, 0, stream()))
    torch.cuda.synchronize()
    ref = R.lstm(gates, c0, dh1, dc1)
    rows = [("acts", acts, ref[0], TOL), ("c1", c1, ref[1], TOL), ("h1", h1, ref[2], TOL)]
    for use_h in (True, False):
        for use_c in (True, False):
            ref = R.lstm(gates, c0, dh1 if use_h else None, dc1 if use_c else None)
            dg, dc0 = nans(rows_n, 4 * H), nans(rows_n, H)
            # the backward reads the saved activations and cell state: the reference's, rounded to fp32
            ok(lib().ocrl_iodine_lstm(None, P(dev(c0)), P(dev(ref[0])), P(dev(ref[1])), None, P(dev(dh1)) if use_h else None,
                                      P(dev(dc1)) if use_c else None, P(dg), P(dc0), rows_n, H, 1, stream()))
            torch.cuda.synchronize()
            t = f"dh{int(use_h)}dc{int(use_c)}"
            rows += [(f"{t}:dgates", dg, ref[3], TOL), (f"{t}:dc0", dc0, ref[4], TOL)]
    grade(f"lstm H{H} rows{rows_n}", rows)


# ------------------------------------------------------------------------------------------------------------------- 64 -> 4 convolution
def c4_inputs(S, Bn, co_n, elu):
    g = torch.Generator().manual_seed(S * 10 + Bn)
    X, W, bias, dY = rnd(g, Bn, S, S, 64), rnd(g, co_n, 64, 3, 3) / 24.0, rnd(g, 4), rnd(g, Bn, S, S, 4)
    pre = rnd(g, Bn, S, S, 64)
    return X, W, bias, dY, (F.elu(pre) if elu else F.relu(pre))


def run_c4(W, co_n, bias, X, act, Y, Bn, S, mode, elu):
    n = lib().ocrl_bcdec_c4_ws_floats()
    ws = nans(n)
    ok(lib().ocrl_bcdec_c4(P(W), co_n, P(bias), P(X), P(act), P(Y), Bn, S, mode, elu, P(ws), n, stream()))
    torch.cuda.synchronize()


def fold_wgrad(X, dY, Bn, S, form):
    nb = lib().ocrl_bcdec_c4_wgrad_blocks(Bn, S)
    tiles = -(-S // 32) * -(-S // 4) * Bn
    assert nb == min(tiles, 1024)
    part = nans(nb, 4, 64, 9)
    ok(lib().ocrl_bcdec_c4_wgrad(P(X), P(dY), P(part), part.numel(), Bn, S, form, stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part).all())
    return part.double().sum(dim=0).reshape(4, 64, 3, 3), nb, tiles


@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("S", [16, 20, 32, 48, 64])          # the tile is 4 x 32: 20 and 48 are ragged in x, 16 is narrower than a tile
def test_c4_conv(S, Bn):
    rows = []
    for co_n in (3, 4):
        for elu in (0, 1):
            X, W, bias, dY, act = c4_inputs(S, Bn, co_n, elu)
            Y_ref, dX_ref, dW_ref = R.c4(X, W, bias, dY, act, elu)
            # W is followed by NaN: with co_n = 3 the pack must not read a fourth output channel
            Wd = torch.cat((dev(W).flatten(), nans(64 * 9)))
            t = f"co{co_n} {'elu' if elu else 'relu'}"
            if elu == 0:
                Y = nans(Bn, S, S, 4)
                run_c4(Wd, co_n, dev(bias), dev(X), None, Y, Bn, S, 0, 0)
                rows.append((f"{t}:Y", Y, Y_ref, TOL))
                if co_n == 3:
                    assert bool((Y[..., 3] == bias[3].item()).all())         # zero weights: the bias alone
            dX = nans(Bn, S, S, 64)
            run_c4(Wd, co_n, None, dev(dY), dev(act), dX, Bn, S, 1, elu)
            rows.append((f"{t}:dX", dX, dX_ref, TOL))
            if co_n == 4 and elu == 0:
                for form, name in ((1, "valu"), (2, "mfma"), (0, "switch")):
                    dW, nb, tiles = fold_wgrad(dev(X), dev(dY), Bn, S, form)
                    rows.append((f"dW:{name}({nb} blocks)", dW, dW_ref, TOL))
    grade(f"c4 S{S} B{Bn}", rows)


def test_c4_wgrad_beyond_the_block_cap():
    """Bn = 33, S = 64: 1056 tiles on the capped grid of 1024, so 32 blocks take a second tile in the stride loop of either form"""
    Bn, S = 33, 64
    g = torch.Generator().manual_seed(33)
    X, dY = rnd(g, Bn, S, S, 64), rnd(g, Bn, S, S, 4)
    Xr = X.double().permute(0, 3, 1, 2)
    W = torch.zeros(4, 64, 3, 3, dtype=torch.float64, requires_grad=True)
    (dW_ref,) = torch.autograd.grad((F.conv2d(Xr, W, padding=1) * dY.double().permute(0, 3, 1, 2)).sum(), W)
    Xd, dYd = dev(X), dev(dY)
    rows = []
    for form, name in ((1, "valu"), (2, "mfma")):
        dW, nb, tiles = fold_wgrad(Xd, dYd, Bn, S, form)
        assert (nb, tiles) == (1024, 1056)
        rows.append((f"dW:{name}", dW, dW_ref, TOL))
    grade("c4 wgrad 1056 tiles", rows)


# ------------------------------------------------------------------------------------------------------------------- mixture, compose
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [16, 48])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 7, 16])
def test_mix(K, C, S, B):
    g = torch.Generator().manual_seed(K * 100 + C * 10 + S + B)
    out4 = torch.cat((torch.rand(B, K, S, S, 3, generator=g) * 1.6 - 0.3, rnd(g, B, K, S, S, 1)), dim=-1)
    obs = torch.rand(B, C, S, S, generator=g)
    recon_ref, loss_ref, d_ref = R.mix(out4, obs)
    n = lib().ocrl_bcdec_mix_ws_floats()
    got = {}
    for want_r, want_d in ((True, True), (False, True), (True, False), (False, False)):
        recon, d, loss, ws = (nans(B, S, S, 4) if want_r else None), (nans(B, K, S, S, 4) if want_d else None), nans(1), nans(n)
        ok(lib().ocrl_bcdec_mix(P(dev(out4)), P(dev(obs)), P(recon), P(d), P(loss), B, K, S, C, P(ws), n, stream()))
        torch.cuda.synchronize()
        if not got:
            got = dict(recon=recon, d=d, loss=loss)
            continue
        assert torch.equal(loss, got["loss"]) and (recon is None or torch.equal(recon, got["recon"])) and (d is None or torch.equal(d, got["d"]))
    assert bool((got["recon"][..., 3] == 0).all())
    grade(f"mix K{K} C{C} S{S} B{B}", [("loss", got["loss"][0], loss_ref, TOL), ("recon", got["recon"][..., :3], recon_ref, TOL),
                                       ("d_rgb", got["d"][..., :3], d_ref[..., :3], TOL), ("d_logit", got["d"][..., 3], d_ref[..., 3], TOL)])


@pytest.mark.parametrize("D", [64, 192])
def test_compose(D):
    g = torch.Generator().manual_seed(D)
    W1, Wpos, bpos = rnd(g, 64, D, 5, 5) / math.sqrt(25 * D), rnd(g, D, 4) / 2, rnd(g, D) / 2
    dWc, dW1r = rnd(g, 25, 64, 5), rnd(g, 25, 64, D)
    Wc_ref, W1r_ref = R.compose(W1, Wpos, bpos)
    ref = R.compose_bwd(W1, Wpos, bpos, dWc, dW1r)
    Wc, W1r, dW1, dWpos, dbpos = nans(25, 64, 5), nans(25, 64, D), nans(64, D, 5, 5), nans(D, 4), nans(D)
    a = [dev(v) for v in (W1, Wpos, bpos)]
    ok(lib().ocrl_bcdec_compose(P(a[0]), P(a[1]), P(a[2]), P(Wc), P(W1r), D, stream()))
    ok(lib().ocrl_bcdec_compose_bwd(P(a[0]), P(a[1]), P(a[2]), P(dev(dWc)), P(dev(dW1r)), P(dW1), P(dWpos), P(dbpos), D, stream()))
    torch.cuda.synchronize()
    assert torch.equal(W1r.cpu().double(), W1r_ref.float().double())                             # a transposed copy
    grade(f"compose D{D}", [("Wc", Wc, Wc_ref, TOL), ("dW1", dW1, ref[0], TOL), ("dWpos", dWpos, ref[1], TOL), ("dbpos", dbpos, ref[2], TOL)])
