"""The clip + Adam update (csrc/optim.hip absmax / clip_adam kernels, csrc/iodine.hip io_l2norm, the per-group dispatch of
SlateModel::clip_adam / IodineModel::clip_adam, FusedAdam) against tests/optim_ref.py: fp64 Adam fed the SAME fp32 gradient, moments,
parameters and step count.  What is left between the two sides is the kernel's own fp32 rounding, so the bars are derived, not measured.

The whole-path update tests (test_gpu_slate.py, test_gpu_iodine.py, ...) run at the learning rates of warm-up steps 0..2, where the
encoder and decoder groups move by <= 3e-8 per step: they do not constrain those groups' update.  Here every case uses learning rates
at which a step is visible (1e-3 .. 4e-3 planted, 9e-5 / 2.7e-4 / 3e-4 from the schedule at step 40000) and grades the update
p_new - p_old itself, not the parameter.

Bars, u = 2^-24 (default hipcc flags: correctly rounded fp32 divide and sqrt; FMA contraction only removes roundings).  With
g' = coef * gscale * g the clipped gradient as the reference has it:
  m   |m_hip - m_ref| <= 4u (|m_old| + |g'|).  m_new = m + (g' - m)(1 - b1): g' carries the roundings of coef (norm * gscale, + 1e-6,
      the divide, * gscale) and of g * coef, then one each for the difference, the product with fl(1 - b1) and the sum; the bound is on
      the terms because the difference form cancels when g' ~ m.
  v   |v_hip - v_ref| <= 6u v_ref while coef = 1, 10u v_ref once the clip bites.  v * fl(b2) + fl(1 - b2) g' g': every term is
      non-negative, no cancellation.  The casts of b2 and 1 - b2, three products and the sum give < 4u on exact g'; the count of 6u
      holds there.  It missed that g' enters SQUARED: with coef < 1, g' carries the roundings of the + 1e-6, of the divide and of
      g * coef (3u; norm * gscale and * gscale are exact for the power-of-two scales used here), which the square doubles:
      3.8u + 2 * 3u < 10u.  A plain fp32 evaluation of the formula on the CPU reaches 7.3u on these inputs.
  Both bounds carry an absolute floor of 4 x 2^-149.  The count above is relative and holds for normal results only; the real
      gradients of a backward pass (coef ~ 2e-4 on entries down to 1e-38) put 0.1 g' and 0.001 g'^2 into the sub-normal range, where
      a correctly rounded result is off by up to half a sub-normal spacing (2^-150) whatever its size.  At most four results of either
      chain can underflow.  A kernel that flushed them to zero would be off by up to 2^-126 and fails the floor.  The first run of
      test_slate_real_gradients_at_real_learning_rates found this (|v_hip - v_ref| = v_ref where v_ref < 2^-150); the planted cases
      keep every intermediate normal.
  dp  for the update dp = p_new - p_old: |dp_hip - dp_ref| <= 32u |dp_ref| + 4u lr + ulp(p)/2.  The chain is coef, m, v, sqrt, two
      divides, the eps add, the step product and the casts of bc1 and sqrt(bc2): a dozen roundings, 32u leaves a factor of two to
      three.  4u lr covers the cancellation case of m (|m_hat / denom| <= ~1 per unit of the bound on m).  The last term is the store
      of p: half an ulp of the stored value, taken at the larger of |p_old| and |p_new| (the sum can cross into the next binade).
  trajectory over n steps: the sum of the n single-step bounds along the reference trajectory (errors in m and v decay with b1, b2,
      so this over-estimates).
  norm: the inf-norm is a maximum of fp32 values and has no rounding: exact.  The L2 norm: 1e-5 relative, the project's bar for it.
The bounds assume that 1 - beta and the bias corrections 1 - beta^t are the decimal betas' (0.9, 0.999) values rounded once.  The
kernel used to form 1.f - 0.999f (1.3e-5 off 0.001: the rounding of 0.999f is small against 1 but 2^-14 of the difference) and
1 - (double)0.999f^t; the single-step v and dp cases of this file caught both (v off by 216u at every t, dp by ~100u at t <= 1000).

Every case plants values only in elements that belong to a tensor and asserts the alignment gaps bit-identical afterwards in p, m
and v.  One exception, stated in test_nan_and_inf_gradients: with a NaN norm the coefficient is NaN and the kernel, which sweeps a
group's whole range, writes 0 * NaN into the gaps of that group too; no kernel reads a gap as data.

The worst observed ratio to each bound is logged (tests.gpu_util.log) and recorded in DESIGN.md section 4."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import iodine_oracle as IO
from oracle import slate_oracle as O
from tests.gpu_util import dims_from_cfg, load_params, log
from tests.optim_ref import ref_step
from tests.test_gpu_iodine import TINY, dims as io_dims
from tests.test_gpu_slate import BC, SMALL, V4096, dev_noise

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SUBNORMAL = 4 * 2.0 ** -149          # absolute floor of the m and v bounds: gradual underflow (module docstring)
LRS = (1e-3, 2e-3, 4e-3)                 # distinct per group: a tensor filed under the wrong group moves by the wrong amount
TWO_TRIPS = 4 * 256 * 1024 + 4           # floats beyond which absmax_kernel's grid-stride loop (1024 blocks x 256 float4) takes a second trip
_ENGINES = {}


# ------------------------------------------------------------------------------------------------------------------ engines
def slate_engine(tag, over, B=2):
    if tag not in _ENGINES:
        from ocrl_amd.engine import SlateEngine
        cfg = O.default_cfg(**over)
        _ENGINES[tag] = (cfg, SlateEngine(dims_from_cfg(cfg), max_batch=B))
    cfg, eng = _ENGINES[tag]
    reset(eng, O.formula_params(cfg))
    return cfg, eng


def iodine_engine(B=2):
    if "iodine" not in _ENGINES:
        from ocrl_amd.engine import IodineEngine
        cfg = IO.default_cfg(**TINY)
        _ENGINES["iodine"] = (cfg, IodineEngine(io_dims(cfg), max_batch=B))
    cfg, eng = _ENGINES["iodine"]
    reset(eng, IO.formula_params(cfg))
    return cfg, eng


def reset(eng, P):
    for f in (eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v):
        f.zero_()
    load_params(eng, P)
    eng.adam_step = 0


def slate_groups(cfg, eng):
    """(offset, numel, group) per engine tensor, the group taken from the oracle's own param_shapes(cfg) by name"""
    grp = {n: g for n, _, g, tr in O.param_shapes(cfg) if tr}
    assert sorted(grp) == sorted(p.name for p in eng.params)
    return [(p.offset, p.numel, grp[p.name]) for p in eng.params]


def iodine_groups(cfg, eng):
    names = [n for n, _, _ in IO.param_shapes(cfg)]
    assert names == [p.name for p in eng.params]
    return [(p.offset, p.numel, 0) for p in eng.params]


def iodine_live(cfg, eng):
    """slot_init never receives a gradient in the reference (not trainable there): torch's Adam skips it"""
    tr = {n: t for n, _, t in IO.param_shapes(cfg)}
    live = [tr[p.name] for p in eng.params]
    assert live.count(False) == 1 and not tr["slot_init"]
    return live


def mask_of(eng, tensors, sel=None):
    """bool [flat_size]: the elements of the (selected) tensors; everything else is an alignment gap or an unselected tensor"""
    mk = torch.zeros(eng.flat_size, dtype=torch.bool)
    for i, (o, n, _) in enumerate(tensors):
        if sel is None or sel[i]:
            mk[o:o + n] = True
    return mk


def lr_elements(eng, tensors, lrs):
    lr = torch.zeros(eng.flat_size, dtype=torch.float64)
    for o, n, g in tensors:
        lr[o:o + n] = float(lrs[g])
    return lr


# ------------------------------------------------------------------------------------------------------------------ planting
def make_grad(eng, tensors, seed, live=None, scale=1.0):
    """flat fp32 gradient: per tensor, signed log-uniform magnitudes over 1e-12 .. 1e2, the first eighth exact zeros, the second
    eighth |g| in 1e-10 .. 1e-6 (where at t = 1 eps is comparable to sqrt(v) / sqrt(bc2): a misplaced eps shows there); zero in
    the gaps and in tensors without a gradient"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.zeros(eng.flat_size, dtype=torch.float32)
    for i, (o, n, _) in enumerate(tensors):
        mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 14 - 12)
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        small = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 4 - 10)
        a = n // 8
        mag[:a] = 0.0
        mag[a:2 * a] = small[a:2 * a]
        if live is None or live[i]:
            g[o:o + n] = (sign * mag * scale).float()
    return g


def make_moments(eng, tensors, seed, sel=None):
    """planted Adam state: m signed log-uniform over 1e-12 .. 1e1 with its block of exact zeros at the END of each tensor (so zero
    gradients meet non-zero moments and the other way round), v >= 0 of the order of m^2 (the step stays of the order of lr) and
    non-zero where m is zero"""
    gen = torch.Generator().manual_seed(seed + 1000)
    m = torch.zeros(eng.flat_size, dtype=torch.float32)
    v = torch.zeros(eng.flat_size, dtype=torch.float32)
    for i, (o, n, _) in enumerate(tensors):
        mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 13 - 12)
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        lone = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 10 - 10)
        spread = 0.5 + 1.5 * torch.rand(n, generator=gen, dtype=torch.float64)
        a = n // 8
        mag[n - a:] = 0.0
        if sel is None or sel[i]:
            m[o:o + n] = (sign * mag).float()
            v[o:o + n] = torch.where(mag == 0, lone ** 2, mag ** 2 * spread).float()
    return m, v


def plant(eng, tensors, g=None, m=None, v=None):
    """write into the tensors' elements only: the gaps keep whatever they held"""
    mk = mask_of(eng, tensors)
    for flat, new in ((eng.flat_g, g), (eng.flat_m, m), (eng.flat_v, v)):
        if new is not None:
            cur = flat.cpu()
            cur[mk] = new[mk]
            flat.copy_(cur)
    torch.cuda.synchronize()


def snap(eng):
    torch.cuda.synchronize()
    return NS(p=eng.flat_p.cpu().clone(), g=eng.flat_g.cpu().clone(), m=eng.flat_m.cpu().clone(), v=eng.flat_v.cpu().clone())


def bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ bounds
def step_bounds(before_p, before_m, g, r, lr_el, gscale):
    """single-step bounds (module docstring) from the reference's own values; all fp64 [flat_size]"""
    gp = g.double() * gscale * float(r.coef)
    bm = 4 * U * (before_m.double().abs() + gp.abs())
    bm = bm + SUBNORMAL * (bm != 0)          # no floor where m_old = g' = 0: the result is an exact zero
    cv = 6 if float(r.coef) == 1.0 else 10
    bv = cv * U * r.v + SUBNORMAL * (r.v != 0)
    dp = r.p - before_p.double()
    big = torch.maximum(before_p.double().abs(), r.p.abs()).float().numpy()
    ulp = torch.from_numpy(np.spacing(big).astype(np.float64))
    bp = 32 * U * dp.abs() + 4 * U * lr_el + ulp / 2
    return NS(m=bm, v=bv, p=bp, cv=cv)


def ratio(err, bound, mk):
    """max err / bound over the masked elements; a zero bound demands a zero error"""
    e, b = err[mk], bound[mk]
    assert bool((e[b == 0] == 0).all()), "non-zero error where the bound is zero"
    nz = b > 0
    return float((e[nz] / b[nz]).max()) if bool(nz.any()) else 0.0


def check(tag, eng, before, after, r, bnd, live_mk, base_p=None):
    """after (HIP) against r (fp64 reference): everything outside the live tensors' elements bit-identical to before in p, m, v; the
    live elements inside the bounds.  base_p: fp64 start of the update on the reference side (default before.p)"""
    rest = ~live_mk
    for k in ("p", "m", "v"):
        a, b = getattr(after, k), getattr(before, k)
        assert torch.equal(bits(a)[rest], bits(b)[rest]), f"{tag}: {k} changed outside the tensors that have a gradient (gaps included)"
    assert torch.equal(bits(after.g), bits(before.g)), f"{tag}: the step wrote to the gradient buffer"
    base_p = before.p.double() if base_p is None else base_p
    rm = ratio((after.m.double() - r.m).abs(), bnd.m, live_mk)
    rv = ratio((after.v.double() - r.v).abs(), bnd.v, live_mk)
    rp = ratio(((after.p.double() - before.p.double()) - (r.p - base_p)).abs(), bnd.p, live_mk)
    moved = float(((after.p != before.p) & live_mk).sum()) / max(1, int(live_mk.sum()))
    log(f"[optim {tag}] worst error / bound: m {rm:.3f} v {rv:.3f} (x {getattr(bnd, 'cv', 0)}u) dp {rp:.3f}; norm {float(r.norm):.6e} coef {float(r.coef):.6e}; {100 * moved:.1f}% of the live elements moved")
    assert rm <= 1.0 and rv <= 1.0 and rp <= 1.0, (tag, rm, rv, rp)
    return rm, rv, rp


def run_step(eng, lrs, clip, gscale, t):
    eng.adam_step = t - 1
    eng.clip_adam(lrs, clip, gscale)
    torch.cuda.synchronize()
    assert eng.adam_step == t
    return float(eng.metrics[3])


def one_step(tag, eng, tensors, lrs, clip, norm_type, gscale, t, live=None):
    """snapshot -> HIP step -> fp64 reference step from the same fp32 inputs -> check; returns the reference result"""
    before = snap(eng)
    norm_hip = run_step(eng, lrs if norm_type == "inf" else lrs[0], clip, gscale, t)
    after = snap(eng)
    r = ref_step(before.p, before.g, before.m, before.v, tensors, lrs, clip, norm_type, t, gscale, live)
    check_norm(tag, norm_hip, before.g, r, norm_type, gscale)
    bnd = step_bounds(before.p, before.m, before.g, r, lr_elements(eng, tensors, lrs), gscale)
    check(tag, eng, before, after, r, bnd, mask_of(eng, tensors, live))
    return r


def check_norm(tag, norm_hip, g, r, norm_type, gscale):
    """the engine reports the norm of the unscaled gradient (the Python surface multiplies by the scale); the clip compares the scaled one"""
    if norm_type == "inf":
        assert norm_hip == float(g.abs().max()), (tag, norm_hip, float(g.abs().max()))          # a maximum has no rounding
        assert norm_hip * gscale == float(r.norm), (tag, norm_hip, gscale, float(r.norm))
    else:
        e = abs(norm_hip * gscale - float(r.norm)) / float(r.norm)
        log(f"[optim {tag}] L2 norm rel err {e:.2e}")
        assert e < 1e-5, (tag, norm_hip, float(r.norm))


# ------------------------------------------------------------------------------------------------------------------ single step
CLIPS_INF = {"off": 0.0, "above": 1.0e3, "below": 0.05}          # planted |g|max ~ 1e2 (x gscale): coef exactly 1, then coef ~ 5e-4 .. 1e-3
CLIPS_L2 = {"off": 0.0, "above": 1.0e7, "below": 5.0}            # planted ||g||_2 ~ 1e4


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("clipmode", ["off", "above", "below"])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_slate_single_step_from_planted_state(t, clipmode, gscale):
    cfg, eng = slate_engine("v4096", V4096)
    assert eng.flat_size > TWO_TRIPS, eng.flat_size
    tensors = slate_groups(cfg, eng)
    g = make_grad(eng, tensors, seed=t)
    m, v = make_moments(eng, tensors, seed=t) if t > 1 else (None, None)
    plant(eng, tensors, g, m, v)
    r = one_step(f"slate t={t} clip={clipmode} gscale={gscale}", eng, tensors, LRS, CLIPS_INF[clipmode], "inf", gscale, t)
    if clipmode == "below":
        assert 0.0 < float(r.coef) < 1.0
    else:
        assert float(r.coef) == 1.0


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("clipmode", ["off", "above", "below"])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_iodine_single_step_from_planted_state(t, clipmode, gscale):
    cfg, eng = iodine_engine()
    tensors, live = iodine_groups(cfg, eng), iodine_live(cfg, eng)
    g = make_grad(eng, tensors, seed=50 + t, live=live)
    m, v = make_moments(eng, tensors, seed=50 + t) if t > 1 else (None, None)          # slot_init's state is planted too: it must not move
    plant(eng, tensors, g, m, v)
    r = one_step(f"iodine t={t} clip={clipmode} gscale={gscale}", eng, tensors, (3e-3,), CLIPS_L2[clipmode], 2, gscale, t, live)
    if clipmode == "below":
        assert 0.0 < float(r.coef) < 1.0
    else:
        assert float(r.coef) == 1.0


# ------------------------------------------------------------------------------------------------------------------ groups and skips
def test_slate_default_config_groups():
    """the default configuration (64x64, vocabulary 4096, four decoder blocks): every tensor moves by its own group's learning rate"""
    cfg, eng = slate_engine("default", {}, B=1)
    tensors = slate_groups(cfg, eng)
    assert [g for _, _, g in tensors] == [p.group for p in eng.params]
    assert [eng.group_begin[g] for g in range(3)] == [min(o for o, _, gg in tensors if gg == g) for g in range(3)]
    m, v = make_moments(eng, tensors, seed=7)
    plant(eng, tensors, make_grad(eng, tensors, seed=7), m, v)
    one_step("slate default groups", eng, tensors, LRS, 0.05, "inf", 1.0, 3)


def test_slate_bcdec_skips_groups_0_and_2():
    """use_bcdec: only the slot-attention group has gradients (the dVAE and the transformer decoder are not part of the loss); the
    slot projection sits in that group without a gradient and, as in a real run, with zero Adam state"""
    cfg, eng = slate_engine("bcdec", BC)
    tensors = slate_groups(cfg, eng)
    live = [g == 1 and p.name != "_slotproj.weight" for p, (_, _, g) in zip(eng.params, tensors)]
    state = [p.name != "_slotproj.weight" for p in eng.params]          # groups 0 and 2 carry planted state: it must come back bit for bit
    m, v = make_moments(eng, tensors, seed=8, sel=state)
    plant(eng, tensors, make_grad(eng, tensors, seed=8, live=live), m, v)
    before = snap(eng)
    one_step("slate bcdec", eng, tensors, LRS, 0.05, "inf", 1.0, 3, live)
    after = snap(eng)
    for (o, n, g), h in zip(tensors, live):
        same = all(torch.equal(bits(getattr(after, k))[o:o + n], bits(getattr(before, k))[o:o + n]) for k in ("p", "m", "v"))
        assert same == (not h), (o, n, g, h)          # groups 0 and 2 (and the slot projection) bit-identical, every other tensor moved


def test_slate_encoder_only_update():
    """encode -> encode_backward -> clip_adam: exactly the tensors that receive a gradient in that mode move (the CNN encoder, its
    position embedding and the slot-attention module: group 1 up to the slot projection, csrc/slate_model.cpp SlateModel::clip_adam)"""
    cfg, eng = slate_engine("small encoder-only", SMALL)          # its own engine: the mode lasts until the next full backward()
    tensors = slate_groups(cfg, eng)
    B = 2
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(3)).cuda()
    eng.encode(obs, seed=5)
    ds = torch.randn(B, cfg.num_slots, cfg.slot_size, generator=torch.Generator().manual_seed(4)).cuda()
    eng.encode_backward(ds)
    torch.cuda.synchronize()
    g0 = eng.flat_g.cpu()
    live = [bool((g0[o:o + n] != 0).any()) for o, n, _ in tensors]
    expect = [p.name.startswith(("_enc.", "_enc_pos.", "_slotattn.")) for p in eng.params]
    assert live == expect, [p.name for p, a, b in zip(eng.params, live, expect) if a != b]
    assert all(g == 1 for (_, _, g), h in zip(tensors, live) if h)
    assert float(g0[~mask_of(eng, tensors, live)].abs().max()) == 0.0
    m, v = make_moments(eng, tensors, seed=9)
    plant(eng, tensors, make_grad(eng, tensors, seed=9, live=live), m, v)
    one_step("slate encoder-only", eng, tensors, LRS, 0.05, "inf", 1.0, 3, live)


def test_iodine_slot_init_is_skipped():
    cfg, eng = iodine_engine()
    tensors, live = iodine_groups(cfg, eng), iodine_live(cfg, eng)
    m, v = make_moments(eng, tensors, seed=10)
    plant(eng, tensors, make_grad(eng, tensors, seed=10, live=live), m, v)
    before = snap(eng)
    one_step("iodine slot_init", eng, tensors, (3e-3,), 5.0, 2, 1.0, 3, live)
    after = snap(eng)
    q = next(p for p in eng.params if p.name == "slot_init")
    assert float(before.m[q.offset:q.offset + q.numel].abs().max()) > 0          # there was state to disturb
    for k in ("p", "m", "v"):
        assert torch.equal(bits(getattr(after, k))[q.offset:q.offset + q.numel], bits(getattr(before, k))[q.offset:q.offset + q.numel])
    lo, hi = after.p[:q.offset] != before.p[:q.offset], after.p[q.offset + q.numel:] != before.p[q.offset + q.numel:]
    assert bool(lo.any()) and bool(hi.any())          # both ranges around it moved


# ------------------------------------------------------------------------------------------------------------------ trajectory
def trajectory(tag, eng, tensors, lrs, clip, norm_type, live, scales):
    """free-running: both sides carry their own p, m, v; a fresh planted gradient each step.  Bound after k steps: the sum of the
    single-step bounds along the reference trajectory."""
    lr_el = lr_elements(eng, tensors, lrs)
    live_mk = mask_of(eng, tensors, live)
    start = snap(eng)
    ref = NS(p=start.p.double(), m=start.m.double(), v=start.v.double())
    acc = NS(m=torch.zeros(eng.flat_size, dtype=torch.float64), v=0, p=torch.zeros(eng.flat_size, dtype=torch.float64))
    coefs, worst = [], [0.0, 0.0, 0.0]
    for k, sc in enumerate(scales):
        t = k + 1
        plant(eng, tensors, make_grad(eng, tensors, seed=100 + k, live=live, scale=sc))
        g = eng.flat_g.cpu().clone()
        eng.clip_adam(lrs if norm_type == "inf" else lrs[0], clip)
        assert eng.adam_step == t
        r = ref_step(ref.p, g, ref.m, ref.v, tensors, lrs, clip, norm_type, t, 1.0, live)
        b = step_bounds(ref.p, ref.m, g, r, lr_el, 1.0)
        # v's bound is relative: the steps' factors add up, relative to the new v (a sum of non-negative terms)
        acc = NS(m=acc.m + b.m, p=acc.p + b.p, v=acc.v + b.cv)
        now = snap(eng)
        bnd = NS(m=acc.m, v=acc.v * U * r.v + t * SUBNORMAL * (r.v != 0), p=acc.p)
        rest = ~live_mk
        for key in ("p", "m", "v"):
            assert torch.equal(bits(getattr(now, key))[rest], bits(getattr(start, key))[rest]), (tag, t, key)
        rm = ratio((now.m.double() - r.m).abs(), bnd.m, live_mk)
        rv = ratio((now.v.double() - r.v).abs(), bnd.v, live_mk)
        rp = ratio((now.p.double() - r.p).abs(), bnd.p, live_mk)
        worst = [max(a, c) for a, c in zip(worst, (rm, rv, rp))]
        assert rm <= 1.0 and rv <= 1.0 and rp <= 1.0, (tag, t, rm, rv, rp)
        coefs.append(float(r.coef))
        ref = NS(p=r.p, m=r.m, v=r.v)
    log(f"[optim {tag}] {len(scales)} free-running steps: worst error / accumulated bound: m {worst[0]:.3f} v {worst[1]:.3f} p {worst[2]:.3f}; "
        f"{sum(c < 1.0 for c in coefs)} steps clipped, {sum(c == 1.0 for c in coefs)} did not")
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)


def test_slate_trajectory_20_steps():
    cfg, eng = slate_engine("small", SMALL)
    tensors = slate_groups(cfg, eng)
    scales = [1.0 if k % 3 else 1e-4 for k in range(20)]          # |g|max ~ 1e2 or ~ 1e-2 against the clip of 0.05
    trajectory("slate trajectory", eng, tensors, LRS, 0.05, "inf", None, scales)


def test_iodine_trajectory_20_steps():
    cfg, eng = iodine_engine()
    tensors, live = iodine_groups(cfg, eng), iodine_live(cfg, eng)
    scales = [1.0 if k % 3 else 1e-5 for k in range(20)]          # ||g||_2 ~ 1e4 or ~ 0.1 against the clip of 5.0
    trajectory("iodine trajectory", eng, tensors, (3e-3,), 5.0, 2, live, scales)


# ------------------------------------------------------------------------------------------------------------------ real gradients
@pytest.mark.parametrize("tag,over", [("small", SMALL), ("bcdec", BC)])
def test_slate_real_gradients_at_real_learning_rates(tag, over):
    """forward + backward at steps 40000..40002 (warm-up over: lr_enc ~ 9e-5, lr_dec ~ 2.7e-4), the step graded on the very gradient the
    backward left in flat_g"""
    cfg, eng = slate_engine(tag, over)
    tensors = slate_groups(cfg, eng)
    live = [g == 1 and p.name != "_slotproj.weight" for p, (_, _, g) in zip(eng.params, tensors)] if cfg.use_bcdec else None
    B = 2
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(9))
    for k, step in enumerate((40000, 40001, 40002)):
        noise = O.make_noise(cfg, B, 20 + k)
        tau, lrs = O.schedules(cfg, step)
        assert 8e-5 < lrs[1] < 1e-4 and 2.4e-4 < lrs[2] < 3e-4
        dn = dict(slots=noise["slots"].cuda()) if cfg.use_bcdec else dev_noise(cfg, noise)
        eng.forward(obs.cuda(), tau, train=False, seed=step, noise=dn)
        eng.backward()
        torch.cuda.synchronize()
        if live is not None:
            g0 = eng.flat_g.cpu()
            assert float(g0[~mask_of(eng, tensors, live)].abs().max()) == 0.0
        one_step(f"slate {tag} real step {step}", eng, tensors, lrs, cfg.clip, "inf", 1.0, k + 1, live)


def test_iodine_real_gradients_at_real_learning_rate():
    cfg, eng = iodine_engine()
    tensors, live = iodine_groups(cfg, eng), iodine_live(cfg, eng)
    B = 2
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(5))
    for k in range(3):
        eps = IO.make_noise(cfg, B, 50 + k)
        eng.forward(obs.cuda(), seed=k, noise=eps.cuda())
        eng.backward()
        torch.cuda.synchronize()
        one_step(f"iodine real step {k}", eng, tensors, (cfg.lr,), cfg.clip, 2, 1.0, k + 1, live)


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_slate_python_surface_update():
    """ocrs.SLATE.update at step 40000 and 40001: FusedAdam.step, the schedule wiring and the adam_step bookkeeping"""
    import os
    from ocrl_amd import ocrs
    from ocrl_amd.utils.config import compose
    from train_ocr import ROOT
    c = compose(os.path.join(ROOT, "configs"), "train_ocr", ["ocr=slate", "ocr.dvae.vocab_size=256", "ocr.tfdec.num_dec_blocks=1",
                                                              "dataset=random-N5C4S4S2", "dataset.obs_size=16"])
    ln = c.ocr.learning
    cfg = O.default_cfg(obs_size=16, vocab_size=256, num_dec_blocks=1, num_slots=int(c.ocr.slotattr.num_slots), num_iterations=int(c.ocr.slotattr.num_iterations),
                        lr_half_life=ln.lr_half_life, lr_dvae=ln.lr_dvae, lr_enc=ln.lr_enc, lr_dec=ln.lr_dec, lr_warmup_steps=ln.lr_warmup_steps, clip=ln.clip)
    B = 2
    obs = torch.rand(B, 3, 16, 16, device="cuda")
    model = ocrs.SLATE(c.ocr, c.dataset)
    model.to("cuda:0")
    model.train()
    model._module._ensure_engine(B)
    eng = model._module.engine
    tensors = slate_groups(cfg, eng)
    lr_seen = []
    for k, step in enumerate((40000, 40001)):
        before = snap(eng)
        met = model.update(obs, None, step)
        assert model._module.engine is eng and eng.adam_step == k + 1
        after = snap(eng)
        before.g = after.g          # clip_adam does not write the gradient: what is there now is what the step consumed
        lrs = [g["lr"] for g in model._opt.param_groups]
        _, want = O.schedules(cfg, step)
        for a, b in zip(lrs, want):
            assert abs(a - b) <= 1e-6 * b, (lrs, want)
        lr_seen.append(lrs)
        r = ref_step(before.p, before.g, before.m, before.v, tensors, lrs, ln.clip, "inf", k + 1)
        assert float(met["norm"]) == float(after.g.abs().max()) == float(r.norm)
        bnd = step_bounds(before.p, before.m, before.g, r, lr_elements(eng, tensors, lrs), 1.0)
        check(f"SLATE.update step {step}", eng, before, after, r, bnd, mask_of(eng, tensors))
    assert lr_seen[0][1] != lr_seen[1][1]


def test_iodine_python_surface_update():
    from ocrl_amd import ocrs
    cfg = IO.default_cfg(**TINY)
    ocr = NS(name="Iodine", slot_size=cfg.slot_size, num_iterations=cfg.num_iterations, num_slots=cfg.num_slots, img_channels=3, sigma=cfg.sigma,
             beta=cfg.beta, layer_norm=True, ref_cnn_hidden_size=64, ref_mlp_hidden_size=256, ref_cnn_layers=4, ref_cnn_kernel_size=3,
             ref_cnn_stride_size=2, dec_cnn_hidden_size=64, dec_cnn_layers=4, dec_cnn_kernel_size=3, learning=NS(lr=3e-4, clip=5.0, clip_norm_type=2.0))
    torch.manual_seed(0)
    model = ocrs.Iodine(ocr, NS(obs_size=cfg.obs_size, obs_channels=3))
    model.to("cuda:0")
    model.train()
    B, K, S = 2, cfg.num_slots, cfg.obs_size
    obs = torch.rand(B, 3, S, S, device="cuda")
    ids = torch.randint(0, K + 1, (B, S, S), device="cuda")
    masks = torch.nn.functional.one_hot(ids, K + 1).permute(0, 3, 1, 2)[:, :, None].float()
    model._module._ensure_engine(B)
    eng = model._module.engine
    tensors, live = iodine_groups(cfg, eng), iodine_live(cfg, eng)
    for k, step in enumerate((40000, 40001)):
        before = snap(eng)
        met = model.update(obs, masks, step)
        assert model._module.engine is eng and eng.adam_step == k + 1
        after = snap(eng)
        before.g = after.g
        lrs = [g["lr"] for g in model._opt.param_groups]
        assert lrs == [3e-4]
        r = ref_step(before.p, before.g, before.m, before.v, tensors, lrs, 5.0, 2, k + 1, 1.0, live)
        check_norm(f"Iodine.update step {step}", float(met["norm"]), before.g, r, 2, 1.0)
        bnd = step_bounds(before.p, before.m, before.g, r, lr_elements(eng, tensors, lrs), 1.0)
        check(f"Iodine.update step {step}", eng, before, after, r, bnd, mask_of(eng, tensors, live))


# ------------------------------------------------------------------------------------------------------------------ the norm
def test_slate_inf_norm_is_exact_at_every_position():
    cfg, eng = slate_engine("v4096", V4096)
    assert eng.flat_size > TWO_TRIPS
    tensors = slate_groups(cfg, eng)
    base = make_grad(eng, tensors, seed=11, scale=1e-3)          # |g| <= 0.1
    last = {g: max(o + n - 1 for o, n, gg in tensors if gg == g) for g in range(3)}
    far = next(o + n - 1 for o, n, _ in tensors if o + n - 1 > TWO_TRIPS + 1000)
    spots = {"first element": tensors[0][0], "last element of the last tensor": tensors[-1][0] + tensors[-1][1] - 1, "beyond two trips": far,
             **{f"last element of group {g}": i for g, i in last.items()}}
    assert spots["first element"] == 0 and far > TWO_TRIPS
    plant(eng, tensors, base)
    assert float(eng.grad_norm()) == float(base.abs().max())
    for name, i in spots.items():
        for val in (7.5, -7.5):
            g = base.clone()
            g[i] = val
            plant(eng, tensors, g)
            got = float(eng.grad_norm())
            assert got == 7.5 == float(g.abs().max()), (name, i, val, got)
    log(f"[optim norm] inf-norm exact with the maximum at {sorted(spots.values())} of {eng.flat_size}")


@pytest.mark.parametrize("model", ["slate", "iodine"])
@pytest.mark.parametrize("bad,clip", [("nan", 0.05), ("nan", 0.0), ("inf", 0.05)])
def test_nan_and_inf_gradients(model, bad, clip):
    """What clip_grad_norm_ + Adam do (tests/test_optimizer_ref_cpu.py): a NaN entry gives a NaN norm and, with the clip on, NaN in every
    updated tensor (the coefficient is NaN); with the clip off only its own element.  An inf entry gives an inf norm, coef = 0, NaN at
    that element (inf * 0) and, from a fresh state, unchanged values elsewhere.  With a NaN coefficient the kernel's sweep of a
    group's range also turns the alignment gaps inside it to NaN (0 * NaN): the gaps are compared in every other case."""
    if model == "slate":
        cfg, eng = slate_engine("small", SMALL)
        tensors, live, lrs, norm_type = slate_groups(cfg, eng), None, LRS, "inf"
        clip = clip and 0.05
    else:
        cfg, eng = iodine_engine()
        tensors, live, lrs, norm_type = iodine_groups(cfg, eng), iodine_live(cfg, eng), (3e-3,), 2
        clip = clip and 5.0
    g = make_grad(eng, tensors, seed=12, live=live)
    o, n, _ = max((tn for tn, h in zip(tensors, live or [True] * len(tensors)) if h), key=lambda tn: tn[1])
    spot = o + n // 2
    g[spot] = float(bad)
    plant(eng, tensors, g)
    before = snap(eng)
    norm_hip = run_step(eng, lrs if norm_type == "inf" else lrs[0], clip, 1.0, 1)
    after = snap(eng)
    r = ref_step(before.p, before.g, before.m, before.v, tensors, lrs, clip, norm_type, 1, 1.0, live)
    live_mk = mask_of(eng, tensors, live)
    if bad == "nan":
        assert np.isnan(norm_hip) and bool(torch.isnan(r.norm))
    else:
        assert norm_hip == float("inf") == float(r.norm) and float(r.coef) == 0.0
    for k in ("p", "m", "v"):
        a, b = getattr(after, k), getattr(r, k)
        assert torch.equal(torch.isnan(a)[live_mk], torch.isnan(b)[live_mk]), (k, int(torch.isnan(a)[live_mk].sum()), int(torch.isnan(b)[live_mk].sum()))
        assert bool(torch.isnan(a[spot]))
    if bad == "nan" and clip:
        assert bool(torch.isnan(after.p[live_mk]).all())
        if live is not None:          # a tensor without a gradient stays as it was
            rest = mask_of(eng, tensors) & ~live_mk
            for k in ("p", "m", "v"):
                assert torch.equal(bits(getattr(after, k))[rest], bits(getattr(before, k))[rest])
        return
    # one poisoned element: everything else inside the usual bounds, the gaps bit-identical
    fin = live_mk.clone()
    fin[spot] = False
    if bad == "inf":
        assert torch.equal(bits(after.p)[fin], bits(before.p)[fin])
    r.coef = torch.ones(()) if not clip else r.coef
    clean = NS(p=before.p, m=before.m, v=before.v, g=before.g)
    bnd = step_bounds(before.p, before.m, torch.where(torch.isfinite(before.g), before.g, torch.zeros(())), r, lr_elements(eng, tensors, lrs), 1.0)
    for k in ("p", "m", "v"):
        getattr(after, k)[spot] = getattr(before, k)[spot]
        getattr(r, k)[spot] = float(getattr(before, k)[spot])
    check(f"{model} {bad} clip={clip}", eng, clean, after, r, bnd, live_mk)
