"""GPU checks of A2C: ocrl_acnet_a2c_fwd_bwd and ocrl_flat_clip_rmsprop_l2 through the C ABI, ``A2C.train()``, the on-device rollout, a
learning run, checkpoints and the entry points, against the fp64 restatement of tests/a2c_ref.py.

Bounds.  The loss step carries those tests/test_gpu_acnet.py applies to the same quantities of ocrl_acnet_ppo_fwd_bwd: scalars 1e-4 with
the 1e-3 floor, dw and dfeatures 3e-4 of each gradient's maximum with the 1e-3 gmax floor.  Updates are graded on dp / lr (and the square
average itself), elementwise, against the fp64 restatement fed the same fp32 inputs; the bound is 4 x the largest deviation of the fp32
torch restatement (a2c_ref in float32) from the fp64 one on the very inputs of the test, measured on a CPU and written at RMS_DP_DEV,
RMS_SQ_DEV, TRAIN_DEV and TRAIN_ADAM_DEV below; the factor 4 is for the different summation order of the norm (and, in train(), of the
MFMA products).  The norm is held to 1e-5 relative."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import a2c_ref as A
from tests import acnet_ref as R
from tests import ppo_ref as P
from tests.gpu_util import log
from tests.test_gpu_acnet import IDENT, MLP, _acnet_cfg, err, make_params, make_x, nanlike

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# largest |dp_fp32 / lr - dp_fp64 / lr| and |sq_fp32 - sq_fp64| of the restatement over every case and step of test_rmsprop_step, set by
# the rounding of p + dp at |p| < 0.5 and lr = 7e-4 (measured on a CPU: 6.14e-5 and 1.65e-7)
RMS_DP_DEV = 6.2e-5
RMS_SQ_DEV = 1.7e-7
# the same for dp / lr over every parameter after the two updates of test_train_against_the_restatement, with RMSprop (measured on a CPU:
# 3.80e-5 of updates that reach 0.56) and with Adam (use_rms_prop=False; measured on a CPU: 4.90e-5 of updates that reach 2.0)
TRAIN_DEV = 3.8e-5
TRAIN_ADAM_DEV = 4.9e-5


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


# ------------------------------------------------------------------------------------------------------------ 1. the loss step
SHAPES = [(1, 4, 1), (5, 8, 2), (16, 8, 3), (17, 12, 3), (37, 128, 4), (64, 12, 64), (1040, 8, 4)]
LAYOUTS = {"ident": IDENT, "mlp": MLP}
VF = 0.5


@functools.lru_cache(maxsize=None)
def loss_case(B, F, A_, lname, kind="plain"):
    """(x, parameters, actions, advantages, returns) of a case on the CPU, built once.  kind: 'plain', 'outside' (actions -3 and A + 5 on the
    first two rows) or 'zeroadv' (all-zero advantages)"""
    layout = LAYOUTS[lname]
    ps, x = make_params(F, A_, layout[0], 71), make_x(B, F, 72)
    gen = torch.Generator().manual_seed(73 + B)
    actions = torch.randint(0, A_, (B,), generator=gen)
    adv, ret = torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    if kind == "outside":
        actions[0], actions[1] = -3, A_ + 5
    if kind == "zeroadv":
        adv = torch.zeros(B)
    return x, ps, actions, adv, ret


@functools.lru_cache(maxsize=None)
def loss_ref(B, F, A_, lname, ent, norm, kind="plain"):
    x, ps, actions, adv, ret = loss_case(B, F, A_, lname, kind)
    return A.a2c_loss(x, ps, LAYOUTS[lname], actions, adv, ret, VF, ent, norm)


def run_a2c(x, ps, layout, A_, actions, adv, ret, vf, ent, norm, want_dx=True):
    lib, L = _lib()
    dims, acts = layout
    B, F = x.shape
    d = lib.acnet_desc(B, F, A_, dims, acts)
    n = L.ocrl_acnet_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    t = [actions.cuda().long(), adv.cuda(), ret.cuda()]
    scal, dw, dx, ws = nanlike(4), [nanlike(*p.shape) for p in ps], nanlike(B, F) if want_dx else None, nanlike(n)
    rc = L.ocrl_acnet_a2c_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), *[lib.ptr(v) for v in t], vf, ent, int(norm), lib.ptr(scal), lib.ptr(dx),
                                  lib.ptrs(dw), lib.ptr(ws), n, lib.stream())
    torch.cuda.synchronize()
    return rc, dict(scal=scal, dw=dw, dx=dx)


def run_generic(x, ps, layout, A_, actions, adv, ret, vf, ent, norm):
    """the same gradients without the fused step: ocrl_acnet_fwd with save, the cotangents formed in torch from its logits and values (the
    closed form of a2c_ref.cotangents in fp32 on the device), then ocrl_acnet_bwd"""
    lib, L = _lib()
    dims, acts = layout
    B, F = x.shape
    d = lib.acnet_desc(B, F, A_, dims, acts)
    n = L.ocrl_acnet_ws_floats(ctypes.byref(d))
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    lg, vl, ws = nanlike(B, A_), nanlike(B), nanlike(n)
    st = lib.stream()
    lib.check(L.ocrl_acnet_fwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), None, None, lib.ptr(lg), lib.ptr(vl), 1, lib.ptr(ws), n, st))
    dz, dv = A.cotangents(lg, vl, actions.cuda(), adv.cuda(), ret.cuda(), vf, ent, norm)
    dz, dv = dz.contiguous(), dv.contiguous()
    dw, dx = [nanlike(*p.shape) for p in ps], nanlike(B, F)
    lib.check(L.ocrl_acnet_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), None, None, lib.ptr(dz), lib.ptr(dv), lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n,
                               st))
    torch.cuda.synchronize()
    return dict(dw=dw, dx=dx)


def grade_loss(tag, got, generic, want):
    scal, dx, dw = want
    smax = scal.abs().max().item()
    worst_s = worst_g = worst_gen = 0.0
    for i, k in enumerate(A.SCALARS):
        e = abs(got["scal"][i].item() - scal[i].item()) / max(abs(scal[i].item()), 1e-3 * smax, 1e-30)
        worst_s = max(worst_s, e)
        assert e <= 1e-4, (tag, k, e, got["scal"].tolist(), scal.tolist())
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    for nme, g, gg, w in zip(["dx"] + [f"dw{i}" for i in range(len(dw))], [got["dx"]] + got["dw"], [generic["dx"]] + generic["dw"], [dx] + dw):
        e, eg = err(g, w, 1e-3 * gmax), err(gg, w, 1e-3 * gmax)
        worst_g, worst_gen = max(worst_g, e), max(worst_gen, eg)
        assert e <= 3e-4 and eg <= 3e-4, (tag, nme, e, eg)
    log(f"a2c {tag}: worst scalar rel err {worst_s:.2e} (bound 1e-4), worst gradient {worst_g:.2e}, generic path {worst_gen:.2e} (bound 3e-4)")


def check_loss_case(B, F, A_, lname, ent, norm, kind="plain"):
    layout = LAYOUTS[lname]
    inp = loss_case(B, F, A_, lname, kind)
    rc, got = run_a2c(*inp[:2], layout, A_, *inp[2:], VF, ent, norm)
    assert rc == 0, _lib()[1].ocrl_last_error().decode()
    rc2, again = run_a2c(*inp[:2], layout, A_, *inp[2:], VF, ent, norm)
    assert rc2 == 0 and torch.equal(got["scal"], again["scal"]) and torch.equal(got["dx"], again["dx"])
    assert all(torch.equal(u, v) for u, v in zip(got["dw"], again["dw"]))
    generic = run_generic(*inp[:2], layout, A_, *inp[2:], VF, ent, norm)
    grade_loss(f"B{B} F{F} A{A_} {lname} ent{ent} norm{int(norm)} {kind}", got, generic, loss_ref(B, F, A_, lname, ent, norm, kind))
    return got


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("ent", [0.0, 0.01])
@pytest.mark.parametrize("lname", ["ident", "mlp"])
@pytest.mark.parametrize("B,F,A_", SHAPES)
def test_a2c_step_against_fp64(B, F, A_, lname, ent, norm):
    if norm and B == 1:
        inp = loss_case(B, F, A_, lname)
        rc, got = run_a2c(*inp[:2], LAYOUTS[lname], A_, *inp[2:], VF, ent, True)
        assert rc != 0 and "normalize_advantage" in _lib()[1].ocrl_last_error().decode()
        assert torch.isnan(got["scal"]).all() and all(torch.isnan(g).all() for g in got["dw"])          # rejected before any launch
        return
    check_loss_case(B, F, A_, lname, ent, norm)


def test_a2c_step_clamps_actions_outside_the_range():
    got = check_loss_case(17, 12, 3, "mlp", 0.01, False, "outside")
    x, ps, actions, adv, ret = loss_case(17, 12, 3, "mlp", "outside")
    _, clamped = run_a2c(x, ps, MLP, 3, actions.clamp(0, 2), adv, ret, VF, 0.01, False)
    assert torch.equal(got["scal"], clamped["scal"]) and all(torch.equal(u, v) for u, v in zip(got["dw"], clamped["dw"]))


def test_a2c_step_with_all_zero_advantages():
    got = check_loss_case(17, 12, 3, "mlp", 0.01, False, "zeroadv")
    assert got["scal"][1].item() == 0.0                                  # the policy loss is exactly zero; the entropy and value terms remain
    got = check_loss_case(17, 12, 3, "mlp", 0.01, True, "zeroadv")      # normalised: (0 - 0) / (0 + 1e-8) = 0, nothing divides by zero
    assert got["scal"][1].item() == 0.0 and all(torch.isfinite(g).all() for g in got["dw"])


# ------------------------------------------------------------------------------------------------------------ 2. the RMSprop step
RMS_LR, RMS_ALPHA, RMS_EPS, RMS_STEPS = 7e-4, 0.99, 1e-5, 3
RMS_NS = [1, 2, 3, 4, 5, 1027, 262147]
RMS_NORMS = [0.0, 0.5, 1e6]


@functools.lru_cache(maxsize=None)
def rms_case(n):
    """p float32 [n] and three gradients with ||g||_2 = 2 (max_norm 0.5 bites, 1e6 does not), built once on the CPU"""
    gen = torch.Generator().manual_seed(900 + n)
    p = 0.1 * torch.randn(n, generator=gen)
    gs = []
    for _ in range(RMS_STEPS):
        g = torch.randn(n, generator=gen)
        gs.append((g * (2.0 / g.double().norm().item())).float())
    return p, gs


@functools.lru_cache(maxsize=None)
def rms_chain(n, max_norm, dtype=torch.float64):
    """the restatement's three consecutive steps from sq = 1 in `dtype`: a list of (p, sq, norm, coef) after each step"""
    p, gs = rms_case(n)
    sq, out = torch.ones(n), []
    for g in gs:
        r = A.rmsprop_tf_l2(p, g, sq, max_norm, RMS_LR, RMS_ALPHA, RMS_EPS, dtype)
        p, sq = r.p, r.sq
        out.append(r)
    return out


def rms_buffers(n, p, sq, fill=77.0, pad=8):
    bufs = []
    for src in (p, None, sq):
        b = torch.full((n + pad,), fill, device="cuda")
        if src is not None:
            b[:n] = src.cuda()
        bufs.append(b)
    return bufs


def rms_step(bufs, n, max_norm, lr=RMS_LR):
    lib, L = _lib()
    nws = L.ocrl_flat_clip_rmsprop_ws_floats()
    ws, norm = nanlike(nws), nanlike(1)
    rc = L.ocrl_flat_clip_rmsprop_l2(*[lib.ptr(b) for b in bufs], n, max_norm, lr, RMS_ALPHA, RMS_EPS, lib.ptr(norm), lib.ptr(ws), nws, lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ocrl_last_error().decode()
    return norm.cpu()[0]


@pytest.mark.parametrize("max_norm", RMS_NORMS)
@pytest.mark.parametrize("n", RMS_NS)
def test_rmsprop_step(n, max_norm):
    p0, gs = rms_case(n)
    want = rms_chain(n, max_norm)
    bufs = rms_buffers(n, p0, torch.ones(n))
    tails = [b[n:].clone() for b in bufs]
    worst_p = worst_s = worst_n = 0.0
    for k, g in enumerate(gs):
        bufs[1][:n] = g.cuda()
        norm = rms_step(bufs, n, max_norm)
        for b, t in zip(bufs, tails):
            assert torch.equal(b[n:].view(torch.int32), t.view(torch.int32)), "the step wrote past the buffer's n floats"
        assert torch.equal(bufs[1][:n].cpu(), g)
        r = want[k]
        assert (r.coef.item() < 1.0) == (max_norm == 0.5)
        worst_n = max(worst_n, abs(norm.item() - r.norm.item()) / r.norm.item())
        worst_p = max(worst_p, ((bufs[0][:n].cpu().double() - p0.double()) - (r.p - p0.double())).abs().max().item() / RMS_LR)
        worst_s = max(worst_s, (bufs[2][:n].cpu().double() - r.sq).abs().max().item())
        assert (bufs[0][:n].cpu() != p0).double().mean().item() > 0.9
    log(f"rmsprop n{n} max_norm {max_norm:g}: norm rel err {worst_n:.2e} (bound 1e-5), dp/lr dev {worst_p:.2e} ({worst_p / (4 * RMS_DP_DEV):.2f} of the "
        f"bound), sq dev {worst_s:.2e} ({worst_s / (4 * RMS_SQ_DEV):.2f} of the bound)")
    assert worst_n <= 1e-5 and worst_p <= 4 * RMS_DP_DEV and worst_s <= 4 * RMS_SQ_DEV


def test_rmsprop_step_is_reproducible_and_carries_a_nan_to_every_weight():
    n = 1027
    p0, gs = rms_case(n)
    runs = []
    for _ in range(2):
        bufs = rms_buffers(n, p0, torch.ones(n))
        bufs[1][:n] = gs[0].cuda()
        norm = rms_step(bufs, n, 0.5)
        runs.append((bufs[0].clone(), bufs[2].clone(), norm))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    bufs = rms_buffers(n, p0, torch.ones(n))
    g = gs[0].clone()
    g[515] = float("nan")
    bufs[1][:n] = g.cuda()
    norm = rms_step(bufs, n, 0.5)
    assert math.isnan(norm.item()) and torch.isnan(bufs[0][:n]).all() and (bufs[0][n:] == 77.0).all()


def test_rmsprop_step_from_a_zero_square_average_stays_finite():
    """eps is inside the root: sq = 0 and g = 0 give 0 / sqrt(1e-5), not 0 / 0"""
    n = 5
    p0 = rms_case(n)[0]
    bufs = rms_buffers(n, p0, torch.zeros(n))
    bufs[1][:n] = 0.0
    norm = rms_step(bufs, n, 0.5)
    assert norm.item() == 0.0 and torch.isfinite(bufs[0][:n]).all() and torch.equal(bufs[0][:n].cpu(), p0) and (bufs[2][:n] == 0).all()


# ------------------------------------------------------------------------------------------------------------ 3. one train()
TRAIN_LR = 7e-4
TRAIN_HYPER = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=False, max_grad_norm=0.5, learning_rate=TRAIN_LR, rms_prop_eps=1e-5)
TRAIN_UPDATES = 2


def _space(shape=None, n=None):
    return types.SimpleNamespace(shape=shape, n=n)


def make_policy(F, A_, seed, acnet="mlp"):
    from ocrl_amd.sb3s import CustomActorCriticPolicy
    torch.manual_seed(seed)
    return CustomActorCriticPolicy(_space((F,)), _space(n=A_), config=types.SimpleNamespace(sb3_acnet=_acnet_cfg(acnet)))


def abi_params(policy):
    return [p.detach().cpu().clone() for p in policy._head_args()[3]]


def train_case():
    """everything test 3 feeds train(), built on the CPU: the policy, its initial parameters and a hand-filled rollout of T = 5, E = 4
    (features behind an identity extractor; actions sampled by the fp64 restatement under the initial parameters; GAE with lambda = 1)"""
    F, A_, T, E = 12, 4, 5, 4
    pol = make_policy(F, A_, 7)
    ps = abi_params(pol)
    gen = torch.Generator().manual_seed(81)
    feats = torch.randn(T, E, F, generator=gen)
    _, _, lg, vl = R.forward(feats.reshape(T * E, F).double(), [p.double() for p in ps], *MLP)
    actions = P.sample(lg, torch.rand(T * E, generator=gen))
    buf = dict(features=feats, actions=actions.reshape(T, E), values=vl.float().reshape(T, E), log_probs=P.log_prob(lg, actions).float().reshape(T, E),
               rewards=((torch.arange(T * E) * 7) % 5).float().reshape(T, E) / 4, episode_starts=torch.zeros(T, E))
    buf["episode_starts"][0] = 1.0
    buf["episode_starts"][3, ::2] = 1.0
    adv, ret = P.gae(buf["rewards"].double(), buf["values"].double(), buf["episode_starts"].double(), torch.zeros(E, dtype=torch.float64),
                     torch.ones(E, dtype=torch.float64), 0.99, 1.0)
    buf["advantages"], buf["returns"] = adv.float(), ret.float()
    return pol, ps, buf


def ref_updates(ps, buf, use_rms_prop, dtype=torch.float64):
    """TRAIN_UPDATES consecutive a2c_ref.train() on the same buffer: (parameters, the scalars of each update)"""
    hyper = dict(TRAIN_HYPER, use_rms_prop=use_rms_prop)
    state, scal = None, []
    for _ in range(TRAIN_UPDATES):
        ps, s, state = A.train(ps, MLP, buf, hyper, dtype, state)
        scal.append(s)
    return ps, scal


def make_a2c(pol, buf, **over):
    from ocrl_amd.sb3s import A2C, RolloutBuffer
    T, E, F = buf["features"].shape
    env = types.SimpleNamespace(num_envs=E, observation_space=_space((F,)), action_space=_space(n=4))
    kw = dict(n_steps=T, seed=3, device="cuda", gamma=0.99, gae_lambda=1.0)
    kw.update({k: v for k, v in TRAIN_HYPER.items()})
    kw.update(over)
    a2c = A2C(pol, env, **kw)
    rb = RolloutBuffer(T, E, (F,), a2c.device, 0.99, 1.0)
    for t in range(T):
        rb.add(buf["features"][t], buf["actions"][t], buf["rewards"][t], buf["episode_starts"][t], buf["values"][t], buf["log_probs"][t])
    rb.advantages.copy_(buf["advantages"])
    rb.returns.copy_(buf["returns"])
    a2c.rollout_buffer = rb
    return a2c


@pytest.mark.parametrize("use_rms_prop", [True, False], ids=["rmsprop", "adam"])
def test_train_against_the_restatement(use_rms_prop):
    pol, ps, buf = train_case()
    a2c = make_a2c(pol, buf, use_rms_prop=use_rms_prop)
    assert all(p.data_ptr() >= a2c.flat_p.data_ptr() and p.data_ptr() < a2c.flat_p.data_ptr() + 4 * a2c.flat_p.numel() for p in a2c.policy.parameters())
    gen_state = a2c.generator.get_state().clone()
    stats = [a2c.train() for _ in range(TRAIN_UPDATES)]
    assert torch.equal(a2c.generator.get_state(), gen_state)            # no permutation is drawn
    want_p, want_s = ref_updates(ps, buf, use_rms_prop)
    if use_rms_prop:
        assert a2c.rmsprop_step == TRAIN_UPDATES and not hasattr(a2c, "flat_m") and (a2c.square_avg != 1).any()
    else:
        assert a2c.adam_step == TRAIN_UPDATES and not hasattr(a2c, "square_avg") and a2c.flat_v.any()
    bound = 4 * (TRAIN_DEV if use_rms_prop else TRAIN_ADAM_DEV)
    worst = 0.0
    for i, (g, w, p0) in enumerate(zip(abi_params(a2c.policy), want_p, ps)):
        worst = max(worst, ((g.double() - p0.double()) - (w - p0.double())).abs().max().item() / TRAIN_LR)
        assert (g != p0).any(), i
    log(f"a2c train ({'rmsprop' if use_rms_prop else 'adam'}): worst dp/lr deviation {worst:.2e} (bound {bound:.2e}, {worst / bound:.2f} of it)")
    assert worst <= bound
    for u, (st, want) in enumerate(zip(stats, want_s)):
        assert set(st) == {"loss", "policy_loss", "value_loss", "entropy_loss", "explained_variance", "grad_norm", "n_updates"} and st["n_updates"] == 1
        smax = want.abs().max().item()
        for i, k in enumerate(A.SCALARS):
            e = abs(st[k] - want[i].item()) / max(abs(want[i].item()), 1e-3 * smax, 1e-30)
            log(f"a2c train update {u} {k}: got {st[k]:.6f} want {want[i].item():.6f} rel err {e:.2e}")
            assert e <= 1e-4, (u, k, e)
        assert 0 < st["grad_norm"] < 100
    y, v = buf["returns"].double().reshape(-1), buf["values"].double().reshape(-1)
    assert abs(stats[0]["explained_variance"] - (1 - (y - v).var(unbiased=False) / y.var(unbiased=False)).item()) <= 1e-4


# ------------------------------------------------------------------------------------------------------------ 4. rollouts on the device
class HostView:
    """the same environment without ``on_device``: the algorithm then takes its host path through ``step``"""

    def __init__(self, env):
        self.env, self.num_envs, self.observation_space, self.action_space = env, env.num_envs, env.observation_space, env.action_space

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        return self.env.step(actions)


BASE = ["ocr=slate", "pooling=transformer", "sb3=a2c", "sb3_acnet=mlp", "env=target-N4C4S3S1", "device=cuda:0"]


def config(*over):
    from ocrl_amd.utils.config import compose
    return compose(os.path.join(ROOT, "configs"), "train_sb3", BASE + list(over))


def test_a2c_device_path_fills_the_buffers_of_the_host_path():
    from ocrl_amd import envs
    from ocrl_amd.sb3s import A2C, CustomActorCriticPolicy

    def build(as_host):
        env = envs.TargetEnv(config("env.obs_size=16", "env.max_steps=5", "env.rew_type=dense").env, 4, seed=31, device="cuda")
        kw = dict(n_steps=5, seed=13, ent_coef=0.01, policy_kwargs=dict(config=types.SimpleNamespace(sb3_acnet=_acnet_cfg("mlp"))))
        return A2C(CustomActorCriticPolicy, HostView(env) if as_host else env, **kw)
    dev, hst = build(False), build(True)
    assert getattr(dev.env, "on_device", False) and not getattr(hst.env, "on_device", False)
    start = dev.flat_p.clone()
    for it in range(2):
        a, b = dev.collect_rollouts(), hst.collect_rollouts()
        for k in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (it, k)
        assert a.observations.dtype == torch.uint8 and a.observations.any() and a.rewards.abs().max() > 0
        assert list(dev._episodes) == list(hst._episodes) and len(dev._episodes) >= 4 * (it + 1)
        assert dev.num_timesteps == hst.num_timesteps == 20 * (it + 1)
        sa, sb = dev.train(), hst.train()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert sa[k] == sb[k] or (math.isnan(sa[k]) and math.isnan(sb[k])), (it, k, sa[k], sb[k])
        assert torch.equal(dev.flat_p, hst.flat_p) and torch.equal(dev.square_avg, hst.square_avg)
    assert not torch.equal(dev.flat_p, start) and 0.0 <= dev.success_rate <= 1.0


# ------------------------------------------------------------------------------------------------------------ 5. it learns
class FourArms:
    """E = 4 environments, a constant observation, episodes of one step, reward 1 for action 0 and 0 for the other three"""
    E, F, A = 4, 4, 4

    def __init__(self):
        self.num_envs, self.observation_space, self.action_space = self.E, _space((self.F,)), _space(n=self.A)
        self.obs = np.ones((self.E, self.F), dtype=np.float32)

    def reset(self):
        return self.obs

    def step(self, actions):
        actions = np.asarray(actions)
        return self.obs, (actions == 0).astype(np.float32), np.ones(self.E, dtype=bool), [dict() for _ in range(self.E)]


# Chosen on the CPU: a2c_ref.train in fp64 on this exact setup (the policy of make_policy(4, 4, LEARN_SEED, "identity"), n_steps = 5, the
# actions drawn by ppo_ref.sample from ppo_ref.uniforms(LEARN_SEED, ...), the stream the policy draws from on the GPU) takes p(action 0)
# from 0.099 to 0.977 in LEARN_UPDATES updates at LEARN_LR (restatement_learns below is that run).
LEARN_SEED, LEARN_LR, LEARN_UPDATES, LEARN_STEPS = 11, 0.03, 200, 5


def restatement_learns(dtype=torch.float64):
    """(p(action 0) before, after) of the fp64 restatement of the run of test_a2c_learns_the_rewarded_arm, on the CPU"""
    env, T = FourArms(), LEARN_STEPS
    ps = [p.to(dtype) for p in abi_params(make_policy(env.F, env.A, LEARN_SEED, "identity"))]
    hyper = dict(vf_coef=0.5, ent_coef=0.0, normalize_advantage=False, max_grad_norm=0.5, learning_rate=LEARN_LR, rms_prop_eps=1e-5, use_rms_prop=True)
    obs = torch.ones(env.E, env.F, dtype=dtype)
    prob0 = lambda: torch.softmax(R.forward(obs, ps, *IDENT)[2][0], -1)[0].item()
    first, state, rows = prob0(), None, 0
    for _ in range(LEARN_UPDATES):
        _, _, lg, vl = R.forward(obs, ps, *IDENT)
        feats, acts, rews, vals = [], [], [], []
        for t in range(T):
            a = P.sample(lg, P.uniforms(LEARN_SEED, rows, env.E))
            rows += env.E
            feats.append(obs), acts.append(a), rews.append((a == 0).to(dtype)), vals.append(vl)
        rew, val = torch.stack(rews), torch.stack(vals)
        adv, ret = P.gae(rew, val, torch.ones(T, env.E, dtype=dtype), vl, torch.ones(env.E, dtype=dtype), 0.99, 1.0)
        buf = dict(features=torch.stack(feats), actions=torch.stack(acts), advantages=adv, returns=ret)
        ps, _, state = A.train(ps, IDENT, buf, hyper, dtype, state)
    return first, prob0()


def test_a2c_learns_the_rewarded_arm():
    from ocrl_amd.sb3s import A2C
    env = FourArms()
    a2c = A2C(make_policy(env.F, env.A, LEARN_SEED, "identity"), env, learning_rate=LEARN_LR, n_steps=LEARN_STEPS, seed=LEARN_SEED)
    obs = torch.ones(1, env.F, device="cuda")
    prob0 = lambda: torch.softmax(a2c.policy.logits_values(obs)[0][0].detach(), -1)[0].item()
    first = prob0()
    a2c.learn(LEARN_UPDATES * LEARN_STEPS * env.E)
    last = prob0()
    log(f"a2c learns: p(action 0) {first:.3f} -> {last:.3f} after {a2c.rmsprop_step} updates at lr {LEARN_LR} (ep_rew_mean {a2c.ep_rew_mean:.2f})")
    assert a2c.rmsprop_step == LEARN_UPDATES and a2c.num_timesteps == LEARN_UPDATES * LEARN_STEPS * env.E
    assert last >= 0.5 and last > first


# ------------------------------------------------------------------------------------------------------------ 6. checkpoints
def test_checkpoints_resume_bit_for_bit_and_name_their_algorithm(tmp_path):
    from ocrl_amd.sb3s import PPO
    pol, ps, buf = train_case()
    a2c = make_a2c(pol, buf)
    a2c.train()
    path = str(tmp_path / "a2c.pt")
    a2c.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["algo"] == "A2C" and set(ck["optimizer"]) == {"square_avg", "step", "sampling_rows"} and ck["optimizer"]["step"] == 1
    fresh = make_a2c(make_policy(12, 4, 99), buf)
    assert not torch.equal(fresh.flat_p, a2c.flat_p)
    assert fresh.load(path) is fresh
    assert torch.equal(fresh.flat_p, a2c.flat_p) and torch.equal(fresh.square_avg, a2c.square_avg) and fresh.rmsprop_step == 1
    assert all(p.data_ptr() >= fresh.flat_p.data_ptr() and p.data_ptr() < fresh.flat_p.data_ptr() + 4 * fresh.flat_p.numel() for p in fresh.policy.parameters())
    sa, sb = a2c.train(), fresh.train()
    assert sa == sb and torch.equal(fresh.flat_p, a2c.flat_p) and torch.equal(fresh.square_avg, a2c.square_avg)
    # the Adam variant keeps Adam's moments
    adam = make_a2c(make_policy(12, 4, 7), buf, use_rms_prop=False)
    adam.train()
    adam.save(str(tmp_path / "a2c_adam.pt"))
    ck = torch.load(str(tmp_path / "a2c_adam.pt"), map_location="cpu", weights_only=True)
    assert ck["algo"] == "A2C" and set(ck["optimizer"]) == {"m", "v", "step", "sampling_rows"}
    twin = make_a2c(make_policy(12, 4, 98), buf, use_rms_prop=False).load(str(tmp_path / "a2c_adam.pt"))
    assert torch.equal(twin.flat_p, adam.flat_p) and torch.equal(twin.flat_v, adam.flat_v) and twin.adam_step == 1
    # each algorithm loads its own files only
    env = types.SimpleNamespace(num_envs=4, observation_space=_space((12,)), action_space=_space(n=4))
    ppo = PPO(make_policy(12, 4, 5), env, n_steps=5, batch_size=10)
    before = ppo.flat_p.clone()
    with pytest.raises(ValueError, match="PPO") as e:
        ppo.load(path)
    assert "A2C" in str(e.value) and torch.equal(ppo.flat_p, before)
    ppo_path = str(tmp_path / "ppo.pt")
    ppo.save(ppo_path)
    before = a2c.flat_p.clone()
    with pytest.raises(ValueError, match="A2C") as e:
        a2c.load(ppo_path)
    assert "PPO" in str(e.value) and torch.equal(a2c.flat_p, before)
    assert torch.equal(PPO(make_policy(12, 4, 6), env, n_steps=5, batch_size=10).load(ppo_path).flat_p, ppo.flat_p)


# ------------------------------------------------------------------------------------------------------------ 7. the entry points
SMOKE_SLATE = ["ocr.dvae.vocab_size=256", "ocr.slotattr.num_slots=6", "ocr.slotattr.num_iterations=3", "ocr.tfdec.num_dec_blocks=2", "env.obs_size=16"]


def test_train_sb3_and_test_sb3_run_a2c_in_child_processes(tmp_path):
    from ocrl_amd import ocrs
    shared = SMOKE_SLATE + ["num_envs=4", "env.max_steps=6", "env.rew_type=dense"]
    c = config(*shared)
    assert c.sb3.name == "A2C"
    src = ocrs.SLATE(c.ocr, c.env)
    src.to("cuda:0")
    ckpt = str(tmp_path / "slate.pth")
    torch.save(src.save(), ckpt)
    shared.append(f"pooling.ocr_checkpoint.local_file={ckpt}")
    over = shared + ["max_steps=64", "eval.freq=32", "eval.n_episodes=4", f"run_dir={tmp_path / 'run'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_sb3.py")] + BASE + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    # n_steps = max(1, 5 // 4) = 1: an update every 4 environment steps
    assert [l["step"] for l in lines] == list(range(4, 65, 4)) and [l["iteration"] for l in lines] == list(range(1, 17))
    for l in lines:
        for k in ("train/loss", "train/policy_loss", "train/value_loss", "train/entropy_loss"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
    evals = [l for l in lines if "eval/mean_reward" in l]
    assert [l["step"] for l in evals] == [32, 64]
    for l in evals:
        for k in ("eval/success_rate", "eval/mean_reward", "eval/mean_ep_length"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
    agent = tmp_path / "run" / "checkpoints" / "model_latest.pth"
    assert agent.exists() and (tmp_path / "run" / "checkpoints" / "model_best.pth").exists()
    assert torch.load(str(agent), map_location="cpu", weights_only=True)["algo"] == "A2C"
    over = shared + [f"agent_checkpoint.local_file={agent}", "n_eval_episodes=4", f"run_dir={tmp_path / 'test'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "test_sb3.py")] + BASE + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(l) for l in open(tmp_path / "test" / "eval.jsonl")]
    assert len(rows) == 1 and rows[0]["episodes"] == 4 and rows[0]["env"] == "TargetN4C4S3S1Env" and math.isfinite(rows[0]["mean_reward"])
    log(f"test_sb3 sb3=a2c: {rows[0]}")
