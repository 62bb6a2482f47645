"""GPU checks of the actor-critic head and the PPO minibatch step: ocrl_acnet_fwd/_bwd/_ppo_fwd_bwd and ocrl_gae through the C ABI against
the fp64 torch restatement of tests/acnet_ref.py (NaN-filled outputs and workspace), the reference fixture through the Python classes,
the ABI contract (reproducibility, independent rows, detached features, rejected shapes) and the path
OCRExtractor -> CustomActorCriticPolicy -> ppo_loss -> backward -> Adam.

Bounds: grid data (small integers, ReLU only) is exact forward (1e-6) and 1e-5 on gradients; Gaussian data 1e-4 of each output's maximum
and 3e-4 of each gradient's maximum with the 1e-3 gmax floor (the RN head's bounds for 64-256 wide fp32 MFMA layers).  Gaussian runs with
ReLU layers stay at B <= 37 rows (fp32 / fp64 ReLU sign ties move whole rows beyond that); B = 2048 runs on grid data and tanh layouts."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import acnet_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

MLP = (((64, 64), (64,), (64,)), ((1, 1), (2,), (2,)))                     # configs/sb3_acnet/mlp.yaml, mlp_orthoinit.yaml
IDENT = (((), (), ()), ((), (), ()))                                       # identity.yaml, identity_orthoinit.yaml
MLP_RELU = (((64, 64), (64,), (64,)), ((1, 1), (1,), (1,)))
DEEP_RELU = (((64, 128), (256,), (128, 64)), ((1, 1), (1,), (1, 1)))
DEEP = (((64, 128), (256,), (128, 64)), ((1, 2), (2,), (0, 2)))
TANH = (((64,), (64,), (64, 64)), ((2,), (2,), (2, 2)))
VAL2 = (((), (), (64, 64)), ((), (), (2, 1)))


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def make_params(F, A, dims, seed, grid=False):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for s in R.param_shapes(F, A, dims):
        if grid:
            if len(s) == 2:
                keep = torch.rand(s, generator=gen) < min(1.0, 4.0 / s[1])
                ps.append(torch.where(keep, torch.randint(0, 2, s, generator=gen).float() * 2 - 1, torch.zeros(())))
            else:
                ps.append(torch.randint(-2, 2, s, generator=gen).float() + 0.5)
        elif len(s) == 2:
            ps.append(torch.randn(s, generator=gen) * (1.4 / s[1] ** 0.5))
        else:
            ps.append(torch.randn(s, generator=gen) * 0.05)
    return ps


def make_x(B, F, seed, grid=False):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (B, F), generator=gen).float() if grid else torch.randn(B, F, generator=gen)


def nanlike(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def run_abi(x, ps, layout, A, cots, want_dx=True, save=1):
    """forward (+ backward when `cots` = (dlat_pi, dlat_vf, dlogits, dvalues), entries may be None) through the C ABI"""
    lib, L = _lib()
    dims, acts = layout
    B, F = x.shape
    d = lib.acnet_desc(B, F, A, dims, acts)
    n = L.ocrl_acnet_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    h = dims[0][-1] if dims[0] else F
    lp, lv = nanlike(B, dims[1][-1] if dims[1] else h), nanlike(B, dims[2][-1] if dims[2] else h)
    lg, vl = (nanlike(B, A), nanlike(B)) if A else (None, None)
    ws = nanlike(n)
    st = lib.stream()
    lib.check(L.ocrl_acnet_fwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd) if pd else None, lib.ptr(lp), lib.ptr(lv), lib.ptr(lg), lib.ptr(vl), save,
                               lib.ptr(ws), n, st))
    out = dict(lp=lp, lv=lv, logits=lg, values=vl)
    if cots is not None:
        cd = [None if c is None else c.cuda().contiguous() for c in cots]
        dw = [nanlike(*p.shape) for p in ps]
        dx = nanlike(B, F) if want_dx else None
        lib.check(L.ocrl_acnet_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd) if pd else None, *[lib.ptr(c) for c in cd], lib.ptr(dx),
                                   lib.ptrs(dw) if dw else None, lib.ptr(ws), n, st))
        out.update(dw=dw, dx=dx)
    torch.cuda.synchronize()
    return out


def run_ppo(x, ps, layout, A, actions, old, adv, ret, clip, vf, ent, norm, want_dx=True):
    lib, L = _lib()
    dims, acts = layout
    B, F = x.shape
    d = lib.acnet_desc(B, F, A, dims, acts)
    n = L.ocrl_acnet_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    t = [actions.cuda().long(), old.cuda(), adv.cuda(), ret.cuda()]
    scal, dw, dx, ws = nanlike(6), [nanlike(*p.shape) for p in ps], nanlike(B, F) if want_dx else None, nanlike(n)
    rc = L.ocrl_acnet_ppo_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), *[lib.ptr(v) for v in t], clip, vf, ent, int(norm), lib.ptr(scal),
                                  lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream())
    torch.cuda.synchronize()
    return rc, dict(scal=scal, dw=dw, dx=dx)


def ref64(x, ps, layout, A, cots):
    dims, acts = layout
    x64 = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in ps]
    lp, lv, lg, vl = R.forward(x64, p64, dims, acts, heads=A > 0)
    out = dict(lp=lp, lv=lv, logits=lg, values=vl)
    if cots is not None:
        tot = 0
        for y, c in zip((lp, lv, lg, vl), cots):
            if c is not None:
                tot = tot + (y * c.double()).sum()
        g = torch.autograd.grad(tot, [x64] + p64, allow_unused=True)
        z = lambda t, like: torch.zeros_like(like) if t is None else t
        out.update(dx=z(g[0], x64), dw=[z(a, b) for a, b in zip(g[1:], p64)])
    return out


def err(got, want, floor=0.0):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert torch.isfinite(got).all(), "non-finite entries (an output the kernels did not write?)"
    return (got - want).abs().max().item() / max(want.abs().max().item(), floor, 1e-30)


def compare(tag, got, want, out_tol, grad_tol, floor_rel):
    for k in ("lp", "lv", "logits", "values"):
        if want[k] is not None:
            e = err(got[k], want[k])
            log(f"{tag} {k} rel err {e:.2e}")
            assert e <= out_tol, (tag, k, e)
    if "dw" in want:
        gs = [want["dx"]] + want["dw"]
        gmax = max([g.abs().max().item() for g in gs] + [1e-30])
        names = ["dx"] + [f"dw{i}" for i in range(len(want["dw"]))]
        for nme, g, w in zip(names, [got["dx"]] + got["dw"], gs):
            if g is None:
                continue
            e = err(g, w, floor_rel * gmax)
            log(f"{tag} {nme} rel err {e:.2e}")
            assert e <= grad_tol, (tag, nme, e)


def make_cots(B, layout, F, A, seed, grid=False, which=(True, True, True, True)):
    dims = layout[0]
    h = dims[0][-1] if dims[0] else F
    shapes = [(B, dims[1][-1] if dims[1] else h), (B, dims[2][-1] if dims[2] else h), (B, A), (B,)]
    gen = torch.Generator().manual_seed(seed)
    out = []
    for s, w in zip(shapes, which):
        if not w or (A == 0 and s in shapes[2:]):
            out.append(None)
        else:
            out.append(torch.randint(-2, 3, s, generator=gen).float() if grid else torch.randn(s, generator=gen))
    if A == 0:
        out[2] = out[3] = None
    return out


GRID_CASES = [(1, 64, 4, MLP_RELU), (4, 67, 1, MLP_RELU), (32, 192, 18, DEEP_RELU), (37, 1152, 4, MLP_RELU), (2048, 64, 4, MLP_RELU),
              (2048, 67, 18, DEEP_RELU), (37, 67, 4, IDENT), (4, 192, 0, DEEP_RELU), (32, 64, 0, IDENT)]


@pytest.mark.parametrize("B,F,A,layout", GRID_CASES)
def test_grid_data_against_fp64(B, F, A, layout):
    ps = make_params(F, A, layout[0], 3, grid=True)
    x = make_x(B, F, 4, grid=True)
    cots = make_cots(B, layout, F, A, 5, grid=True)
    got, want = run_abi(x, ps, layout, A, cots), ref64(x, ps, layout, A, cots)
    compare(f"grid B{B} F{F} A{A}", got, want, 1e-6, 1e-5, 1e-3)


GAUSS_CASES = [(1, 64, 4, MLP), (4, 128, 4, MLP), (32, 67, 18, MLP), (37, 192, 1, DEEP), (4, 1152, 4, MLP), (32, 1152, 18, IDENT),
               (37, 64, 4, VAL2), (2048, 192, 4, TANH), (2048, 67, 18, TANH), (32, 128, 0, MLP), (4, 64, 0, VAL2)]


@pytest.mark.parametrize("B,F,A,layout", GAUSS_CASES)
def test_gaussian_data_against_fp64(B, F, A, layout):
    ps = make_params(F, A, layout[0], 7)
    x = make_x(B, F, 8)
    cots = make_cots(B, layout, F, A, 9)
    got, want = run_abi(x, ps, layout, A, cots), ref64(x, ps, layout, A, cots)
    compare(f"gauss B{B} F{F} A{A}", got, want, 1e-4, 3e-4, 1e-3)


def test_partial_cotangents_and_detached_features():
    """a NULL cotangent is zero (its side's dW is written as zeros); dfeatures = NULL leaves dw unchanged, bit for bit"""
    B, F, A, layout = 37, 67, 4, MLP
    ps, x = make_params(F, A, layout[0], 7), make_x(B, F, 8)
    cots = make_cots(B, layout, F, A, 9, which=(False, False, True, False))
    got, want = run_abi(x, ps, layout, A, cots), ref64(x, ps, layout, A, cots)
    compare("logits only", got, want, 1e-4, 3e-4, 1e-3)
    cots = make_cots(B, layout, F, A, 9)
    a, b = run_abi(x, ps, layout, A, cots), run_abi(x, ps, layout, A, cots, want_dx=False)
    assert all(torch.equal(u, v) for u, v in zip(a["dw"], b["dw"]))
    nosave = run_abi(x, ps, layout, A, None, save=0)
    assert torch.equal(nosave["logits"], a["logits"]) and torch.equal(nosave["values"], a["values"])


def ppo_inputs(B, A, logits, seed, spread=0.35):
    """actions, old_log_prob, advantages, returns with the clamp active above and below on some rows and inactive on others"""
    gen = torch.Generator().manual_seed(seed)
    actions = torch.randint(0, A, (B,), generator=gen)
    logp = torch.log_softmax(logits.detach().float().cpu(), -1).gather(1, actions[:, None])[:, 0]
    shift = (torch.arange(B) % 3 - 1).float() * spread                    # ratio = exp(shift): below, inside, above the clip range in turn
    return actions, logp - shift, torch.randn(B, generator=gen), torch.randn(B, generator=gen)


def ppo_ref64(x, ps, layout, A, inp, clip, vf, ent, norm):
    dims, acts = layout
    x64 = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in ps]
    _, _, lg, vl = R.forward(x64, p64, dims, acts)
    a, old, adv, ret = inp
    s = R.ppo(lg, vl, a, old.double(), adv.double(), ret.double(), clip, vf, ent, norm)
    g = torch.autograd.grad(s["loss"], [x64] + p64)
    return torch.stack([s[k].detach() for k in R.SCALARS]), g[0], list(g[1:])


PPO_CASES = [(32, 128, 4, MLP, True, 0.0), (32, 128, 4, MLP, False, 0.01), (37, 67, 18, DEEP, True, 0.01), (4, 1152, 4, IDENT, True, 0.01),
             (2048, 128, 4, TANH, True, 0.01), (1, 64, 4, MLP, False, 0.01), (3, 64, 1, VAL2, True, 0.0), (2048, 64, 18, TANH, False, 0.0)]


@pytest.mark.parametrize("B,F,A,layout,norm,ent", PPO_CASES)
def test_ppo_step_against_fp64(B, F, A, layout, norm, ent):
    ps, x = make_params(F, A, layout[0], 21), make_x(B, F, 22)
    lg64 = R.forward(x.double(), [p.double() for p in ps], *layout)[2]
    inp = ppo_inputs(B, A, lg64, 23)
    clip, vf = 0.2, 0.5
    rc, got = run_ppo(x, ps, layout, A, *inp, clip, vf, ent, norm)
    assert rc == 0
    scal, dx, dw = ppo_ref64(x, ps, layout, A, inp, clip, vf, ent, norm)
    log(f"ppo B{B} F{F} A{A}: got {got['scal'].tolist()} want {scal.tolist()}")
    if B >= 3 and A > 1:
        assert 0.0 < scal[5].item() < 1.0                             # the clamp is active on some rows and inactive on others
    smax = scal[:5].abs().max().item()
    for i, k in enumerate(R.SCALARS):
        e = abs(got["scal"][i].item() - scal[i].item()) / max(abs(scal[i].item()), 1e-3 * smax, 1e-30)
        log(f"ppo B{B} {k} rel err {e:.2e}")
        assert e <= 1e-4, (k, e)
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    for nme, g, w in zip(["dx"] + [f"dw{i}" for i in range(len(dw))], [got["dx"]] + got["dw"], [dx] + dw):
        e = err(g, w, 1e-3 * gmax)
        log(f"ppo B{B} {nme} rel err {e:.2e}")
        assert e <= 3e-4, (nme, e)


def test_ppo_rejects_one_row_with_normalisation():
    lib, L = _lib()
    ps, x = make_params(64, 4, MLP[0], 1), make_x(1, 64, 2)
    rc, _ = run_ppo(x, ps, MLP, 4, torch.zeros(1), torch.zeros(1), torch.ones(1), torch.ones(1), 0.2, 0.5, 0.0, True)
    assert rc != 0 and "normalize_advantage" in L.ocrl_last_error().decode()


@pytest.mark.parametrize("T", [1, 5, 512])
@pytest.mark.parametrize("E", [1, 4, 16])
def test_gae_against_the_restatement(T, E):
    lib, L = _lib()
    gen = torch.Generator().manual_seed(T * 31 + E)
    rw, val = torch.randn(T, E, generator=gen), torch.randn(T, E, generator=gen)
    st = (torch.rand(T, E, generator=gen) < 0.1).float()
    st[0] = 1.0
    st[T - 1, ::2] = 1.0
    lastv, dones = torch.randn(E, generator=gen), (torch.rand(E, generator=gen) < 0.5).float()
    want_a, want_r = R.gae(rw.double(), val.double(), st.double(), lastv.double(), dones.double(), 0.99, 0.95)
    d = [t.cuda() for t in (rw, val, st, lastv, dones)]
    adv, ret = nanlike(T, E), nanlike(T, E)
    lib.check(L.ocrl_gae(*[lib.ptr(t) for t in d], lib.ptr(adv), lib.ptr(ret), T, E, 0.99, 0.95, lib.stream()))
    torch.cuda.synchronize()
    ea, er = err(adv, want_a), err(ret, want_r)
    log(f"gae T{T} E{E}: adv {ea:.2e} ret {er:.2e}")
    assert ea <= 1e-5 and er <= 1e-5
    from ocrl_amd.sb3s import compute_gae
    a2, r2 = compute_gae(*d, 0.99, 0.95)
    assert torch.equal(a2, adv) and torch.equal(r2, ret)


@pytest.mark.parametrize("B", [37, 2048])
def test_runs_are_bit_identical_and_rows_independent(B):
    F, A, layout = 128, 4, MLP
    ps, x = make_params(F, A, layout[0], 31), make_x(B, F, 32)
    cots = make_cots(B, layout, F, A, 33)
    a, b = run_abi(x, ps, layout, A, cots), run_abi(x, ps, layout, A, cots)
    for k in ("lp", "lv", "logits", "values", "dx"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(u, v) for u, v in zip(a["dw"], b["dw"]))
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(34))
    c = run_abi(x[perm], ps, layout, A, None)
    assert torch.equal(c["logits"], a["logits"][perm.cuda()]) and torch.equal(c["values"], a["values"][perm.cuda()])
    inp = ppo_inputs(B, A, a["logits"], 35)
    (_, p1), (_, p2) = run_ppo(x, ps, layout, A, *inp, 0.2, 0.5, 0.01, True), run_ppo(x, ps, layout, A, *inp, 0.2, 0.5, 0.01, True)
    assert torch.equal(p1["scal"], p2["scal"]) and torch.equal(p1["dx"], p2["dx"]) and all(torch.equal(u, v) for u, v in zip(p1["dw"], p2["dw"]))
    _, p3 = run_ppo(x, ps, layout, A, *inp, 0.2, 0.5, 0.01, True, want_dx=False)
    assert all(torch.equal(u, v) for u, v in zip(p1["dw"], p3["dw"]))


@pytest.mark.parametrize("bad", [dict(B=0), dict(F=0), dict(A=65), dict(A=-1), dict(dims=((66,), (), ())), dict(dims=((260,), (), ())),
                                 dict(dims=((64,) * 9, (), ())), dict(acts=((3,), (), ()), dims=((64,), (), ()))])
def test_rejected_shapes(bad):
    lib, L = _lib()
    kw = dict(B=4, F=64, A=4, dims=((64,), (), ()), acts=None)
    kw.update(bad)
    if kw["acts"] is None:
        kw["acts"] = tuple(tuple(1 for _ in t) for t in kw["dims"])
    d = lib.AcnetDesc(B=kw["B"], F=kw["F"], A=kw["A"])
    for t in range(3):
        d.n[t] = len(kw["dims"][t])
        for l in range(min(len(kw["dims"][t]), 8)):
            d.dims[t][l], d.acts[t][l] = kw["dims"][t][l], kw["acts"][t][l]
    assert L.ocrl_acnet_ws_floats(ctypes.byref(d)) == 0
    x = torch.zeros(4, 64, device="cuda")
    dummy = [torch.zeros(64 * 64, device="cuda") for _ in range(6)]
    out = nanlike(4, 64)
    rc = L.ocrl_acnet_fwd(ctypes.byref(d), lib.ptr(x), lib.ptrs(dummy), lib.ptr(out), None, None, None, 0, None, 0, lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and L.ocrl_last_error().decode() and torch.isnan(out).all()


def _acnet_cfg(name):
    from ocrl_amd.utils.config import compose
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return compose(os.path.join(root, "configs", "sb3_acnet"), name)


def test_reference_fixture_through_the_python_classes():
    """latents, logits, values, the six PPO scalars and every gradient of tests/golden/acnet.npz"""
    from ocrl_amd.sb3s import CustomActorCriticPolicy, CustomNetwork, ppo_loss
    from tests.golden.make_golden_acnet import CASES, FIXTURE, case_config
    fx = np.load(FIXTURE)
    for tag, (F, B, A, _) in CASES.items():
        cfg = case_config(tag)
        pol = CustomActorCriticPolicy(None, types.SimpleNamespace(n=A), config=types.SimpleNamespace(sb3_acnet=cfg),
                                      features_extractor=types.SimpleNamespace(features_dim=F)).cuda()
        names = [k for k, _ in pol.mlp_extractor.state_dict().items()]
        assert names == list(fx[f"{tag}.keys"])
        pol.mlp_extractor.load_state_dict({k: torch.from_numpy(fx[f"{tag}.w.{k}"]) for k in names})
        for k in ("action_net", "value_net"):
            getattr(pol, k).load_state_dict({"weight": torch.from_numpy(fx[f"{tag}.{k}.weight"]), "bias": torch.from_numpy(fx[f"{tag}.{k}.bias"])})
        x = torch.from_numpy(fx[f"{tag}.features"]).cuda().requires_grad_(True)
        lp, lv = pol.mlp_extractor(x)
        lg, vl = pol.logits_values(x)
        for nme, got in (("latent_pi", lp), ("latent_vf", lv), ("logits", lg), ("values", vl)):
            e = err(got, torch.from_numpy(fx[f"{tag}.{nme}"]))
            log(f"fixture {tag} {nme} rel err {e:.2e}")
            assert e <= 1e-4
        t = lambda k: torch.from_numpy(fx[f"{tag}.{k}"]).cuda()
        loss, m = ppo_loss(pol, x, t("actions"), t("old_log_prob"), t("advantages"), t("returns"), 0.2, 0.5, 0.01, True)
        loss.backward()
        want = fx[f"{tag}.scalars"]
        smax = np.abs(want[:5]).max()
        for i, k in enumerate(R.SCALARS):
            e = abs(m[k].item() - want[i]) / max(abs(want[i]), 1e-3 * smax)
            log(f"fixture {tag} {k} rel err {e:.2e}")
            assert e <= 1e-4, (k, e)
        grads = {"features": x.grad}
        grads.update({f"w.{k}": p.grad for k, p in pol.mlp_extractor.named_parameters()})
        grads.update({f"{h}.{k}": p.grad for h in ("action_net", "value_net") for k, p in getattr(pol, h).named_parameters()})
        gmax = max(np.abs(fx[f"{tag}.grad.{k}"]).max() for k in grads)
        for k, g in grads.items():
            e = err(g, torch.from_numpy(fx[f"{tag}.grad.{k}"]), 1e-3 * gmax)
            log(f"fixture {tag} grad {k} rel err {e:.2e}")
            assert e <= 3e-4, (k, e)
    net = CustomNetwork(24, _acnet_cfg("identity")).cuda()
    x = torch.randn(4, 24, device="cuda")
    a, b = net(x)
    assert a is x and b is x
    with pytest.raises(RuntimeError):
        CustomNetwork(24, _acnet_cfg("mlp"))(torch.randn(4, 24))


def test_extractor_policy_ppo_loss_and_an_adam_step():
    from ocrl_amd.sb3s import CustomActorCriticPolicy, OCRExtractor, ppo_loss
    from ocrl_amd.utils.config import compose
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ocr_cfg = compose(os.path.join(root, "configs"), "train_ocr", ["ocr=slate", "ocr.slotattr.num_slots=5", "ocr.dvae.vocab_size=256",
                                                                  "ocr.tfdec.num_dec_blocks=1", "dataset=random-N5C4S4S2", "dataset.obs_size=32"])
    full = types.SimpleNamespace(ocr=ocr_cfg.ocr, env=ocr_cfg.dataset, pooling=compose(os.path.join(root, "configs", "pooling"), "transformer"),
                                 num_envs=4, device="cuda:0", sb3_acnet=_acnet_cfg("mlp"))
    torch.manual_seed(5)
    pol = CustomActorCriticPolicy(None, types.SimpleNamespace(n=4), config=full, features_extractor_class=OCRExtractor,
                                  features_extractor_kwargs=dict(config=full)).to("cuda:0")
    pol.train()
    B = 8
    obs = torch.rand(B, 3, 32, 32, device="cuda")
    with torch.no_grad():
        actions, values, logp = pol(obs)
    assert actions.shape == (B,) and values.shape == (B, 1) and logp.shape == (B,) and (logp <= 0).all()
    assert pol.predict_values(obs).shape == (B, 1)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    before = {k: p.detach().clone() for k, p in pol.named_parameters()}
    feats = pol.extract_features(obs)
    assert feats.requires_grad
    adv, ret = torch.randn(B, device="cuda"), torch.randn(B, device="cuda")
    old = logp + 0.3 * (torch.arange(B, device="cuda") % 3 - 1)
    loss, m = ppo_loss(pol, feats, actions, old, adv, ret, 0.2, 0.5, 0.01, True)
    # the same features through the restatement, and through evaluate_actions of a policy that shares the networks and takes features
    lg, vl = pol.logits_values(feats.detach())
    want = R.ppo(lg.double(), vl.double(), actions, old.double(), adv.double(), ret.double(), 0.2, 0.5, 0.01, True)
    assert abs(loss.item() - want["loss"].item()) <= 1e-4 * max(abs(want["loss"].item()), 1e-3)
    ident = torch.nn.Identity()
    ident.features_dim = feats.shape[1]
    twin = CustomActorCriticPolicy(None, types.SimpleNamespace(n=4), config=full, features_extractor=ident)
    twin.mlp_extractor, twin.action_net, twin.value_net = pol.mlp_extractor, pol.action_net, pol.value_net
    with torch.no_grad():
        v2, lp2, ent2 = twin.evaluate_actions(feats.detach(), actions)
    assert v2.shape == (B, 1) and lp2.shape == (B,) and ent2.shape == (B,)
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp2 - old)
    mine = -torch.min(a * ratio, a * ratio.clamp(0.8, 1.2)).mean() + 0.01 * -ent2.mean() + 0.5 * ((ret - v2[:, 0]) ** 2).mean()
    assert abs(loss.item() - mine.item()) <= 1e-4 * max(abs(mine.item()), 1e-3)
    assert abs(m["entropy_loss"].item() + ent2.mean().item()) <= 1e-4 * ent2.mean().abs().item()
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    changed = {k: not torch.equal(p.detach(), before[k]) for k, p in pol.named_parameters()}
    assert all(torch.isfinite(p).all() for p in pol.parameters())
    for prefix in ("features_extractor._ocr.", "features_extractor._pooling.", "mlp_extractor.", "action_net.", "value_net."):
        assert any(v for k, v in changed.items() if k.startswith(prefix)), prefix
