"""GPU checks of DQN's noisy linear layers: the entry points of include/ocrl_hip_noisy.h through the C ABI, the autograd function that
puts them in front of the unchanged heads, and ``DQN(noisy=True)``, against the restatement of tests/noisy_ref.py.

Bounds.  ``ocrl_noisy_perturb`` and ``ocrl_noisy_grad`` are products and sums of fp32 numbers, each rounded once: they are compared to the
bit with the CPU's fp32 arithmetic on the factors the GPU wrote.  The factors themselves go through the hardware's fast log and cos and a
square root whose slope grows towards 0: FACTOR_DEV below is the largest absolute deviation from the fp64 restatement measured on an MI355X
over cases a to d and three draws, the bound is 4 x that, and it must stay below 1e-3 (a mis-indexed stream deviates by order 1).  With
``eps`` given a factor is one correctly rounded square root: 2 ulp.  The distribution test allows five standard errors of a unit normal's
mean and second moment over N = 65536 values; the run is deterministic.  Gradients through the heads carry the bounds of
tests/test_gpu_c51.py and tests/test_gpu_dqn.py for the same tile arithmetic on the effective weights (3e-4 of a tensor's largest entry,
with a floor of 1e-3 of the largest gradient); the gradient of a sigma is that of its effective weight times p (one more rounding, 6e-8
relative), so its error is at most the weight gradient's bound times the layer's largest |p|.

The cases: (a) a feature width that is no multiple of 4, a 15-wide advantage layer and a dueling value layer; (b) one (1, 1) layer; (c) rows
that straddle vector and workgroup boundaries (4680 floats = 5 workgroups of 256 groups of 4); (d) ten layers; and, for perturb and grad,
(e) weights whose float count leaves a ragged last group of 1, 3 and 2."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import c51_ref as C
from tests import dqn_ref as R
from tests import noisy_ref as N
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
CASES = {"a": [(6, 8), (8, 4), (4, 15), (4, 5)], "b": [(1, 1)], "c": [(130, 36), (36, 15)], "d": [(4, 4)] * 10}
RAGGED = {"e": [(7, 3), (3, 5), (2, 3)]}
DRAWS = (0, 1, 5)
SEED = 2024
# largest |factor - fp64 restatement| over CASES x DRAWS at SEED, measured on an MI355X (test_factors_against_fp64 logs it)
FACTOR_DEV = 5.333e-6
GAMMA, VMIN, VMAX = 0.9, -1.0, 2.0


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def nanlike(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def err(got, want, floor=0.0):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert torch.isfinite(got).all(), "non-finite entries (an output the kernels did not write?)"
    return (got - want).abs().max().item() / max(want.abs().max().item(), floor, 1e-30)


def run_factors(layers, seed, draw, eps=None):
    lib, L = _lib()
    d = lib.noisy_desc(layers)
    n = L.ocrl_noisy_factor_floats(ctypes.byref(d))
    assert n == N.layout(layers)[1] > 0, L.ocrl_last_error().decode()
    buf = nanlike(n + 8)                                                    # four floats on either side must stay untouched
    fac = buf[4:4 + n]
    lib.check(L.ocrl_noisy_factors(ctypes.byref(d), seed, draw, lib.ptr(eps), lib.ptr(fac), lib.stream()))
    torch.cuda.synchronize()
    assert torch.isnan(buf[:4]).all() and torch.isnan(buf[4 + n:]).all()
    return fac.clone()


def guarded(like):
    """NaN-filled outputs shaped like `like`, each inside a buffer with four guard floats on either side (16-byte aligned)"""
    bufs = [nanlike(t.numel() + 8) for t in like]
    return bufs, [b[4:4 + t.numel()].view(t.shape) for b, t in zip(bufs, like)]


def guards_untouched(bufs):
    return all(torch.isnan(b[:4]).all() and torch.isnan(b[-4:]).all() for b in bufs)


def padding_mask(layers):
    offs, n = N.layout(layers)
    pad = np.ones(n, dtype=bool)
    for (i, o), (a, b) in zip(layers, offs):
        pad[a:a + i] = False
        pad[b:b + o] = False
    return pad


# ------------------------------------------------------------------------------------------------------------ 1. the factors
def test_factors_against_fp64():
    assert 4 * FACTOR_DEV < 1e-3                                            # the condition on the bound: see the docstring
    worst, where = 0.0, None
    for name, layers in CASES.items():
        pad = padding_mask(layers)
        for draw in DRAWS:
            fac = run_factors(layers, SEED, draw)
            want = N.factors(layers, SEED, draw)
            dev = np.abs(fac.cpu().double().numpy() - want).max()
            if dev > worst:
                worst, where = dev, (name, draw)
            assert (fac.cpu().numpy()[pad] == 0).all() and pad.sum() == sum(N.up4(i) - i + N.up4(o) - o for i, o in layers), (name, draw)
            assert torch.isfinite(fac).all() and (fac.cpu().numpy()[~pad] != 0).all()
            assert torch.equal(bits(run_factors(layers, SEED, draw)), bits(fac))                        # the same call twice
    log(f"noisy factors: largest deviation from fp64 {worst:.3e} at case {where[0]} draw {where[1]} (FACTOR_DEV {FACTOR_DEV:.1e}, bound 4 x that "
        f"= {4 * FACTOR_DEV:.1e}, {worst / (4 * FACTOR_DEV):.2f} of it)")
    assert worst <= 4 * FACTOR_DEV


def test_factors_follow_seed_draw_layer_and_side():
    layers = CASES["d"]
    base = run_factors(layers, SEED, 1).cpu()
    assert not torch.equal(run_factors(layers, SEED + 1, 1).cpu(), base) and not torch.equal(run_factors(layers, SEED, 2).cpu(), base)
    assert not torch.equal(run_factors(layers, SEED + (1 << 32), 1).cpu(), base)                         # the seed's high word counts
    assert torch.equal(bits(run_factors(layers, SEED, 1 + (1 << 32))), bits(base))                       # the draw counts mod 2^32
    sp = N.split(layers, base)
    for l in range(10):
        assert not torch.equal(sp[l][0], sp[l][1])                                                       # the side
        for k in range(l):
            assert not torch.equal(sp[l][0], sp[k][0]) and not torch.equal(sp[l][1], sp[k][1])           # the layer
    assert len({float(v) for fi, fo in sp for v in torch.cat([fi, fo])}) == 80                           # no value twice
    # a layer's values do not depend on the layers around it: layer 1 of case a alone is its own stream at index 1 only
    a = N.split(CASES["a"], run_factors(CASES["a"], SEED, 1).cpu())
    alone = N.split(CASES["a"][:2], run_factors(CASES["a"][:2], SEED, 1).cpu())
    assert torch.equal(a[1][0], alone[1][0]) and torch.equal(a[1][1], alone[1][1]) and torch.equal(a[0][0][:4], sp[0][0])


def test_factors_of_a_given_eps():
    for name, layers in CASES.items():
        n = N.layout(layers)[1]
        pad = padding_mask(layers)
        gen = torch.Generator().manual_seed(len(name) + n)
        eps = torch.randn(n, generator=gen) * 2
        vals = np.flatnonzero(~pad)
        eps[vals[0]] = 0.0
        if len(vals) > 2:
            eps[vals[1]], eps[vals[2]] = -4.0, 1e-30
        eps[torch.as_tensor(pad)] = float("nan")                                                          # never read
        fac = run_factors(layers, SEED, 0, eps.cuda()).cpu().numpy()
        want = N.factors(layers, SEED, 0, eps.double().numpy())
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (fac[pad] == 0).all() and (np.abs(fac.astype(np.float64) - want)[~pad] <= 2 * ulp[~pad]).all(), name
        assert fac[vals[0]] == 0.0 and (len(vals) <= 2 or fac[vals[1]] == -2.0)
        assert (np.sign(fac[~pad]) == np.sign(eps.numpy()[~pad])).all()


# ------------------------------------------------------------------------------------------------------------ 2. the distribution
def test_the_draw_is_a_unit_normal():
    layers = [(32768, 32768)]
    f = run_factors(layers, SEED, 3).double()
    n = f.numel()
    assert n == 65536
    g = f * f.abs()
    m1, m2 = g.mean().item(), (g * g).mean().item()
    log(f"noisy distribution: mean {m1:+.4f} (bound {5 / math.sqrt(n):.4f}), second moment {m2:.4f} (1 +- {5 * math.sqrt(2 / n):.4f})")
    assert abs(m1) < 5 / math.sqrt(n) and abs(m2 - 1) < 5 * math.sqrt(2 / n)
    # every index up to 32767 is its own counter: a mis-indexed stream deviates by order 1 nearly everywhere.  1e-3 is the ceiling of
    # test_factors_against_fp64's bound; a thousandth of the values may exceed it (the square root's slope grows towards g = 0)
    close = ((f.cpu() - torch.as_tensor(N.factors(layers, SEED, 3))).abs() <= 1e-3).double().mean().item()
    assert close >= 0.999, close


# ------------------------------------------------------------------------------------------------------------ 3. perturb, 4. grad
@pytest.mark.parametrize("name", list(CASES) + list(RAGGED))
def test_perturb_and_grad_to_the_bit(name):
    lib, L = _lib()
    layers = {**CASES, **RAGGED}[name]
    d = lib.noisy_desc(layers)
    mu, sigma = N.make_layers(layers, seed=31 + len(layers))
    dw = [torch.randn(p.shape, generator=torch.Generator().manual_seed(7 + i)) for i, p in enumerate(mu)]
    for draw in DRAWS[:2]:
        fac = run_factors(layers, SEED, draw)
        md, sd, dd = [p.cuda() for p in mu], [p.cuda() for p in sigma], [p.cuda() for p in dw]
        keep = [t.clone() for t in md + sd + dd]
        bufs, w_eff = guarded(mu)
        lib.check(L.ocrl_noisy_perturb(ctypes.byref(d), lib.ptrs(md), lib.ptrs(sd), lib.ptr(fac), lib.ptrs(w_eff), lib.stream()))
        gbufs, dsigma = guarded(mu)
        lib.check(L.ocrl_noisy_grad(ctypes.byref(d), lib.ptrs(dd), lib.ptr(fac), lib.ptrs(dsigma), lib.stream()))
        torch.cuda.synchronize()
        assert guards_untouched(bufs) and guards_untouched(gbufs)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(md + sd + dd, keep))                    # the inputs are read only
        for q, (got, want) in enumerate(zip(w_eff, N.perturb(layers, mu, sigma, fac))):
            assert torch.equal(bits(got), bits(want)), (name, draw, "w_eff", q, (got.cpu() - want).abs().max().item())
        for q, (got, want) in enumerate(zip(dsigma, N.grad(layers, dw, fac))):
            assert torch.equal(bits(got), bits(want)), (name, draw, "dsigma", q, (got.cpu() - want).abs().max().item())
        assert any((a.cpu() != m).any() for a, m in zip(w_eff, mu))                                       # the noise is there


def noisy_mods(layers, seed=17):
    from ocrl_amd.sb3s import NoisyLinear
    torch.manual_seed(seed)
    mods = [NoisyLinear(i, o).cuda() for i, o in layers]
    for m in mods:                                                          # random sigmas of both signs
        m.weight_sigma.data.normal_(0, 0.3)
        m.bias_sigma.data.normal_(0, 0.3)
    return mods


@pytest.mark.parametrize("name", ["a", "c"])
def test_the_autograd_function_hands_the_gradient_through(name):
    from ocrl_amd.sb3s.noisy import effective_params
    layers = CASES[name]
    mods = noisy_mods(layers)
    assert effective_params(mods, None) == [p for m in mods for p in (m.weight, m.bias)]                 # the means themselves
    w_eff = effective_params(mods, (SEED, 4))
    fac = run_factors(layers, SEED, 4)
    mu = [p.detach().cpu() for m in mods for p in (m.weight, m.bias)]
    sigma = [p.detach().cpu() for m in mods for p in (m.weight_sigma, m.bias_sigma)]
    for got, want in zip(w_eff, N.perturb(layers, mu, sigma, fac)):
        assert got.requires_grad and torch.equal(bits(got), bits(want))
    again = effective_params(mods, (SEED, 4))
    assert all(a.data_ptr() != b.data_ptr() and torch.equal(bits(a), bits(b)) for a, b in zip(w_eff, again))      # regenerated, not cached
    cot = [torch.randn(p.shape, generator=torch.Generator().manual_seed(50 + i)).cuda() for i, p in enumerate(mu)]
    torch.autograd.backward(w_eff, cot)
    want = N.grad(layers, [c.cpu() for c in cot], fac)
    for l, m in enumerate(mods):
        assert torch.equal(bits(m.weight.grad), bits(cot[2 * l])) and torch.equal(bits(m.bias.grad), bits(cot[2 * l + 1]))
        assert torch.equal(bits(m.weight_sigma.grad), bits(want[2 * l])) and torch.equal(bits(m.bias_sigma.grad), bits(want[2 * l + 1]))
    with torch.no_grad():
        assert not any(t.requires_grad for t in effective_params(mods, (SEED, 4)))


# ------------------------------------------------------------------------------------------------------------ 5. mean weights, 6. the heads
def head_policy(categorical, noisy, seed=11):
    """case a's widths: features 6 -> 8 -> 4 -> 15 outputs (15 actions, or 3 actions of 5 atoms with a 5-wide value layer)"""
    from ocrl_amd import sb3s
    kw = dict(n_atoms=5, v_min=VMIN, v_max=VMAX, dueling=True) if categorical else {}
    torch.manual_seed(seed)
    pol = sb3s.DQNPolicy(types.SimpleNamespace(shape=(6,)), types.SimpleNamespace(n=3 if categorical else 15), net_arch=(8, 4), noisy=noisy, **kw).cuda()
    if noisy:
        for k, p in pol.named_parameters():
            if k.endswith("_sigma"):
                p.data.normal_(0, 0.3)
        pol.set_sampling(SEED)
    return pol


def head_mods(pol):
    net = pol.q_net
    return [m for m in net.q_net if isinstance(m, torch.nn.Linear)] + ([net.value_net] if pol.dueling else [])


def head_inputs(categorical):
    gen = torch.Generator().manual_seed(23)
    A = 3 if categorical else 15
    x = torch.randn(5, 6, generator=gen)
    a, r, d = torch.randint(0, A, (5,), generator=gen), torch.rand(5, generator=gen) * 1.5, torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8)
    next_q = torch.randn(5, A, generator=gen)
    next_probs = torch.softmax(torch.randn(5, A, 5, generator=gen), dim=-1)
    return x, a, r, d, next_q, next_probs


@pytest.mark.parametrize("categorical", [False, True], ids=["scalar", "categorical"])
def test_the_mean_weights(categorical):
    pol = head_policy(categorical, True)
    x = head_inputs(categorical)[0].cuda()
    with torch.no_grad():
        pol.set_noise(None)
        mean = pol.q_values(x)
        pol.set_noise(3)
        drawn = pol.q_values(x)
        det = pol.act(x, row_offset=0, deterministic=True)[1]
        assert pol.q_net._noise == (SEED, 3)                                                             # the draw stays chosen
        sampled = pol.act(x, row_offset=0)[1]
        assert not torch.equal(drawn, mean) and torch.equal(bits(det), bits(pol.act(x, row_offset=0, epsilon=0.0, deterministic=True)[1]))
        pol.set_noise(None)
        assert torch.equal(bits(pol.act(x, row_offset=0)[1]), bits(det)) and not torch.equal(sampled, det)
        for k, p in pol.named_parameters():
            if k.endswith("_sigma"):
                p.data.zero_()
        pol.set_noise(3)
        assert torch.equal(bits(pol.q_values(x)), bits(mean))


@pytest.mark.parametrize("categorical", [False, True], ids=["scalar", "categorical"])
def test_through_the_heads(categorical):
    from ocrl_amd import sb3s
    layers = CASES["a"] if categorical else CASES["a"][:3]
    pol, plain = head_policy(categorical, True), head_policy(categorical, False)
    mods = head_mods(pol)
    assert [(m.in_features, m.out_features) for m in mods] == layers
    x, a, r, d, next_q, next_probs = head_inputs(categorical)
    draw = 6
    fac = run_factors(layers, SEED, draw)
    mu = [p.detach().cpu() for m in mods for p in (m.weight, m.bias)]
    sigma = [p.detach().cpu() for m in mods for p in (m.weight_sigma, m.bias_sigma)]
    w_eff = N.perturb(layers, mu, sigma, fac)
    for p, w in zip(plain.q_net._param_list(), w_eff):                       # the unchanged head on hand-perturbed weights
        p.data.copy_(w)
    pol.set_noise(draw)
    with torch.no_grad():
        q, want_q = pol.q_values(x.cuda()), plain.q_values(x.cuda())
        assert torch.equal(bits(q), bits(want_q)) and torch.equal(bits(pol.act(x.cuda(), row_offset=0)[1]), bits(plain.act(x.cuda(), row_offset=0)[1]))
        if categorical:
            assert all(torch.equal(bits(g), bits(w)) for g, w in zip(pol.q_net.distribution(x.cuda()), plain.q_net.distribution(x.cuda())))
    # the gradients of the fused step, against the fp64 chain on w_eff and the chain rule
    if categorical:
        loss, _, _ = sb3s.c51_loss(pol, x.cuda(), next_probs.cuda(), next_q.cuda(), a, r, d, GAMMA)
        scal, _, dw, _ = C.c51_step(x, w_eff, (1, 1), 3, 5, True, VMIN, VMAX, next_probs, next_q, a, r, d, GAMMA)
    else:
        loss, _ = sb3s.dqn_loss(pol, x.cuda(), next_q.cuda(), a, r, d, GAMMA)
        scal, _, dw = R.td_step(x, w_eff, (1, 1), next_q, a, r, d, GAMMA)
    loss.backward()
    assert abs(loss.item() - scal[0].item()) <= 1e-4 * abs(scal[0].item())
    gmax = max(g.abs().max().item() for g in dw)
    sp = N.split(layers, fac.cpu())
    worst_mu = worst_sigma = 0.0
    for l, m in enumerate(mods):
        fi, fo = sp[l]
        p = (fo.unsqueeze(1) * fi.unsqueeze(0)).double()                     # the rounded fp32 product
        for got_mu, got_sigma, w, pp in ((m.weight.grad, m.weight_sigma.grad, dw[2 * l], p), (m.bias.grad, m.bias_sigma.grad, dw[2 * l + 1], fo.double())):
            e = err(got_mu, w, 1e-3 * gmax)
            tol = 3e-4 * max(w.abs().max().item(), 1e-3 * gmax) * pp.abs().max().item()
            es = (got_sigma.detach().cpu().double() - w * pp).abs().max().item() / tol
            worst_mu, worst_sigma = max(worst_mu, e), max(worst_sigma, es)
            assert e <= 3e-4 and es <= 1.0, (l, e, es)
            assert (got_sigma != 0).any()
    log(f"noisy heads {'categorical' if categorical else 'scalar'}: worst mu gradient {worst_mu:.2e} (bound 3e-4), worst sigma gradient "
        f"{worst_sigma:.2f} of its bound")


# ------------------------------------------------------------------------------------------------------------ 7. DQN(noisy=True), 8. noisy=False
LOOP = ["sb3.algo_kwargs.buffer_size=64", "sb3.algo_kwargs.learning_starts=16", "sb3.algo_kwargs.train_freq=4", "sb3.algo_kwargs.target_update_interval=8",
        "sb3.algo_kwargs.batch_size=8", "+sb3.algo_kwargs.log_interval=1", "sb3.algo_kwargs.learning_rate=1e-3", "env.max_steps=6"]


def build_loop(sb3="rainbow", *over):
    """DQN on four on-device Target environments (obs_size 64, read as state rows by the ground-truth encoder)"""
    import train_sb3
    from ocrl_amd.utils.config import compose
    c = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0",
                                   "env.rew_type=dense"] + LOOP + list(over))
    assert c.env.obs_size == 64 and c.num_envs == 4
    return train_sb3.build(c)[2]


def sigmas(model):
    return torch.cat([p.detach().flatten() for k, p in model.policy.named_parameters() if k.endswith("_sigma")])


def test_the_noise_explores_and_the_draws_are_counted():
    from ocrl_amd import sb3s
    model = build_loop()
    assert model.noisy and model.env.on_device and model.n_envs == 4 and model.learning_starts == 16
    lin = [m for m in model.policy.q_net.modules() if isinstance(m, torch.nn.Linear)]
    assert len(lin) == 4 and all(type(m) is sb3s.NoisyLinear for m in lin) and all(type(m) is sb3s.NoisyLinear for m in model.target.q_net.modules()
                                                                                   if isinstance(m, torch.nn.Linear))
    assert (model.policy._sample_seed, model.target._sample_seed) == (model.seed, model.seed + 1)
    # epsilon is 0 from the first step, the warm-up included
    assert model.num_timesteps == 0 < model.learning_starts and model.epsilon() == 0.0 and model.exploration_rate == 0.0 and model.noise_draws == 0
    s0 = sigmas(model).clone()
    for t in range(4):
        model.collect_step()
        assert model.noise_draws == t + 1 and model.policy.q_net._noise == (model.seed, t) and model.exploration_rate == 0.0
    for u in range(2):
        model.train_step()
        assert model.noise_draws == 4 + 2 * (u + 1)
        assert model.policy.q_net._noise == (model.seed, 4 + 2 * u) and model.target.q_net._noise == (model.seed + 1, 5 + 2 * u)
    s1 = sigmas(model)
    assert (s1 != s0).any() and torch.isfinite(s1).all() and model.train_stats()["exploration_rate"] == 0.0
    assert torch.equal(sigmas(types.SimpleNamespace(policy=model.target)), s0)                           # the target stood still
    # every mu zeroed, the same observation in all rows: the rows agree, the steps do not
    for m in lin:
        m.weight.data.zero_()
        m.bias.data.zero_()
    obs = model._last_obs[:1].expand(4, *model._last_obs.shape[1:]).contiguous()
    seen = []
    with torch.no_grad():
        feats = model.policy.extract_features(model._obs(obs))
        for t in range(32):
            model.policy.set_noise(100 + t)
            actions, q, _ = model.policy.act(feats, epsilon=model.epsilon())
            assert (actions == actions[0]).all() and torch.equal(bits(q), bits(q[:1].expand_as(q).contiguous()))
            seen.append(int(actions[0]))
    log(f"noisy exploration: actions of 32 draws on one observation with zero means: {seen}")
    assert len(set(seen)) >= 2


def test_checkpoints_keep_the_noise_stream(tmp_path):
    """save, then load into a fresh instance that collected the same steps (the replay buffer is not part of a checkpoint) and whose
    parameters, Adam state and counters were then wiped: one more iteration is bitwise the uninterrupted run's"""
    path = str(tmp_path / "rainbow.pt")
    model = build_loop()
    model.learn(64)
    assert model.n_updates == 3 and model.noise_draws == 16 + 2 * 3
    model.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["hyper"]["noise_draws"] == 22 and ck["hyper"]["noisy"] is True and ck["hyper"]["noisy_sigma0"] == 0.5 and ck["exploration_rate"] == 0.0
    assert "q_net.value_net.weight_sigma" in ck["policy"] and "q_net.q_net.0.bias_sigma" in ck["target"]
    model.learn(80)
    other = build_loop()
    other.learn(64)
    for t in (other.flat_p, other.flat_target, other.flat_m, other.flat_v):
        t.zero_()
    other.adam_step, other.noise_draws, other.n_updates, other.policy._sample_rows = 0, 0, 0, 0
    assert other.load(path) is other and other.noise_draws == 22 and other.adam_step == 3
    other.learn(80)
    assert model.n_updates == other.n_updates == 4 and model.noise_draws == other.noise_draws == 22 + 4 + 2
    for k in ("flat_p", "flat_target", "flat_m", "flat_v"):
        assert torch.equal(bits(getattr(other, k)), bits(getattr(model, k))), k
    assert other.adam_step == model.adam_step and other.policy._sample_rows == model.policy._sample_rows
    # a checkpoint of the plain head is another layout: refused
    plain = build_loop("dqn_c51")
    with pytest.raises(ValueError, match="Adam entries"):
        plain.load(path)


def test_without_noisy_nothing_changes():
    base, off = build_loop("dqn_c51"), build_loop("dqn_c51", "+sb3.algo_kwargs.noisy=False", "+sb3.algo_kwargs.noisy_sigma0=0.5")
    assert list(base.policy.state_dict()) == list(off.policy.state_dict()) and not off.noisy and not off.policy.noisy
    assert not any("sigma" in k for k in off.policy.state_dict())
    base.learn(48)
    off.learn(48)
    assert base.n_updates == off.n_updates == 2 and off.noise_draws == 0 and off.policy.q_net._noise is None
    for k in ("flat_p", "flat_target", "flat_m", "flat_v"):
        assert torch.equal(bits(getattr(off, k)), bits(getattr(base, k))), k
    assert off.exploration_rate == base.exploration_rate > 0 and torch.equal(base.replay_buffer.priorities, off.replay_buffer.priorities)
