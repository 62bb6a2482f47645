"""GPU checks of DQN's fully parameterized quantile function: the entry points of include/ocrl_hip_fqf.h through the C ABI,
``DQN._train_step_fqf``, checkpoints and ``train_sb3.build``, against the restatement of tests/fqf_ref.py in fp64.

Bounds.  Where the arithmetic is the implicit quantile head's (the quantile values, q, the TD step behind ``train_step``) the bounds are
tests/test_gpu_iqn.py's, unchanged: quantile values within 1e-5 of the largest, q within 1e-4, ``train_step`` on dp / lr within 4 x the
deviation of the fp32 restatement.  For the new arithmetic (the fractions, logp, the entropy, dWf, dbf, the fraction scalars, the
proposal's dp / lr) no number is fixed in advance: a tensor is graded against 4 x the largest deviation of the fp32 torch restatement
from the fp64 one on the very inputs of the case, measured here on the CPU (the rule of tests/test_gpu_c51.py), with a floor of 16 x 2^-24
of the tensor's maximum: N <= 32 serial additions of at most half an ulp each, so the bound is never zero.  The integer rules (actions),
tau_0 = 0, tau_N = 1, the order of a row, the layout of eval_taus and a row's independence of the batch are exact."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import dqn_ref as R
from tests import fqf_ref as FQ
from tests import iqn_ref as I
from tests import qr_ref as Q
from tests import replay_ext_ref as X
from tests.gpu_util import log
from tests.test_gpu_iqn import LAYOUTS, bits, build_loop, err, head_layers, nanlike

pytestmark = pytest.mark.gpu

# (B, F, A, N, C): the smallest; a general small one; odd N, rows that do not fill a wave evenly; N at its limit (63 evaluation fractions);
# F at its limit; many actions; enough rows that the blocks and the partial-sum slabs wrap
SHAPES = [(1, 4, 1, 2, 4), (5, 8, 2, 5, 8), (2, 12, 3, 17, 64), (3, 12, 4, 32, 64), (3, 256, 4, 8, 64), (20, 12, 64, 4, 12), (130, 8, 4, 8, 64)]
ULP16 = 16 * 2.0 ** -24


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def rule(want64, want32):
    """the bound of a tensor of the new arithmetic, absolute: 4 x the fp32 restatement's deviation, at least 16 x 2^-24 of the maximum"""
    return max(4 * (want32.double() - want64).abs().max().item(), ULP16 * want64.abs().max().item())


def dev(got, want64):
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), "non-finite entries (an output the kernel did not write?)"
    return (got - want64).abs().max().item()


def graded(tag, got, want64, want32):
    d, b = dev(got, want64), rule(want64, want32)
    log(f"fqf {tag}: deviation {d:.2e}, bound {b:.2e} (max {want64.abs().max().item():.2e}; {d / b if b else 0:.2f} of it)")
    assert d <= b, (tag, d, b)


# ------------------------------------------------------------------------------------------------------------ 1. the fractions
def run_fractions(x, W, b, only_taus=False):
    lib, L = _lib()
    (B, F), N = x.shape, W.shape[0]
    xs, Ws, bs = x.cuda().contiguous(), W.cuda().contiguous(), b.cuda().contiguous()
    out = [nanlike(B, N + 1), nanlike(B, N), nanlike(B, 2 * N - 1), nanlike(B, N), nanlike(B)]
    ptrs = [lib.ptr(out[0])] + [None if only_taus else lib.ptr(t) for t in out[1:]]
    lib.check(L.ocrl_fqf_fractions(lib.ptr(xs), lib.ptr(Ws), lib.ptr(bs), B, F, N, *ptrs, lib.stream()))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def frac_case(B, F, N, gap):
    """features and a proposal whose soft-max is visibly non-uniform (logits of a standard deviation near 2; at the initialisation's gain
    0.01 every error hides); ``gap``: the upper half of the logits sits 40 lower, so their p underflow towards 0 and the serial sum has
    reached 1 before its last terms"""
    gen = torch.Generator().manual_seed(97 + B + N)
    x = torch.randn(B, F, generator=gen)
    W = torch.randn(N, F, generator=gen) * 2 / F ** 0.5
    b = torch.randn(N, generator=gen) * 0.5
    if gap:
        b[N // 2:] -= 40.0
    return x, W, b


@pytest.mark.parametrize("gap", [False, True], ids=["plain", "gap40"])
@pytest.mark.parametrize("B, F, A, N, C", SHAPES, ids=lambda v: str(v))
def test_fractions_against_fp64(B, F, A, N, C, gap):
    x, W, b = frac_case(B, F, N, gap)
    got = run_fractions(x, W, b)
    want64, want32 = FQ.fractions(x.double(), W.double(), b.double()), FQ.fractions(x, W, b)
    names = ("taus", "tau_hats", "eval_taus", "logp", "entropy")
    for k in (0, 1, 3, 4):
        graded(f"fractions {(B, F, N)} {'gap40' if gap else 'plain'} {names[k]}", got[k], want64[k], want32[k])
    taus, hats, ev, logp, H = (t.cpu() for t in got)
    p = want64[3].exp()
    assert p.max() > 3 * p.min() and (not gap or (p.min() < 1e-15 and math.isfinite(logp.min().item()) and logp.min() < -35))
    # the exact facts
    assert (taus[:, 0] == 0).all() and (taus[:, N] == 1).all() and (taus[:, 1:] >= taus[:, :-1]).all()
    assert torch.equal(bits(ev), bits(torch.cat([taus[:, 1:N], hats], dim=1))) and torch.equal(bits(hats), bits(0.5 * (taus[:, :-1] + taus[:, 1:])))
    alone = run_fractions(x[:1], W, b)                                       # a row's results do not change with B
    assert all(torch.equal(bits(a), bits(g[:1])) for a, g in zip(alone, got))
    if B > 2:
        last = run_fractions(x[B - 2:], W, b)
        assert all(torch.equal(bits(a), bits(g[B - 2:])) for a, g in zip(last, got))
    only = run_fractions(x, W, b, only_taus=True)                            # every output but taus may be NULL
    assert torch.equal(bits(only[0]), bits(got[0])) and all(torch.isnan(t).all() for t in only[1:])


# ------------------------------------------------------------------------------------------------------------ 2. q and acting, 3. the fraction loss
def run_theta(x, fr, ps, layout, A, C):
    """ocrl_iqn_fwd's quantile values at the fractions fr [B, M] (a GPU tensor)"""
    lib, L = _lib()
    (B, F), M = x.shape, fr.shape[1]
    d = lib.iqn_desc(B, F, A, M, C, *layout)
    xs, pd, th = x.cuda(), [p.cuda() for p in ps], nanlike(B, A, M)
    lib.check(L.ocrl_iqn_fwd(ctypes.byref(d), lib.ptr(xs), lib.ptr(fr.contiguous()), lib.ptrs(pd), lib.ptr(th), None, 0, None, 0, lib.stream()))
    torch.cuda.synchronize()
    return th


def run_q(theta, taus):
    lib, L = _lib()
    B, A, N = theta.shape
    q = nanlike(B, A)
    lib.check(L.ocrl_fqf_q(lib.ptr(theta), lib.ptr(taus), B, A, N, lib.ptr(q), lib.stream()))
    torch.cuda.synchronize()
    return q


def run_act(x, taus, ps, layout, A, N, C, seed, row_offset, epsilon, uniforms=None, want_q=True):
    lib, L = _lib()
    B, F = x.shape
    d = lib.fqf_desc(B, F, A, N, C, *layout)
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    u = None if uniforms is None else torch.as_tensor(uniforms).cuda().contiguous()
    actions, q = torch.full((B,), -7, device="cuda", dtype=torch.int64), nanlike(B, A) if want_q else None
    lib.check(L.ocrl_fqf_act(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(taus), seed, row_offset, epsilon, lib.ptr(u), lib.ptr(actions), lib.ptr(q),
                             lib.stream()))
    torch.cuda.synchronize()
    return actions.cpu().numpy(), None if q is None else q.cpu()


@functools.lru_cache(maxsize=None)
def head_case(B, F, A, N, C, lname):
    """the head's parameters beside frac_case's inputs, and what the GPU makes of them, once: the fractions, the quantile values at
    tau_hats and at eval_taus"""
    x, W, b = frac_case(B, F, N, False)
    ps = I.make_params(F, A, C, LAYOUTS[lname][0], 83)
    taus, hats, ev, logp, H = run_fractions(x, W, b)
    return dict(x=x, W=W, b=b, ps=ps, taus=taus, hats=hats, ev=ev, logp=logp, H=H, theta=run_theta(x, hats, ps, LAYOUTS[lname], A, C),
                theta_eval=run_theta(x, ev, ps, LAYOUTS[lname], A, C))


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A, N, C", SHAPES, ids=lambda v: str(v))
def test_q_and_act(B, F, A, N, C, lname):
    c, layout = head_case(B, F, A, N, C, lname), LAYOUTS[lname]
    x, ps, taus = c["x"], c["ps"], c["taus"]
    q = run_q(c["theta"], taus)
    wt, wq = FQ.act_q(x.double(), taus.cpu().double(), [p.double() for p in ps], layout[1], A, C)
    e_t, e_q = err(c["theta"], wt), err(q, wq)
    e_own = err(q, FQ.weighted_q(c["theta"].cpu().double(), taus.cpu().double()))          # the fold alone, on the GPU's own quantile values
    log(f"fqf q {(B, F, A, N, C)} {lname}: theta {e_t:.2e} (bound 1e-5), q {e_q:.2e} (bound 1e-4), the fold alone {e_own:.2e}")
    assert e_t <= 1e-5 and e_q <= 1e-4 and e_own <= 1e-4
    gen = torch.Generator().manual_seed(5 + N)
    u = (torch.randint(0, 2 ** 24, (B, 2), generator=gen).float() / 2 ** 24).numpy()
    actions, qa = run_act(x, taus, ps, layout, A, N, C, 3, 0, 0.3, u)
    assert torch.equal(bits(qa), bits(q))                                    # ocrl_fqf_act's q is ocrl_fqf_q(ocrl_iqn_fwd(tau_hats)) bit for bit
    want, explore = R.act_rule(qa.numpy(), u, 0.3)
    assert np.array_equal(actions, want)
    greedy, none = run_act(x, taus, ps, layout, A, N, C, 3, 0, 0.0, u, want_q=False)
    rand, _ = run_act(x, taus, ps, layout, A, N, C, 3, 0, 1.0, u)
    assert none is None and np.array_equal(greedy, qa.numpy().argmax(axis=1)) and np.array_equal(rand, R.act_rule(qa.numpy(), u, 1.0)[0])
    # without uniforms the coin is ocrl_dqn_act's draw; a row's result does not depend on how the batch is split
    lib, L = _lib()
    du = nanlike(B, 2)
    lib.check(L.ocrl_dqn_act_uniforms(11, 1000, B, lib.ptr(du), lib.stream()))
    du = du.cpu().numpy()
    whole, qw = run_act(x, taus, ps, layout, A, N, C, 11, 1000, 0.3)
    given, qg = run_act(x, taus, ps, layout, A, N, C, 11, 1000, 0.3, du)
    assert np.array_equal(whole, given) and torch.equal(bits(qw), bits(qg)) and torch.equal(bits(qw), bits(q))
    assert np.array_equal(whole, R.act_rule(qw.numpy(), du, 0.3)[0])
    if B > 1:
        k = B // 2
        parts = [run_act(x[a:e], taus[a:e].contiguous(), ps, layout, A, N, C, 11, 1000 + a, 0.3) for a, e in ((0, k), (k, B))]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), whole) and torch.equal(bits(torch.cat([p[1] for p in parts])), bits(qw))


def test_act_explores_every_action_and_breaks_ties_low():
    B, F, A, N, C, layout = 512, 12, 5, 17, 64, LAYOUTS["mlp"]
    gen = torch.Generator().manual_seed(8)
    x, ps = torch.randn(B, F, generator=gen), I.make_params(F, A, C, layout[0], 17)
    W, b = torch.randn(N, F, generator=gen) / F ** 0.5, torch.zeros(N)
    taus = run_fractions(x, W, b)[0]
    u = (torch.randint(0, 2 ** 24, (B, 2), generator=gen).float() / 2 ** 24).numpy()
    actions, q = run_act(x, taus, ps, layout, A, N, C, 3, 0, 0.3, u)
    want, explore = R.act_rule(q.numpy(), u, 0.3)
    assert np.array_equal(actions, want) and 0.2 < explore.mean() < 0.4 and set(actions[explore].tolist()) == set(range(A))
    tie = [p.clone() for p in ps]
    tie[-2][:] = tie[-2][0]                                                  # every action's output row the same: q ties, the lowest index wins
    tie[-1][:] = tie[-1][0]
    actions, q = run_act(x, taus, tie, layout, A, N, C, 3, 0, 0.0, u)
    assert (q == q[:, :1]).all() and (actions == 0).all()


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A, N, C", SHAPES, ids=lambda v: str(v))
def test_fraction_bwd_against_fp64(B, F, A, N, C, lname):
    lib, L = _lib()
    c = head_case(B, F, A, N, C, lname)
    gen = torch.Generator().manual_seed(41 + B)
    actions = torch.randint(0, A, (B,), generator=gen)
    if B > 1:
        actions[0], actions[-1] = -3, A + 5                                   # two actions outside [0, A)
    weights = torch.rand(B, generator=gen) * 0.9 + 0.1
    n = L.ocrl_fqf_ws_floats(B, F, N)
    assert n > 0, L.ocrl_last_error().decode()
    xs, acts = c["x"].cuda(), actions.cuda()
    x32, logp32, H32, th32 = c["x"], c["logp"].cpu(), c["H"].cpu(), c["theta_eval"].cpu()          # the GPU's own logp and quantile values
    th_a = th32[torch.arange(B), actions.clamp(0, A - 1)]
    assert (FQ.g_analytic(th_a[:, :N - 1], th_a[:, N - 1:]).abs() > 0).any()
    for wts, ent in ((None, 0.0), (weights, 0.01), (None, 0.01), (weights, 0.0)):
        dW, db, scal, ws = nanlike(N, F), nanlike(N), nanlike(2), nanlike(n)
        lib.check(L.ocrl_fqf_fraction_bwd(lib.ptr(xs), lib.ptr(c["logp"]), lib.ptr(c["H"]), lib.ptr(c["theta_eval"]), lib.ptr(acts),
                                          lib.ptr(None if wts is None else wts.cuda()), ent, B, F, A, N, lib.ptr(dW), lib.ptr(db), lib.ptr(scal), lib.ptr(ws),
                                          n, lib.stream()))
        torch.cuda.synchronize()
        w64 = FQ.fraction_grads(x32.double(), logp32.double(), H32.double(), th32.double(), actions, None if wts is None else wts.double(), ent)
        w32 = FQ.fraction_grads(x32, logp32, H32, th32, actions, wts, ent)
        tag = f"fraction_bwd {(B, F, A, N, C)} {lname} {'weights' if wts is not None else 'no weights'} ent_coef {ent}"
        for name, g, a, b in zip(("dWf", "dbf"), (dW, db), w64, w32):
            graded(f"{tag} {name}", g, a, b)
        for k, name in enumerate(("fraction loss", "mean entropy")):
            graded(f"{tag} {name}", scal[k:k + 1], w64[2][k:k + 1], w32[2][k:k + 1])
        again = [nanlike(N, F), nanlike(N), nanlike(2)]
        lib.check(L.ocrl_fqf_fraction_bwd(lib.ptr(xs), lib.ptr(c["logp"]), lib.ptr(c["H"]), lib.ptr(c["theta_eval"]), lib.ptr(acts),
                                          lib.ptr(None if wts is None else wts.cuda()), ent, B, F, A, N, *(lib.ptr(t) for t in again), lib.ptr(ws), n,
                                          lib.stream()))
        torch.cuda.synchronize()
        assert all(torch.equal(bits(a), bits(g)) for a, g in zip(again, (dW, db, scal)))          # overwritten, not accumulated; reproducible


# ------------------------------------------------------------------------------------------------------------ 4. DQN(fqf=True)
UPDATES = 3
FRAC_LR = 1e-3                  # at the paper's 2.5e-9 the proposal's step is a handful of ulps of its weights
FQF = ["sb3.algo_kwargs.n_tau_samples=8", f"sb3.algo_kwargs.fqf_fraction_lr={FRAC_LR}", "sb3.algo_kwargs.fqf_ent_coef=0.01"]
VARIANTS = {"plain": ["sb3.algo_kwargs.double_q=False", "sb3.algo_kwargs.n_step=1", "sb3.algo_kwargs.prioritized_replay=False", "sb3.algo_kwargs.noisy=False"],
            "extended": ["sb3.algo_kwargs.noisy=False"],                      # double Q + 3-step returns + prioritized replay
            "noisy": []}                                                      # ... and noisy layers: fqf.yaml as it stands


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_three_updates_against_the_restatement(variant):
    """DQN(fqf=True, n_tau_samples=8) on four Target environments, plain, then with double Q + n-step + prioritized replay, then with
    noisy layers too: three train_step() calls against the restatement fed the batches and the fractions the run produced, on dp / lr for
    the policy's parameters (clip + Adam) and for the proposal's (RMSprop at fqf_fraction_lr = 1e-3)"""
    from ocrl_amd import sb3s
    from ocrl_amd.sb3s.noisy import draw_factors
    N, BS = 8, 8
    model = build_loop("fqf", *FQF, *VARIANTS[variant])
    noisy, per, n_step = variant == "noisy", variant != "plain", 1 if variant == "plain" else 3
    assert type(model.policy.q_net) is sb3s.FullyParameterizedQuantileQNetwork and type(model.target.q_net) is sb3s.FullyParameterizedQuantileQNetwork
    assert (model.fqf, model.fqf_fraction_lr, model.fqf_ent_coef, model.n_tau_samples, model.n_tau_prime_samples, model.n_cos, model.double_q, model.n_step,
            model.prioritized_replay, model.noisy) == (True, FRAC_LR, 0.01, N, 0, 64, per, n_step, per, noisy)
    for _ in range(8):
        model.collect_step()
    buf = model.replay_buffer
    assert buf.n_slots == 16 and buf.pos == 8 and torch.equal(model.flat_target, model.flat_p)
    every = [p.detach().cpu().clone() for p in model.policy.parameters() if p.requires_grad]
    ps0, frac0 = every[:-2], every[-2:]                                      # the proposal is the last module of the head
    F = model.policy.features_dim
    assert tuple(frac0[0].shape) == (N, F) and tuple(frac0[1].shape) == (N,) and tuple(ps0[-2].shape) == (F, 64)
    assert sum(p.numel() for p in model._params) == sum(p.numel() for p in ps0) and model.frac_p.numel() == N * F + N
    n_plain = sum(1 for _ in model.policy.features_extractor._pooling.parameters())
    acts = model.policy.q_net._layout()[1]
    layers = head_layers(model.policy)
    lr = model.learning_rate
    NE = 16 * 4
    batches, frs, leaves, facs = [], [], [], []
    for u in range(UPDATES):
        if per:
            idx, w = buf.sample_prioritized(BS, model.n_updates, model.beta())               # what train_step is about to draw: a pure function
        else:
            idx, w = buf.sample_indices(BS, model.n_updates, n_step), None
        b = buf.gather(idx, n_step, model.gamma) if n_step > 1 else buf.gather(idx)
        batches.append(tuple(None if t is None else t.cpu() for t in (model._obs(b.observations), model._obs(b.next_observations), b.actions, b.rewards,
                                                                      b.dones, b.discounts, w)))
        if noisy:                                                                            # the step's two draws, as the GPU writes them
            facs.append((draw_factors(layers, model.seed, model.noise_draws, model.device)[1].cpu(),
                         draw_factors(layers, model.seed + 1, model.noise_draws + 1, model.device)[1].cpu()))
        model.train_step()
        frs.append(tuple(t.cpu() for t in model.last_fractions))                             # the fractions the step proposed
        if per:
            assert torch.equal(model.last_weights, w)
            leaves.append((idx.cpu().numpy(), X.parse_store(buf.priorities.cpu().numpy(), NE)[0]))
    assert model.n_updates == UPDATES and all(torch.equal(t.cpu(), p0) for t, p0 in zip(model.target.parameters(), every))      # the target stood still
    taus = frs[0][0]
    assert (taus[:, 0] == 0).all() and (taus[:, -1] == 1).all() and (taus[:, 1:] >= taus[:, :-1]).all() and not torch.equal(frs[0][0], frs[1][0])

    def split(ps, fac=None):
        chain = list(ps[:-2]) if fac is None else Q.noisy_chain(list(ps[:-2]), n_plain, layers, fac)
        return chain[:n_plain], list(ps[-2:]) + chain[n_plain:]

    def ref(dtype):
        cur, m, v = [p.to(dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0]
        frac, sq = [p.to(dtype) for p in frac0], torch.ones(N * F + N, dtype=dtype)
        out = []
        for step, (batch, fr) in enumerate(zip(batches, frs), 1):
            fo, ft = facs[step - 1] if noisy else (None, None)
            cur, m, v, scal, ql, frac, sq, fscal = FQ.train_step(cur, ps0, m, v, step, batch, fr, acts, 4, 64, model.gamma, model.huber_kappa, model.double_q,
                                                                  lr, model.max_grad_norm, lambda ps, f=fo: split(ps, f), lambda ps, f=ft: split(ps, f), frac, sq,
                                                                  FRAC_LR, model.fqf_ent_coef, dtype)
            out.append((scal, ql, fscal))
        return cur, list(frac), sq, out
    p64, f64_, sq64, out64 = ref(torch.float64)
    p32, f32_, sq32, out32 = ref(torch.float32)
    step_of = lambda new, old: [a.double() - o.double() for a, o in zip(new, old)]
    worst_of = lambda a, b: max((x - y).abs().max().item() for x, y in zip(a, b))
    got = [p.detach().cpu() for p in model.policy.parameters() if p.requires_grad]
    dev_p = worst_of(step_of(p32, ps0), step_of(p64, ps0)) / lr
    worst_p = worst_of(step_of(got[:-2], ps0), step_of(p64, ps0)) / lr
    log(f"fqf train_step {variant}: policy worst dp/lr deviation {worst_p:.2e}; the fp32 restatement's {dev_p:.2e} (bound 4 x that: {4 * dev_p:.2e}, "
        f"{worst_p / (4 * dev_p):.2f} of it)")
    big = max(s.abs().max().item() for s in step_of(f64_, frac0)) / FRAC_LR
    dev_f = worst_of(step_of(f32_, frac0), step_of(f64_, frac0)) / FRAC_LR
    worst_f = worst_of(step_of(got[-2:], frac0), step_of(f64_, frac0)) / FRAC_LR
    bound_f = max(4 * dev_f, ULP16 * big)
    log(f"fqf train_step {variant}: proposal worst dp/lr deviation {worst_f:.2e}; the fp32 restatement's {dev_f:.2e} (bound {bound_f:.2e}, "
        f"{worst_f / bound_f:.2f} of it; largest dp/lr {big:.2e})")
    assert all((g != p0).any() for g, p0 in zip(got, every)) and worst_p <= 4 * dev_p and worst_f <= bound_f
    e_sq = err(model.frac_sq[:N * F + N], sq64)
    assert e_sq <= 1e-6, e_sq
    # the priorities written back are the rows' quantile losses (test_gpu_iqn.py's check)
    for (idx, lv), (_, ql, _) in zip(leaves, out64):
        ql = np.array([ql.numpy()[idx == i].max() for i in idx])
        want = X.quantise64(ql, model.prioritized_replay_alpha, model.prioritized_replay_eps)
        assert (np.abs(lv[idx] - want) <= 1 + 3e-4 * want).all(), (lv[idx], want)
    st = model.train_stats()
    for i, k in enumerate(("loss", "mean_q", "mean_target")):
        want = sum(s[i].item() for s, _, _ in out64) / UPDATES
        assert abs(st[k] - want) <= 1e-4 * max(abs(want), 1e-3 * max(s.abs().max().item() for s, _, _ in out64)), (k, st[k], want)
    for i, k in enumerate(("fraction_loss", "fraction_entropy")):
        w64 = torch.stack([f[i] for _, _, f in out64]).mean().reshape(1)
        w32 = torch.stack([f[i] for _, _, f in out32]).double().mean().reshape(1)
        scale = torch.stack([f[i] for _, _, f in out64]).abs().max().reshape(1)
        bound = max(rule(w64, w32), ULP16 * scale.item())
        log(f"fqf train_step {variant}: {k} {st[k]:.6e}, the restatement's {w64.item():.6e} (bound {bound:.2e})")
        assert abs(st[k] - w64.item()) <= bound, (k, st[k], w64.item(), bound)
    assert 0.0 < st["fraction_entropy"] <= math.log(N) + 1e-5


def test_checkpoints_round_trip_and_an_iqn_checkpoint_stays_iqn(tmp_path):
    """save / load reproduces the next step bit for bit; an IQN checkpoint of a version without the keys loads with fqf off; a mismatch
    is refused by the key's name"""
    def run():
        model = build_loop("fqf", *FQF)
        model.learn(96)
        return model
    model, twin = run(), run()
    assert model.n_updates == 5 and torch.equal(twin.flat_p, model.flat_p) and torch.equal(twin.frac_p, model.frac_p) and torch.equal(twin.frac_sq, model.frac_sq)
    assert torch.isfinite(model.flat_p).all() and torch.isfinite(model.frac_p).all() and (model.frac_sq != 1).any()
    path = str(tmp_path / "fqf.pt")
    model.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert (ck["hyper"]["fqf"], ck["hyper"]["fqf_fraction_lr"], ck["hyper"]["fqf_ent_coef"]) == (True, FRAC_LR, 0.01)
    assert torch.equal(ck["optimizer"]["frac_sq"], model.frac_sq.cpu()) and torch.equal(ck["policy"]["q_net.fraction_net.weight"].flatten(), model.frac_p[:-8].cpu())
    for k in ("flat_p", "flat_target", "flat_m", "flat_v", "frac_p", "frac_sq"):                 # the twin keeps its replay ring and loses everything else
        getattr(twin, k).add_(0.5)
    assert twin.load(path) is twin
    for k in ("flat_p", "flat_target", "flat_m", "flat_v", "frac_p", "frac_sq"):
        assert torch.equal(getattr(twin, k), getattr(model, k)), k
    obs = model._last_obs.clone()
    assert np.array_equal(model.predict(obs, deterministic=True)[0], twin.predict(obs, deterministic=True)[0])
    model.train_step()
    twin.train_step()
    for k in ("flat_p", "flat_m", "flat_v", "frac_p", "frac_g", "frac_sq"):
        assert torch.equal(bits(getattr(twin, k)), bits(getattr(model, k))), k
    # an IQN checkpoint as an earlier version wrote it
    iqn = build_loop("iqn")
    old = str(tmp_path / "iqn.pt")
    iqn.save(old)
    ck = torch.load(old, map_location="cpu", weights_only=True)
    for k in ("fqf", "fqf_fraction_lr", "fqf_ent_coef"):
        del ck["hyper"][k]
    torch.save(ck, old)
    other = build_loop("iqn", "seed=5")
    assert other.load(old) is other and other.fqf is False and torch.equal(other.flat_p, iqn.flat_p) and not hasattr(other, "frac_p")
    keep = model.flat_p.clone()
    with pytest.raises(ValueError, match="the checkpoint was written with fqf = False, this instance has fqf = True"):
        build_loop("fqf", "sb3.algo_kwargs.n_tau_samples=8", "sb3.algo_kwargs.n_tau_prime_samples=8").load(old)
    with pytest.raises(ValueError, match="the checkpoint was written with fqf = True, this instance has fqf = False"):
        build_loop("iqn", "sb3.algo_kwargs.n_tau_prime_samples=0").load(path)
    assert torch.equal(model.flat_p, keep)


def test_train_sb3_build_runs_fqf_and_logs_the_two_stats():
    """sb3=fqf as configs/sb3/fqf.yaml has it (32 fractions, the paper's learning rate), on 4 environments: a short learn() whose
    callback rows carry fraction_loss and fraction_entropy"""
    from ocrl_amd import sb3s
    model = build_loop("fqf")
    assert type(model.policy.q_net) is sb3s.FullyParameterizedQuantileQNetwork and (model.n_tau_samples, model.fqf_fraction_lr) == (32, 2.5e-9)
    rows = []
    model.learn(96, callback=lambda loc: rows.append(dict(loc["train"])))
    assert model.n_updates == 5 and len(rows) == 6
    assert all({"fraction_loss", "fraction_entropy", "loss"} <= set(r) for r in rows) and math.isnan(rows[0]["fraction_loss"])
    for r in rows[1:]:
        assert math.isfinite(r["fraction_loss"]) and 0.0 < r["fraction_entropy"] <= math.log(32) + 1e-5 and math.isfinite(r["loss"]), r
    log(f"fqf learn(96): {rows[-1]}")
    obs = model._last_obs.clone()
    a = model.predict(obs, deterministic=True)[0]
    assert np.array_equal(model.predict(obs, deterministic=True)[0], a)      # evaluation uses the proposed fractions: a function of the observation
    q = model.policy.q_values(model._obs(obs))                               # attached to autograd through the head
    assert q.requires_grad and q.shape == (4, 4)
    with torch.no_grad():
        assert err(q, model.policy.q_values(model._obs(obs)).cpu().double()) <= 1e-5


def parent_train_step(model):
    """``DQN.train_step`` as it stood before fqf existed, for the implicit quantile head, spelled out on the model's own parts"""
    batch, idx, weights = model._draw_batch()
    model._draw_train_noise()
    loss, m, row_err = model._train_step_iqn(batch, weights)
    loss.backward()
    model._adam_step()
    if model.prioritized_replay:
        same = idx.unsqueeze(1) == idx.unsqueeze(0)
        row_err = torch.where(same, row_err.unsqueeze(0), row_err.new_full((), -math.inf)).amax(dim=1)
        model.replay_buffer.update_priorities(idx, row_err, model.prioritized_replay_alpha, model.prioritized_replay_eps)
        model.last_weights = weights
    model.n_updates += 1
    model._acc += torch.cat([torch.stack([m[k] for k in ("loss", "mean_q", "mean_target")]), model._norm])
    model._acc_n += 1


def test_without_fqf_the_step_is_iqns_bit_for_bit():
    """DQN(n_tau_samples=8) without fqf dispatches _train_step_iqn, owns no fraction buffers, and its three train_step() calls are bit
    for bit the step as it stood before fqf existed (``parent_train_step``), also with the new keywords spelled out at their defaults"""
    def never(*a):
        raise AssertionError("the FQF step ran with fqf = False")

    def three(step, *over):
        model = build_loop("iqn", *over)
        assert model.fqf is False and not hasattr(model, "frac_p") and not hasattr(model, "frac_g") and not hasattr(model, "frac_sq")
        assert not hasattr(model.policy.q_net, "fraction_net") and not any("fraction" in k for k in model.policy.state_dict())
        taken, inner = [], model._train_step_iqn
        model._train_step_iqn = lambda *a: (taken.append(1), inner(*a))[1]
        model._train_step_fqf = model._fraction_step = never
        for _ in range(8):
            model.collect_step()
        for _ in range(3):
            step(model)
        assert len(taken) == 3 and model.n_updates == 3 and "fraction_loss" not in model.train_stats()
        return model
    a = three(lambda m: m.train_step())
    b = three(lambda m: m.train_step(), "+sb3.algo_kwargs.fqf=False", "+sb3.algo_kwargs.fqf_fraction_lr=2.5e-9", "+sb3.algo_kwargs.fqf_ent_coef=0.0")
    c = three(parent_train_step)
    for other in (b, c):
        for k in ("flat_p", "flat_m", "flat_v", "flat_target"):
            assert torch.equal(bits(getattr(a, k)), bits(getattr(other, k))), k
        assert torch.equal(a.replay_buffer.priorities, other.replay_buffer.priorities)
