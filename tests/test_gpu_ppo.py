"""GPU checks of the PPO loop (ocrl_amd.sb3s.ppo) and its two C entry points against the fp64 restatement of tests/ppo_ref.py:
ocrl_acnet_act (sampling inside the head's launch) with injected and with drawn uniforms, ocrl_flat_clip_adam_l2, one PPO.train(),
collect_rollouts on a scripted environment, and learn() end to end.

Bounds.  Forward outputs (values, log_prob, logits): 1e-4 of each output's maximum, tests/test_gpu_acnet.py's bound for Gaussian data.
Actions: exact wherever the fp64 interval of u that maps to them is wider than 1e-4 and u is its midpoint.  The six PPO scalars: 1e-4 with
the 1e-3 floor of tests/test_gpu_acnet.py.  Updates are graded on dp / lr, elementwise, against the fp64 restatement; the bound is 4 x the
deviation of the fp32 torch restatement (clip_grad_norm_ + torch.optim.Adam(eps = 1e-5)) from the fp64 one on the very inputs of the test,
measured on a CPU (ppo_ref.torch_clip_adam_l2 / ppo_ref.train(torch_step=True)) and written at STEP_DEV / TRAIN_DEV below; the factor 4
is for the different summation order of the norm (and, in train(), of the MFMA products)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import acnet_ref as R
from tests import ppo_ref as P
from tests.gpu_util import log
from tests.test_gpu_acnet import IDENT, MLP, _acnet_cfg, err, make_params, make_x, nanlike

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-4
# largest |dp_fp32 / lr - dp_fp64 / lr| of the torch restatement over every case of test_flat_clip_adam_step (measured on a CPU: 5.17e-6)
STEP_DEV = 5.2e-6
# the same over every parameter of test_train_against_the_restatement's eight updates (measured on a CPU: 5.42e-5 of updates that reach 8.1)
TRAIN_DEV = 5.4e-5


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def run_act(x, ps, layout, A, seed=0, offset=0, uniforms=None, det=0, want_logits=True):
    lib, L = _lib()
    dims, acts = layout
    B, F = x.shape
    d = lib.acnet_desc(B, F, A, dims, acts)
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    u = None if uniforms is None else uniforms.float().cuda().contiguous()
    actions = torch.full((B,), -7, device="cuda", dtype=torch.int64)
    values, logp, logits = nanlike(B), nanlike(B), nanlike(B, A) if want_logits else None
    rc = L.ocrl_acnet_act(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), seed, offset, lib.ptr(u), det, lib.ptr(actions), lib.ptr(values), lib.ptr(logp),
                          lib.ptr(logits), lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ocrl_last_error().decode()
    return types.SimpleNamespace(actions=actions.cpu(), values=values.cpu(), logp=logp.cpu(), logits=None if logits is None else logits.cpu())


def dump_uniforms(seed, offset, n):
    lib, L = _lib()
    out = nanlike(n)
    lib.check(L.ocrl_acnet_act_uniforms(seed, offset, n, lib.ptr(out), lib.stream()))
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------------------ 1. injected uniforms
@pytest.mark.parametrize("layout", [IDENT, MLP], ids=["ident", "mlp"])
@pytest.mark.parametrize("B,F,A", [(1, 4, 1), (5, 8, 2), (37, 128, 4), (64, 12, 64)])
def test_sampler_against_the_restatement_on_midpoint_uniforms(B, F, A, layout):
    ps, x = make_params(F, A, layout[0], 41), make_x(B, F, 42)
    _, _, lg64, vl64 = R.forward(x.double(), [p.double() for p in ps], *layout)
    mid, width = P.intervals(lg64)
    wide = width > 1e-4
    skipped = 1.0 - wide.double().mean().item()
    log(f"act B{B} F{F} A{A}: {skipped:.4f} of the intervals are narrower than 1e-4")
    assert skipped <= (0.02 if A == 64 else 0.0)
    for a in range(A):
        got = run_act(x, ps, layout, A, uniforms=mid[:, a], want_logits=a == 0)
        assert ((got.actions >= 0) & (got.actions < A)).all()
        rows = wide[:, a]
        assert torch.equal(got.actions[rows], torch.full((int(rows.sum()),), a)), (a, got.actions.tolist())
        e_v, e_lp = err(got.values, vl64), err(got.logp, P.log_prob(lg64, got.actions), 1e-3)
        assert e_v <= OUT_TOL and e_lp <= OUT_TOL, (a, e_v, e_lp)
        if a == 0:
            e_lg = err(got.logits, lg64)
            log(f"act B{B} F{F} A{A}: values {e_v:.2e} log_prob {e_lp:.2e} logits {e_lg:.2e}")
            assert e_lg <= OUT_TOL
    det = run_act(x, ps, layout, A, det=1)
    assert torch.equal(det.actions, P.argmax_lowest(det.logits))
    assert err(det.logp, P.log_prob(lg64, det.actions), 1e-3) <= OUT_TOL


def _constant_logits(row, B):
    """(x, parameters) of the empty layout whose logits are `row` on every one of B rows: a zero action_net.weight under the bias"""
    A = len(row)
    return make_x(B, 4, 43), [torch.zeros(A, 4), torch.tensor(row), torch.zeros(1, 4), torch.zeros(1)]


def test_deterministic_takes_the_lowest_index_of_equal_maxima():
    x, ps = _constant_logits([1.0, 3.0, 3.0, 0.0], 19)
    got = run_act(x, ps, IDENT, 4, det=1)
    assert got.actions.tolist() == [1] * 19
    assert err(got.logp, P.log_prob(got.logits, got.actions)) <= OUT_TOL
    lib, L = _lib()
    d = lib.acnet_desc(19, 4, 0, *IDENT)
    out = torch.full((19,), -7, device="cuda", dtype=torch.int64)
    f = nanlike(19)
    assert L.ocrl_acnet_act(ctypes.byref(d), lib.ptr(x.cuda()), None, 0, 0, None, 1, lib.ptr(out), lib.ptr(f), lib.ptr(f), None, lib.stream()) != 0
    assert "heads" in L.ocrl_last_error().decode()
    torch.cuda.synchronize()
    assert (out == -7).all()


# ------------------------------------------------------------------------------------------------------------ 2. the drawn stream
def test_drawn_stream_is_the_dumped_one_and_rows_are_independent():
    B, F, A, seed = 8, 12, 4, 2024
    ps, x = make_params(F, A, MLP[0], 44), make_x(B, F, 45)
    drawn = run_act(x, ps, MLP, A, seed=seed)
    u = dump_uniforms(seed, 0, B)
    assert ((u >= 0) & (u < 1)).all() and torch.equal(u, P.uniforms(seed, 0, B))
    fed = run_act(x, ps, MLP, A, uniforms=u)
    for k in ("actions", "values", "logp", "logits"):
        assert torch.equal(getattr(drawn, k), getattr(fed, k)), k
    lo, hi = run_act(x[:4], ps, MLP, A, seed=seed), run_act(x[4:], ps, MLP, A, seed=seed, offset=4)
    for k in ("actions", "values", "logp", "logits"):
        assert torch.equal(torch.cat([getattr(lo, k), getattr(hi, k)]), getattr(drawn, k)), k
    assert torch.equal(dump_uniforms(seed, 4, 4), u[4:])
    other = run_act(x, ps, MLP, A, seed=seed + 1)
    assert not torch.equal(other.actions, drawn.actions)
    big = dump_uniforms(seed, 2 ** 32 - 3, 6)                            # across the 2^32 boundary of the counter: the key changes
    assert ((big >= 0) & (big < 1)).all() and torch.equal(big[:3], P.uniforms(seed, 2 ** 32 - 3, 3))


def test_action_frequencies_follow_the_probabilities():
    """Pearson's chi-square of 65 536 draws of one logit row against its fp64 probabilities, 4 degrees of freedom: below 33.4, the
    1 - 1e-6 quantile.  The seed is fixed, the result deterministic (the host restatement of the stream gives 3.43 for it)."""
    row, B, seed = [0.3, -1.2, 1.1, 0.0, -0.4], 65536, 2024
    x, ps = _constant_logits(row, B)
    got = run_act(x, ps, IDENT, 5, seed=seed, want_logits=False)
    cnt = torch.bincount(got.actions, minlength=5).double()
    exp = B * torch.softmax(torch.tensor(row, dtype=torch.float64), 0)
    chi2 = ((cnt - exp) ** 2 / exp).sum().item()
    log(f"act frequencies: counts {cnt.tolist()} chi2 {chi2:.3f}")
    assert chi2 < 33.4


# ------------------------------------------------------------------------------------------------------------ 3. the flat optimiser step
MAX_NORM, STEP_LR = 0.5, 3e-3
STEP_MODES = (("below", 0.5, MAX_NORM), ("at", 1.0, MAX_NORM), ("above", 100.0, MAX_NORM), ("noclip", 100.0, 0.0))


def step_case(n, t, scale, seed=0):
    """planted state of one step on the CPU: p, g, m, v float32 [n] with ||g||_2 = scale * MAX_NORM; step 1 starts from zero moments"""
    gen = torch.Generator().manual_seed(1000 * t + n + seed)
    p = 0.1 * torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    g = (g * (scale * MAX_NORM / g.double().norm().item())).float()
    m = torch.zeros(n) if t == 1 else 0.1 * g.abs().mean() * torch.randn(n, generator=gen)
    v = torch.zeros(n) if t == 1 else (g.abs().mean() ** 2) * (0.5 + torch.rand(n, generator=gen))
    return p, g, m, v


def run_flat_step(p, g, m, v, max_norm, lr, t):
    lib, L = _lib()
    n, pad = p.numel(), 8
    dev = []
    for src in (p, g, m, v):
        b = torch.full((n + pad,), 77.0, device="cuda")
        b[:n] = src.cuda()
        dev.append(b)
    nws = L.ocrl_flat_clip_adam_ws_floats()
    ws, norm = nanlike(nws), nanlike(1)
    rc = L.ocrl_flat_clip_adam_l2(*[lib.ptr(b) for b in dev], n, max_norm, lr, 0.9, 0.999, 1e-5, t, lib.ptr(norm), lib.ptr(ws), nws, lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ocrl_last_error().decode()
    for b in dev:
        assert (b[n:] == 77.0).all(), "the step wrote past the buffer's n floats"
    assert torch.equal(dev[1][:n].cpu(), g)
    return dev[0][:n].cpu(), dev[2][:n].cpu(), dev[3][:n].cpu(), norm.cpu()[0]


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("n", [1, 3, 1027, 70001])
def test_flat_clip_adam_step(n, t):
    """dp / lr against the fp64 step within 4 x STEP_DEV = 2.1e-5 (STEP_DEV = 5.2e-6: the fp32 torch step's own largest deviation over
    these cases, set by the rounding of p + dp at |p| < 0.5 and lr = 3e-3); the norm within 1e-6; two runs bit-identical"""
    for tag, scale, max_norm in STEP_MODES:
        p, g, m, v = step_case(n, t, scale)
        r = P.clip_adam_l2(p, g, m, v, max_norm, STEP_LR, t)
        p1, m1, v1, norm = run_flat_step(p, g, m, v, max_norm, STEP_LR, t)
        p2, m2, v2, norm2 = run_flat_step(p, g, m, v, max_norm, STEP_LR, t)
        assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(norm, norm2)
        e_n = abs(norm.item() - r.norm.item()) / r.norm.item()
        dev = ((p1.double() - p.double()) - (r.p - p.double())).abs().max().item() / STEP_LR
        moved = (p1 != p).double().mean().item()
        log(f"flat step n{n} t{t} {tag}: norm rel err {e_n:.2e}, dp/lr dev {dev:.2e}, coef {r.coef.item():.4f}, {moved:.2f} of p moved")
        assert e_n <= 1e-6 and dev <= 4 * STEP_DEV
        assert (r.coef.item() < 1.0) == (tag in ("at", "above")) and moved > 0.9
        assert err(m1, r.m) <= 1e-6 and err(v1, r.v) <= 1e-6


def test_flat_clip_adam_rejects_bad_arguments():
    lib, L = _lib()
    nws = L.ocrl_flat_clip_adam_ws_floats()
    b = [torch.zeros(8, device="cuda") for _ in range(4)]
    ws, norm = torch.zeros(nws, device="cuda"), nanlike(1)
    ptrs = [lib.ptr(t) for t in b]
    call = lambda ps, n, w, nw, nrm=norm: L.ocrl_flat_clip_adam_l2(*ps, n, 0.5, 1e-3, 0.9, 0.999, 1e-5, 1, lib.ptr(nrm), w, nw, lib.stream())
    assert call(ptrs, 0, lib.ptr(ws), nws) != 0 and call(ptrs, -4, lib.ptr(ws), nws) != 0
    for k in range(4):
        assert call(ptrs[:k] + [None] + ptrs[k + 1:], 8, lib.ptr(ws), nws) != 0
    assert call(ptrs, 8, None, nws) != 0 and call(ptrs, 8, lib.ptr(ws), nws, None) != 0
    assert call(ptrs, 8, lib.ptr(ws), nws - 1) != 0 and "workspace" in L.ocrl_last_error().decode()
    torch.cuda.synchronize()
    assert all((t == 0).all() for t in b) and torch.isnan(norm).all()


# ------------------------------------------------------------------------------------------------------------ 4. one train()
TRAIN_LR = 1e-3
TRAIN_HYPER = dict(batch_size=8, clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=True, max_grad_norm=0.5, learning_rate=TRAIN_LR)


def _space(shape=None, n=None):
    return types.SimpleNamespace(shape=shape, n=n)


def make_policy(F, A, seed):
    from ocrl_amd.sb3s import CustomActorCriticPolicy
    torch.manual_seed(seed)
    return CustomActorCriticPolicy(_space((F,)), _space(n=A), config=types.SimpleNamespace(sb3_acnet=_acnet_cfg("mlp")))


def abi_params(policy):
    return [p.detach().cpu().clone() for p in policy._head_args()[3]]


def train_case():
    """everything test 4 feeds train(), built on the CPU: the policy's initial parameters, a hand-filled rollout of T = 8, E = 4 and the
    two permutations.  Actions, values and log-probs are the fp64 restatement's under the initial parameters, rounded to fp32."""
    F, A, T, E = 12, 4, 8, 4
    pol = make_policy(F, A, 7)
    ps = abi_params(pol)
    gen = torch.Generator().manual_seed(51)
    feats = torch.randn(T, E, F, generator=gen)
    _, _, lg, vl = R.forward(feats.reshape(T * E, F).double(), [p.double() for p in ps], *MLP)
    actions = P.sample(lg, torch.rand(T * E, generator=gen))
    buf = dict(features=feats, actions=actions.reshape(T, E), values=vl.float().reshape(T, E), log_probs=P.log_prob(lg, actions).float().reshape(T, E),
               rewards=((torch.arange(T * E) * 7) % 5).float().reshape(T, E) / 4, episode_starts=torch.zeros(T, E))
    buf["episode_starts"][0] = 1.0
    buf["episode_starts"][5, ::2] = 1.0
    adv, ret = P.gae(buf["rewards"].double(), buf["values"].double(), buf["episode_starts"].double(), torch.zeros(E, dtype=torch.float64),
                     torch.ones(E, dtype=torch.float64), 0.99, 0.95)
    buf["advantages"], buf["returns"] = adv.float(), ret.float()
    perms = [torch.randperm(T * E, generator=gen) for _ in range(2)]
    return pol, ps, buf, perms


def make_ppo(pol, buf, **over):
    from ocrl_amd.sb3s import PPO, RolloutBuffer
    T, E, F = buf["features"].shape
    env = types.SimpleNamespace(num_envs=E, observation_space=_space((F,)), action_space=_space(n=4))
    kw = dict(n_steps=T, n_epochs=2, seed=3, device="cuda", gamma=0.99, gae_lambda=0.95)
    kw.update(TRAIN_HYPER)
    kw.update(over)
    ppo = PPO(pol, env, **kw)
    rb = RolloutBuffer(T, E, (F,), ppo.device, 0.99, 0.95)
    for t in range(T):
        rb.add(buf["features"][t], buf["actions"][t], buf["rewards"][t], buf["episode_starts"][t], buf["values"][t], buf["log_probs"][t])
    rb.advantages.copy_(buf["advantages"])
    rb.returns.copy_(buf["returns"])
    ppo.rollout_buffer = rb
    return ppo


def test_train_against_the_restatement():
    """parameters after the eight updates (2 epochs x 4 minibatches of 8) as dp / lr against the fp64 restatement within 4 x TRAIN_DEV =
    2.2e-4 (TRAIN_DEV = 5.4e-5: the fp32 torch restatement's own largest deviation on these inputs); the means of the six scalars within
    1e-4"""
    pol, ps, buf, perms = train_case()
    keys = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    ppo = make_ppo(pol, buf)
    assert {k: tuple(v.shape) for k, v in ppo.policy.state_dict().items()} == keys
    assert all(p.data_ptr() >= ppo.flat_p.data_ptr() and p.data_ptr() < ppo.flat_p.data_ptr() + 4 * ppo.flat_p.numel() for p in ppo.policy.parameters())
    stats = ppo.train(perms)
    want_p, want_s, n = P.train(ps, MLP, buf, perms, TRAIN_HYPER)
    assert stats["n_updates"] == n == 8 and ppo.adam_step == 8
    got_p = abi_params(ppo.policy)
    worst = 0.0
    for i, (g, w, p0) in enumerate(zip(got_p, want_p, ps)):
        dev = ((g.double() - p0.double()) - (w - p0.double())).abs().max().item() / TRAIN_LR
        worst = max(worst, dev)
        assert (g != p0).any(), i
    log(f"train: worst dp/lr deviation {worst:.2e} (bound {4 * TRAIN_DEV:.2e})")
    assert worst <= 4 * TRAIN_DEV
    smax = want_s[:5].abs().max().item()
    for i, k in enumerate(R.SCALARS):
        e = abs(stats[k] - want_s[i].item()) / max(abs(want_s[i].item()), 1e-3 * smax, 1e-30)
        log(f"train {k}: got {stats[k]:.6f} want {want_s[i].item():.6f} rel err {e:.2e}")
        assert e <= 1e-4, (k, e)
    y, v = buf["returns"].double().reshape(-1), buf["values"].double().reshape(-1)
    assert abs(stats["explained_variance"] - (1 - (y - v).var(unbiased=False) / y.var(unbiased=False)).item()) <= 1e-4
    assert 0 < stats["grad_norm"] < 100


def test_train_edges_zero_rate_target_kl_and_checkpoint(tmp_path):
    pol, ps, buf, perms = train_case()
    ppo = make_ppo(pol, buf, learning_rate=0.0)
    ppo.train(perms)
    assert all(torch.equal(a, b) for a, b in zip(abi_params(ppo.policy), ps)) and ppo.adam_step == 8
    pol, ps, buf, perms = train_case()
    ppo = make_ppo(pol, buf, target_kl=1e-9)
    # actions and log-probs as the rollout records them (the policy's own launch): the first minibatch then sees ratio = 1 and approx_kl = 0
    # and takes its step; after it the policy has moved by lr = 1e-3 per weight, approx_kl is of the order of 1e-5 and the second one trips
    rb = ppo.rollout_buffer
    a, _, lp = ppo.policy.act(rb.observations.reshape(-1, 12), uniforms=torch.rand(32, generator=torch.Generator().manual_seed(52)))
    rb.actions.copy_(a.view(8, 4))
    rb.log_probs.copy_(lp.view(8, 4))
    stats = ppo.train(perms)
    assert stats["n_updates"] == 1 and ppo.adam_step == 1 and stats["approx_kl"] > 1.5e-9 / 2
    path = str(tmp_path / "ppo.pt")
    ppo.save(path)
    fresh = make_ppo(make_policy(12, 4, 99), buf, target_kl=1e-9)
    assert not torch.equal(fresh.flat_p, ppo.flat_p)
    fresh.load(path)
    assert torch.equal(fresh.flat_p, ppo.flat_p) and torch.equal(fresh.flat_m, ppo.flat_m) and torch.equal(fresh.flat_v, ppo.flat_v)
    assert fresh.adam_step == 1 and all(torch.equal(a, b) for a, b in zip(fresh.policy.state_dict().values(), ppo.policy.state_dict().values()))
    assert all(p.data_ptr() >= fresh.flat_p.data_ptr() and p.data_ptr() < fresh.flat_p.data_ptr() + 4 * fresh.flat_p.numel() for p in fresh.policy.parameters())


# ------------------------------------------------------------------------------------------------------------ 5. rollouts
class ScriptedEnv:
    """E = 3 environments, observations from a fixed table indexed by (env, global step), reward 1 for action == step mod A, episodes of 5
    steps; every second episode of an environment ends by its time limit (TimeLimit.truncated with the terminal observation)"""
    E, F, A, LEN, STEPS = 3, 12, 4, 5, 40

    def __init__(self):
        gen = torch.Generator().manual_seed(61)
        self.table = torch.randn(self.STEPS + 1, self.E, self.F, generator=gen)
        self.terminal = torch.randn(self.STEPS + 1, self.E, self.F, generator=gen)
        self.num_envs, self.observation_space, self.action_space = self.E, _space((self.F,)), _space(n=self.A)
        self.k = 0

    def reset(self):
        self.k = 0
        return self.table[0].numpy()

    def truncated(self, k, e):
        return (k + 1) % self.LEN == 0 and ((k // self.LEN) + e) % 2 == 1

    def step(self, actions):
        k = self.k
        actions = np.asarray(actions)
        assert actions.shape == (self.E,)
        rewards = (actions == k % self.A).astype(np.float32)
        done = (k + 1) % self.LEN == 0
        infos = [dict() for _ in range(self.E)]
        if done:
            for e in range(self.E):
                infos[e] = {"terminal_observation": self.terminal[k, e].numpy(), "TimeLimit.truncated": self.truncated(k, e)}
        self.k += 1
        return self.table[self.k].numpy(), rewards, np.full(self.E, done), infos


def scripted_ppo(seed, **over):
    from ocrl_amd.sb3s import PPO, CustomActorCriticPolicy
    kw = dict(n_steps=12, batch_size=8, n_epochs=1, seed=seed, learning_rate=1e-3, ent_coef=0.01,
              policy_kwargs=dict(config=types.SimpleNamespace(sb3_acnet=_acnet_cfg("mlp"))))
    kw.update(over)
    return PPO(CustomActorCriticPolicy, ScriptedEnv(), **kw)


def test_collect_rollouts_on_the_scripted_environment():
    T, seed = 12, 5
    ppo = scripted_ppo(seed)
    env, E = ppo.env, ScriptedEnv.E
    ps = [p.double() for p in abi_params(ppo.policy)]
    buf = ppo.collect_rollouts()
    assert ppo.num_timesteps == T * E and ppo.policy._sample_rows == T * E
    fwd = lambda obs: R.forward(obs.double(), ps, *MLP)
    want_starts = torch.zeros(T, E)
    for t in range(T):
        _, _, lg, vl = fwd(env.table[t])
        u = dump_uniforms(seed, t * E, E)
        actions = P.sample(lg, u)
        assert torch.equal(buf.actions[t].cpu(), actions), t
        assert torch.equal(buf.observations[t].cpu(), env.table[t])
        assert err(buf.values[t], vl) <= OUT_TOL and err(buf.log_probs[t], P.log_prob(lg, actions), 1e-3) <= OUT_TOL
        rew = (actions == t % env.A).double()
        for e in range(E):
            if env.truncated(t, e):
                rew[e] += 0.99 * fwd(env.terminal[t, e][None])[3][0]
        assert (buf.rewards[t].cpu().double() - rew).abs().max().item() <= 1e-5, t
        want_starts[t] = 1.0 if t % env.LEN == 0 else 0.0
    assert torch.equal(buf.episode_starts.cpu(), want_starts)
    assert sum(env.truncated(t, e) for t in range(T) for e in range(E)) == 3            # both kinds of episode end are in the rollout
    last = fwd(env.table[T])[3]
    adv, ret = P.gae(buf.rewards.cpu().double(), buf.values.cpu().double(), want_starts.double(), last, torch.zeros(E, dtype=torch.float64), 0.99, 0.95)
    assert err(buf.advantages, adv) <= 1e-4 and err(buf.returns, ret) <= 1e-4
    assert len(ppo._episodes) == 2 * E and ppo.ep_len_mean == env.LEN
    host = sum(float((buf.actions[t].cpu() == t % env.A).sum()) for t in range(10)) / (2 * E)
    assert abs(ppo.ep_rew_mean - host) <= 1e-9
    twin, other = scripted_ppo(seed), scripted_ppo(seed + 1)
    b2, b3 = twin.collect_rollouts(), other.collect_rollouts()
    for k in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
        assert torch.equal(getattr(buf, k), getattr(b2, k)), k
    assert not torch.equal(buf.log_probs, b3.log_probs)


# ------------------------------------------------------------------------------------------------------------ 6. end to end
def test_learn_runs_two_iterations_reproducibly():
    """not a learning claim: two iterations of rollouts and updates run, count their steps and end bit-identical for one seed.  The same
    run behind a frozen SLATE OCRExtractor is not part of this file (not run)."""
    def run():
        ppo, calls = scripted_ppo(9, n_steps=16), []
        assert ppo.learn(96, callback=lambda loc: calls.append((loc["iteration"], loc["num_timesteps"], loc["ep_rew_mean"]))) is ppo
        return ppo, calls
    ppo, calls = run()
    assert [c[:2] for c in calls] == [(1, 48), (2, 96)] and ppo.num_timesteps == 96 and ppo.adam_step == 12
    assert torch.isfinite(ppo.flat_p).all() and torch.isfinite(ppo.flat_m).all() and torch.isfinite(ppo.flat_v).all()
    log(f"learn: ep_rew_mean after the two iterations {calls[0][2]:.3f}, {calls[1][2]:.3f}")
    again, calls2 = run()
    assert torch.equal(again.flat_p, ppo.flat_p) and torch.equal(again.flat_v, ppo.flat_v) and calls2 == calls
    actions, state = ppo.predict(ppo.env.table[0], deterministic=True)
    assert state is None and actions.shape == (3,) and actions.dtype == np.int64
