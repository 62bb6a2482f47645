"""GPU checks of DQN's Munchausen targets: ``ocrl_munchausen_targets`` (include/ocrl_hip_munchausen.h) through the C ABI, its outputs
through the unchanged TD kernels, ``DQN(munchausen=True)`` on the scalar, quantile and implicit quantile heads, checkpoints and
``train_sb3.build``, against the fp64 restatement of tests/munchausen_ref.py.

Bounds.  Every output of the kernel, absolute: (16 + A) * 2^-24 * max(1, the largest finite |input| of the case).  pi carries a few ulp
of the total mass (|s| e^s <= 1 / e bounds what the rounding of s does to it), logpi a few ulp of |x - v|, and a serial sum of A terms
adds A / 2 ulp; a missing tau * logpi term would be off by about 0.04.  The facts the header calls bit for bit are compared as bits.
Through the TD kernels the bounds are those tests/test_gpu_replay_ext.py, tests/test_gpu_qr.py and tests/test_gpu_iqn.py state for these
kernels: scalars 1e-4 relative with a floor of 1e-3 of the largest, |delta| 1e-4 of its maximum, gradients and row_loss 3e-4 of their
tensor's maximum with a floor of 1e-3 of the largest gradient.  ``train_step()`` is graded on dp / lr, elementwise, against the fp64
restatement fed the batches, fractions and noise factors the run drew; the bound is the one of
test_gpu_c51.py::test_three_updates_against_the_restatement: 4 x the largest deviation of the fp32 torch restatement from the fp64 one on
the very inputs of the test, measured by the test itself on the CPU."""
import ctypes
import functools
import math
import os

import pytest
import torch

from tests import dqn_ref as R
from tests import iqn_ref as I
from tests import munchausen_ref as M
from tests import qr_ref as Q
from tests import replay_ext_ref as X
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
# (B, A, N'): the smallest, without and with quantile values; small and odd; N' = 16; several rows; the limit of A; the limit of N';
# more rows than a hundred; no quantile values at an odd A
SHAPES = [(1, 1, 0), (1, 1, 1), (5, 2, 3), (3, 3, 16), (37, 4, 8), (20, 64, 4), (3, 4, 64), (130, 4, 8), (257, 5, 0)]
TAUS = [0.03, 1.0]
ALPHA, CLIP = 0.9, -1.0
GAMMA, KAPPA = 0.9, 1.0
f64 = torch.float64


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


# ------------------------------------------------------------------------------------------------------------ 1. the kernel against fp64
@functools.lru_cache(maxsize=None)
def case(B, A, Np):
    """the inputs of a case on the CPU, built once: randn * 2; row 2 all-equal; row 3 with one entry + 40 (its other actions' exp
    underflows at tau = 0.03); every third row done with next_q = inf and next_quantiles = NaN there; two actions outside [0, A)"""
    gen = torch.Generator().manual_seed(97 + B + 3 * A + Np)
    cur, nxt = torch.randn(B, A, generator=gen) * 2, torch.randn(B, A, generator=gen) * 2
    quant = torch.randn(B, A, Np, generator=gen) * 2 if Np else None
    actions = torch.randint(0, A, (B,), generator=gen)
    rewards = torch.randn(B, generator=gen) * 2
    dones = (torch.arange(B) % 3 == 1).to(torch.uint8)
    if B > 3:
        cur[2], nxt[2] = cur[2, 0].item(), nxt[2, 0].item()
        cur[3, A // 2] += 40.0
        nxt[3, A - 1] += 40.0
        actions[3] = 0                                                         # with A > 1 not the raised entry: the bonus is the whole clip
    nxt[dones.bool()] = float("inf")
    if Np:
        quant[dones.bool()] = float("nan")
    largest = max(t[torch.isfinite(t)].abs().max().item() for t in (cur, nxt, rewards) + ((quant,) if Np else ()) if torch.isfinite(t).any())
    if B > 1:
        actions[0], actions[-1] = -3, A + 5
    return dict(cur=cur, nxt=nxt, quant=quant, actions=actions, rewards=rewards, dones=dones, largest=largest)


@functools.lru_cache(maxsize=None)
def truth(B, A, Np, tau):
    c = case(B, A, Np)
    return M.targets(c["cur"].double(), c["nxt"].double(), c["actions"], c["rewards"].double(), c["dones"], ALPHA, tau, CLIP,
                     None if c["quant"] is None else c["quant"].double())


def run(c, tau, alpha=ALPHA, clip=CLIP, rows=None):
    """ocrl_munchausen_targets on a case (or on its rows ``rows``), the outputs pre-filled with NaN"""
    lib, L = _lib()
    sel = lambda t: None if t is None else (t if rows is None else t[rows]).cuda().contiguous()
    cur, nxt, quant, actions, rewards, dones = (sel(c[k]) for k in ("cur", "nxt", "quant", "actions", "rewards", "dones"))
    B, A = cur.shape
    Np = 0 if quant is None else quant.shape[2]
    ro, nv, nm = nanlike(B), nanlike(B, A), nanlike(B, A, Np) if Np else None
    lib.check(L.ocrl_munchausen_targets(lib.ptr(cur), lib.ptr(nxt), lib.ptr(quant), Np, lib.ptr(actions.long()), lib.ptr(rewards), lib.ptr(dones), B, A,
                                        alpha, tau, clip, lib.ptr(ro), lib.ptr(nv), lib.ptr(nm), lib.stream()))
    torch.cuda.synchronize()
    return ro, nv, nm


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("B, A, Np", SHAPES, ids=lambda v: str(v))
def test_targets_against_fp64(B, A, Np, tau):
    c = case(B, A, Np)
    want = truth(B, A, Np, tau)
    assert all(torch.isfinite(w).all() for w in want if w is not None)
    got = run(c, tau)
    bound = (16 + A) * 2.0 ** -24 * max(1.0, c["largest"])
    worst = 0.0
    for name, g, w in zip(("rewards_out", "next_v", "next_m"), got, want):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape and torch.isfinite(g).all(), (name, "an element the kernel did not write, or a NaN")
        e = (g.cpu().double() - w).abs().max().item()
        worst = max(worst, e / bound)
        log(f"munchausen B{B} A{A} N'{Np} tau {tau} {name}: worst abs err {e:.3e}, bound {bound:.3e} ({e / bound:.3f} of it)")
        assert e <= bound, (name, e, bound)
    log(f"munchausen B{B} A{A} N'{Np} tau {tau}: worst ratio to the bound {worst:.3f}")
    done = c["dones"].bool()
    assert (got[1].cpu()[done] == 0).all() and (Np == 0 or (got[2].cpu()[done] == 0).all())
    if B > 3 and A > 1:
        assert got[0][3].item() == (c["rewards"][3] + torch.tensor(ALPHA * CLIP)).item()          # far below the maximum: the whole clip, exactly
    again = run(c, tau)
    assert all(a is None and b is None or torch.equal(bits(a), bits(b)) for a, b in zip(again, got))


# ------------------------------------------------------------------------------------------------------------ 2. the facts that hold bit for bit
@pytest.mark.parametrize("tau", TAUS)
def test_one_action_changes_nothing(tau):
    gen = torch.Generator().manual_seed(3)
    B, Np = 9, 5
    c = dict(cur=torch.randn(B, 1, generator=gen) * 2, nxt=torch.randn(B, 1, generator=gen) * 2, quant=torch.randn(B, 1, Np, generator=gen) * 2,
             actions=torch.randint(-2, 3, (B,), generator=gen), rewards=torch.randn(B, generator=gen), dones=(torch.arange(B) % 3 == 1).to(torch.uint8))
    ro, nv, nm = run(c, tau)
    keep = ~c["dones"].bool()
    assert torch.equal(ro.cpu(), c["rewards"]) and torch.equal(nv.cpu()[keep], c["nxt"][keep]) and torch.equal(nm.cpu()[keep], c["quant"][keep])
    assert (nv.cpu()[~keep] == 0).all() and (nm.cpu()[~keep] == 0).all()


@pytest.mark.parametrize("tau", TAUS)
def test_alpha_zero_leaves_the_rewards(tau):
    for shape in ((37, 4, 8), (257, 5, 0)):
        c = case(*shape)
        ro, nv, nm = run(c, tau, alpha=0.0)
        assert torch.equal(ro.cpu(), c["rewards"])
        full = run(c, tau)
        assert torch.equal(bits(nv), bits(full[1])) and (nm is None or torch.equal(bits(nm), bits(full[2])))     # alpha touches the rewards alone
        assert not torch.equal(full[0].cpu(), c["rewards"])


@pytest.mark.parametrize("tau", TAUS)
def test_a_row_does_not_depend_on_its_position_or_on_the_batch(tau):
    c = case(130, 4, 8)
    full = run(c, tau)
    for rows in (slice(5, 20), slice(64, 130), torch.tensor([129, 3, 2, 77, 1])):
        part = run(c, tau, rows=rows)
        assert all(torch.equal(bits(p), bits(f[rows])) for p, f in zip(part, full))


@pytest.mark.parametrize("B, A, Np", [(37, 4, 8), (20, 64, 4), (3, 4, 64)], ids=lambda v: str(v))
def test_the_columns_are_a_broadcast(B, A, Np):
    for tau in TAUS:
        _, nv, nm = run(case(B, A, Np), tau)
        assert torch.equal(bits(nv), bits(nv[:, :1].expand(B, A))) and torch.equal(bits(nm), bits(nm[:, :1].expand(B, A, Np)))


# ------------------------------------------------------------------------------------------------------------ 3. through the unchanged TD kernels
TD_B, TD_F, TD_A, TD_N, TD_NP, TD_C = 5, 8, 3, 5, 3, 8
TD_LAYOUT = ((64, 64), (1, 1))                                                   # test_gpu_qr.py's "mlp"
TD_TAU = 0.03


@functools.lru_cache(maxsize=None)
def td_inputs(Np):
    """what the three heads share: features, the target network's values (Np quantile values per action), the transition, per-row
    discounts and weights; row 1 done with non-finite next inputs, row 4 done too, two actions outside [0, A).  The action values lie
    within a few tau of each other, so the policy is soft and the targets are far from the plain ones"""
    gen = torch.Generator().manual_seed(41 + Np)
    B, F, A = TD_B, TD_F, TD_A
    c = dict(x=torch.randn(B, F, generator=gen), cur=torch.randn(B, A, generator=gen) * 0.05, nxt=torch.randn(B, A, generator=gen) * 0.05,
             quant=torch.randn(B, A, Np, generator=gen) * 2 if Np else None, actions=torch.tensor([-3, 1, 2, 0, A + 5]),
             rewards=torch.randn(B, generator=gen) * 1.5, dones=torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8))
    c["nxt"][1] = float("inf")
    if Np:
        c["quant"][1] = float("nan")
    c["discounts"] = GAMMA ** torch.randint(1, 4, (B,), generator=gen).float()
    c["weights"] = torch.rand(B, generator=gen) * 0.9 + 0.1
    return c


def gpu_targets(c):
    """(rewards_m, next_v, next_m) of the kernel on td_inputs, on the device, and the fp64 ones of the restatement"""
    got = run(c, TD_TAU)
    want = M.targets(c["cur"].double(), c["nxt"].double(), c["actions"], c["rewards"].double(), c["dones"], ALPHA, TD_TAU, CLIP,
                     None if c["quant"] is None else c["quant"].double())
    live = ~c["dones"].bool()
    assert (want[0] - c["rewards"].double()).abs().min() > 5e-4                                                   # the targets did change
    assert (want[1][live, 0] - c["nxt"][live].double().max(dim=1).values).min() > 5e-4
    return got, want


def check_td(tag, got, scal, dx, dw, row, row_bound):
    smax = scal.abs().max().item()
    for i, k in enumerate(("loss", "mean_q", "mean_target")):
        e = abs(got["scal"][i].item() - scal[i].item()) / max(abs(scal[i].item()), 1e-3 * smax, 1e-30)
        log(f"munchausen -> {tag} {k}: got {got['scal'][i].item():.6f} want {scal[i].item():.6f} rel err {e:.2e} (bound 1e-4)")
        assert e <= 1e-4, (tag, k, e)
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    worst = max(err(g, w, 1e-3 * gmax) for g, w in zip([got["dx"]] + got["dw"], [dx] + dw))
    er = err(got["row"], row, *row_bound[1:])
    log(f"munchausen -> {tag}: worst gradient {worst:.2e} (bound 3e-4), rows' errors {er:.2e} (bound {row_bound[0]:.0e})")
    assert worst <= 3e-4 and er <= row_bound[0], (tag, worst, er)


def test_through_the_scalar_td_step():
    lib, L = _lib()
    c = td_inputs(0)
    B, F, A = TD_B, TD_F, TD_A
    ps = R.make_params(F, A, TD_LAYOUT[0], 71)
    (rm, nv, _), (rm64, nv64, _) = gpu_targets(c)
    scal, dx, dw, ad = X.td_step_ext(c["x"], ps, TD_LAYOUT[1], nv64, c["actions"], rm64, c["dones"], GAMMA, None, c["discounts"], c["weights"])
    d = lib.qnet_desc(B, F, A, *TD_LAYOUT)
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = c["x"].cuda(), [p.cuda() for p in ps]
    ac, dn, dc, wt = c["actions"].cuda().long(), c["dones"].cuda(), c["discounts"].cuda(), c["weights"].cuda()
    out = dict(scal=nanlike(3), dw=[nanlike(*p.shape) for p in ps], dx=nanlike(B, F), row=nanlike(B))
    ws = nanlike(n)
    lib.check(L.ocrl_dqn_td_fwd_bwd_ext(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(nv), None, lib.ptr(ac), lib.ptr(rm),
                                        lib.ptr(dn), lib.ptr(dc), lib.ptr(wt), GAMMA, lib.ptr(out["scal"]),
                                        lib.ptr(out["row"]), lib.ptr(out["dx"]), lib.ptrs(out["dw"]), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    check_td("ocrl_dqn_td_fwd_bwd_ext", out, scal, dx, dw, ad, (1e-4,))


def test_through_the_quantile_td_step():
    lib, L = _lib()
    c = td_inputs(TD_N)
    B, F, A, N = TD_B, TD_F, TD_A, TD_N
    ps = Q.make_params(F, A, N, TD_LAYOUT[0], False, 79)
    (rm, nv, nm), (rm64, nv64, nm64) = gpu_targets(c)
    scal, dx, dw, ql = Q.qr_step(c["x"], ps, TD_LAYOUT[1], A, N, False, nm64, nv64, c["actions"], rm64, c["dones"], GAMMA, KAPPA, c["discounts"], c["weights"])
    d = lib.qr_desc(B, F, A, N, *TD_LAYOUT, False)
    n = L.ocrl_qr_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = c["x"].cuda(), [p.cuda() for p in ps]
    ac, dn, dc, wt = c["actions"].cuda().long(), c["dones"].cuda(), c["discounts"].cuda(), c["weights"].cuda()
    out = dict(scal=nanlike(3), dw=[nanlike(*p.shape) for p in ps], dx=nanlike(B, F), row=nanlike(B))
    ws = nanlike(n)
    lib.check(L.ocrl_qr_td_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(nm), lib.ptr(nv), lib.ptr(ac), lib.ptr(rm),
                                   lib.ptr(dn), lib.ptr(dc), lib.ptr(wt), GAMMA, KAPPA, lib.ptr(out["scal"]),
                                   lib.ptr(out["row"]), lib.ptr(out["dx"]), lib.ptrs(out["dw"]), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    check_td("ocrl_qr_td_fwd_bwd", out, scal, dx, dw, ql, (3e-4, 1e-3 * gmax))


def test_through_the_implicit_quantile_td_step():
    lib, L = _lib()
    c = td_inputs(TD_NP)
    B, F, A, N, Np, C = TD_B, TD_F, TD_A, TD_N, TD_NP, TD_C
    ps = I.make_params(F, A, C, TD_LAYOUT[0], 83)
    taus = torch.randint(0, 2 ** 24, (B, N), generator=torch.Generator().manual_seed(9)).float() / 2 ** 24
    (rm, nv, nm), (rm64, nv64, nm64) = gpu_targets(c)
    scal, dx, dw, ql = I.iqn_step(c["x"], taus, ps, TD_LAYOUT[1], A, C, nm64, nv64, c["actions"], rm64, c["dones"], GAMMA, KAPPA, c["discounts"], c["weights"])
    d = lib.iqn_desc(B, F, A, N, C, *TD_LAYOUT)
    n = L.ocrl_iqn_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, ts, pd = c["x"].cuda(), taus.cuda(), [p.cuda() for p in ps]
    ac, dn, dc, wt = c["actions"].cuda().long(), c["dones"].cuda(), c["discounts"].cuda(), c["weights"].cuda()
    out = dict(scal=nanlike(3), dw=[nanlike(*p.shape) for p in ps], dx=nanlike(B, F), row=nanlike(B))
    ws = nanlike(n)
    lib.check(L.ocrl_iqn_td_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptr(ts), lib.ptrs(pd), lib.ptr(nm), Np, lib.ptr(nv), lib.ptr(ac),
                                    lib.ptr(rm), lib.ptr(dn), lib.ptr(dc), lib.ptr(wt), GAMMA, KAPPA,
                                    lib.ptr(out["scal"]), lib.ptr(out["row"]), lib.ptr(out["dx"]), lib.ptrs(out["dw"]), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    check_td("ocrl_iqn_td_fwd_bwd", out, scal, dx, dw, ql, (3e-4, 1e-3 * gmax))


def test_the_function_returns_fresh_constants():
    from ocrl_amd import sb3s
    c = case(37, 4, 8)
    dev = lambda t: t.cuda()
    cur = dev(c["cur"]).requires_grad_(True)
    ro, nv, nm = sb3s.munchausen_targets(cur, dev(c["nxt"]), dev(c["actions"]), dev(c["rewards"]), dev(c["dones"]), ALPHA, 0.03, CLIP,
                                         next_quantiles=dev(c["quant"]))
    want = run(c, 0.03)
    assert all(torch.equal(bits(a), bits(b)) and not a.requires_grad for a, b in zip((ro, nv, nm), want))
    ro2, nv2, none = sb3s.munchausen_targets(cur, dev(c["nxt"]), dev(c["actions"]), dev(c["rewards"]), dev(c["dones"]), ALPHA, 0.03, CLIP)
    assert none is None and torch.equal(bits(ro2), bits(ro)) and torch.equal(bits(nv2), bits(nv)) and ro2.data_ptr() != ro.data_ptr()
    for kw, name in ((dict(alpha=1.5), "alpha"), (dict(tau=0.0), "tau"), (dict(clip_lo=0.5), "clip_lo")):
        args = dict(dict(alpha=ALPHA, tau=0.03, clip_lo=CLIP), **kw)
        with pytest.raises(ValueError, match=name):
            sb3s.munchausen_targets(cur, dev(c["nxt"]), dev(c["actions"]), dev(c["rewards"]), dev(c["dones"]), **args)
    with pytest.raises(ValueError, match="next_quantiles is"):
        sb3s.munchausen_targets(cur, dev(c["nxt"]), dev(c["actions"]), dev(c["rewards"]), dev(c["dones"]), ALPHA, 0.03, CLIP, next_quantiles=dev(c["quant"])[:, :2])


# ------------------------------------------------------------------------------------------------------------ 4. three updates, 5. the loop
LOOP = ["sb3.algo_kwargs.buffer_size=64", "sb3.algo_kwargs.learning_starts=16", "sb3.algo_kwargs.train_freq=4", "sb3.algo_kwargs.target_update_interval=8",
        "sb3.algo_kwargs.batch_size=8", "+sb3.algo_kwargs.log_interval=1", "sb3.algo_kwargs.learning_rate=1e-3", "env.max_steps=6"]
UPDATES, BS, NQ = 3, 8, 8
MUN_ON = ["+sb3.algo_kwargs.munchausen=True", "+sb3.algo_kwargs.munchausen_alpha=0.9", "+sb3.algo_kwargs.munchausen_tau=0.03",
          "+sb3.algo_kwargs.munchausen_clip=-1.0"]
# the scalar head as mdqn.yaml has it; the quantile head with dueling, 3-step returns and prioritized replay; the implicit quantile
# head as miqn.yaml has it (3-step returns, prioritized replay, noisy layers) at N' = 5
HEADS = {"scalar": ("mdqn", []),
         "quantile": ("qrdqn", [f"sb3.algo_kwargs.n_quantiles={NQ}", "sb3.algo_kwargs.noisy=False", "sb3.algo_kwargs.double_q=False"] + MUN_ON),
         "implicit": ("miqn", ["sb3.algo_kwargs.n_tau_prime_samples=5"])}


def build_loop(sb3, *over):
    import train_sb3
    from ocrl_amd.utils.config import compose
    c = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0",
                                   "env.rew_type=dense"] + LOOP + list(over))
    return train_sb3.build(c)[2]


@pytest.mark.parametrize("head", list(HEADS))
def test_three_updates_against_the_restatement(head):
    """DQN(munchausen=True) on four Target environments, one run per head: three train_step() calls against the restatement fed the
    batches, the fractions and the noise factors the run drew"""
    from ocrl_amd import sb3s
    from ocrl_amd.sb3s.iqn import TRAIN_SEED_SALT, draw_taus
    from ocrl_amd.sb3s.noisy import draw_factors
    model = build_loop(HEADS[head][0], *HEADS[head][1])
    want = {"scalar": (sb3s.QNetwork, False, 1, False, False), "quantile": (sb3s.QuantileQNetwork, True, 3, True, False),
            "implicit": (sb3s.ImplicitQuantileQNetwork, False, 3, True, True)}[head]
    assert type(model.policy.q_net) is want[0] and type(model.target.q_net) is want[0]
    assert (model.dueling, model.n_step, model.prioritized_replay, model.noisy, model.double_q, model.munchausen) == (*want[1:], False, True)
    mun = (model.munchausen_alpha, model.munchausen_tau, model.munchausen_clip)
    assert mun == (0.9, 0.03, -1.0)
    n_step, per, noisy = want[2:]
    N, Np = model.n_tau_samples, model.n_tau_prime_samples
    for _ in range(8):
        model.collect_step()
    buf = model.replay_buffer
    assert buf.pos == 8 and torch.equal(model.flat_target, model.flat_p) and model.noise_draws == (8 if noisy else 0)
    ps0 = [p.detach().cpu().clone() for p in model.policy.parameters() if p.requires_grad]
    n_plain = sum(1 for _ in model.policy.features_extractor._pooling.parameters())
    net = model.policy.q_net
    head_acts = net._layout()[1]
    if head == "quantile":
        layers = [(m.in_features, m.out_features) for m in list(net.q_net) + [net.value_net] if isinstance(m, torch.nn.Linear)]
    else:
        layers = [(m.in_features, m.out_features) for m in net.q_net if isinstance(m, torch.nn.Linear)]
    acts = (1,) * (n_plain // 2) + tuple(head_acts)
    lr = model.learning_rate
    rows_before = model.policy._sample_rows
    batches, taus, facs = [], [], []
    for u in range(UPDATES):
        if per:
            idx, w = buf.sample_prioritized(BS, model.n_updates, model.beta())               # what train_step is about to draw: a pure function
        else:
            idx, w = buf.sample_indices(BS, model.n_updates, n_step), None
        b = buf.gather(idx, n_step, model.gamma) if n_step > 1 else buf.gather(idx)
        batches.append(tuple(None if t is None else t.cpu() for t in (model._obs(b.observations), model._obs(b.next_observations), b.actions, b.rewards,
                                                                      b.dones, b.discounts, w)))
        if head == "implicit":                                                               # the fractions, as the GPU writes them
            seed = model.seed + TRAIN_SEED_SALT
            taus.append(tuple(draw_taus(seed, (3 * model.n_updates + k) * BS, BS, n, model.device).cpu() for k, n in ((0, N), (1, Np), (2, Np))))
        if noisy:                                                                            # the step's two draws, as the GPU writes them
            facs.append((draw_factors(layers, model.seed, model.noise_draws, model.device)[1].cpu(),
                         draw_factors(layers, model.seed + 1, model.noise_draws + 1, model.device)[1].cpu()))
        model.train_step()
        if per:
            assert torch.equal(model.last_weights, w)
    assert model.n_updates == UPDATES and all(torch.equal(t.cpu(), p0) for t, p0 in zip(model.target.parameters(), ps0))      # the target stood still
    assert model.noise_draws == (8 + 2 * UPDATES if noisy else 0) and model.policy._sample_rows == rows_before                 # two draws an update, no acting row

    def split(ps, fac=None):                                                                 # the implicit head: the embedding is the last module
        chain = list(ps[:-2]) if fac is None else Q.noisy_chain(list(ps[:-2]), n_plain, layers, fac)
        return chain[:n_plain], list(ps[-2:]) + chain[n_plain:]

    def ref(dtype):
        cur, m, v = [p.to(dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0], [torch.zeros_like(p, dtype=dtype) for p in ps0]
        out = []
        for step, batch in enumerate(batches, 1):
            fo, ft = facs[step - 1] if noisy else (None, None)
            if head == "scalar":
                cur, m, v, scal, _ = M.dqn_train_step(cur, ps0, m, v, step, batch, acts, mun, model.gamma, lr, model.max_grad_norm, dtype)
            elif head == "quantile":
                cur, m, v, scal, _ = M.qr_train_step(cur, ps0, m, v, step, batch, acts, 4, NQ, True, mun, model.gamma, model.huber_kappa, lr,
                                                     model.max_grad_norm, dtype)
            else:
                cur, m, v, scal, _ = M.iqn_train_step(cur, ps0, m, v, step, batch, taus[step - 1], head_acts, 4, model.n_cos, mun, model.gamma,
                                                      model.huber_kappa, lr, model.max_grad_norm, lambda ps, f=fo: split(ps, f),
                                                      lambda ps, f=ft: split(ps, f), dtype)
            out.append(scal)
        return cur, out
    p64, out64 = ref(torch.float64)
    p32, _ = ref(torch.float32)
    dev = max(((a.double() - p0.double()) - (w - p0.double())).abs().max().item() for a, w, p0 in zip(p32, p64, ps0)) / lr
    bound = 4 * dev
    got = [p.detach().cpu() for p in model.policy.parameters() if p.requires_grad]
    worst = max(((g.double() - p0.double()) - (w - p0.double())).abs().max().item() for g, w, p0 in zip(got, p64, ps0)) / lr
    log(f"munchausen train_step {head}: worst dp/lr deviation {worst:.2e}; the fp32 restatement's {dev:.2e} (bound 4 x that: {bound:.2e}, "
        f"{worst / bound:.2f} of it)")
    assert all((g != p0).any() for g, p0 in zip(got, ps0)) and worst <= bound
    st = model.train_stats()
    for i, k in enumerate(("loss", "mean_q", "mean_target")):
        mean = sum(s[i].item() for s in out64) / UPDATES
        assert abs(st[k] - mean) <= 1e-4 * max(abs(mean), 1e-3 * max(s.abs().max().item() for s in out64)), (k, st[k], mean)


def test_munchausen_off_never_takes_the_new_launch():
    """munchausen=False is the step as it was: the same parameters as a run that has never heard of the arguments, and no launch"""
    from ocrl_amd.sb3s import dqn
    plain, off = build_loop("dqn"), build_loop("mdqn", "sb3.algo_kwargs.munchausen=False")
    keep = dqn.munchausen_targets

    def never(*a, **k):
        raise AssertionError("munchausen_targets ran with munchausen=False")
    dqn.munchausen_targets = never
    try:
        plain.learn(48)
        off.learn(48)
    finally:
        dqn.munchausen_targets = keep
    assert off.n_updates == 2 and torch.equal(off.flat_p, plain.flat_p) and torch.equal(off.flat_v, plain.flat_v)
    on = build_loop("mdqn")
    on.learn(48)
    assert on.n_updates == 2 and not torch.equal(on.flat_p, plain.flat_p) and math.isfinite(on.train_stats()["loss"])


@pytest.mark.parametrize("sb3", ["mdqn", "miqn"])
def test_train_sb3_builds_and_checkpoints_round_trip(sb3, tmp_path):
    model = build_loop(sb3)
    assert model.munchausen and (model.munchausen_alpha, model.munchausen_tau, model.munchausen_clip) == (0.9, 0.03, -1.0)
    losses = []
    model.learn(48, callback=lambda loc: losses.append(loc["train"]["loss"]))
    assert model.iteration == 3 and model.n_updates == 2 and math.isnan(losses[0]) and all(math.isfinite(l) for l in losses[1:])
    assert torch.isfinite(model.flat_p).all()
    path = str(tmp_path / "m.pt")
    model.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert {k: ck["hyper"][k] for k in ("munchausen", "munchausen_alpha", "munchausen_tau", "munchausen_clip")} == dict(
        munchausen=True, munchausen_alpha=0.9, munchausen_tau=0.03, munchausen_clip=-1.0)
    other = build_loop(sb3, "seed=5")
    assert not torch.equal(other.flat_p, model.flat_p) and other.load(path) is other
    for k in ("flat_p", "flat_target", "flat_m", "flat_v"):
        assert torch.equal(getattr(other, k), getattr(model, k)), k
    assert other.munchausen is True and other.n_updates == 2
    for over, key in ((["sb3.algo_kwargs.munchausen=False"], "munchausen"), (["sb3.algo_kwargs.munchausen_tau=0.1"], "munchausen_tau"),
                      (["sb3.algo_kwargs.munchausen_alpha=0.5"], "munchausen_alpha"), (["sb3.algo_kwargs.munchausen_clip=-2.0"], "munchausen_clip")):
        cat = build_loop(sb3, *over)
        hold = cat.flat_p.clone()
        with pytest.raises(ValueError, match=f"the checkpoint was written with {key} = "):
            cat.load(path)
        assert torch.equal(cat.flat_p, hold)


def test_an_iqn_checkpoint_without_the_keys_loads_as_munchausen_off(tmp_path):
    model = build_loop("iqn")
    model.learn(32)
    path = str(tmp_path / "iqn.pt")
    model.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("munchausen", "munchausen_alpha", "munchausen_tau", "munchausen_clip"):
        assert k in ck["hyper"]
        del ck["hyper"][k]
    torch.save(ck, path)
    other = build_loop("iqn", "seed=5")
    assert other.load(path) is other and other.munchausen is False and torch.equal(other.flat_p, model.flat_p)
    with pytest.raises(ValueError, match="the checkpoint was written with munchausen = False, this instance has munchausen = True"):
        build_loop("miqn", "sb3.algo_kwargs.double_q=False").load(path)
