"""GPU checks of DQN's replay extensions (include/ocrl_hip_replay.h) through the C ABI and through ``ReplayBuffer`` / ``dqn_loss`` /
``DQN``, against the restatements of tests/replay_ext_ref.py.

Bounds.  The n-step read and both sampling rules are exact (the returns and discounts bit for bit against the float32 loop).  The extended
TD step carries the bounds of tests/test_gpu_dqn.py::test_td_step_against_fp64: scalars 1e-4 with the 1e-3 floor, dw and dfeatures 3e-4 of
the largest gradient with the 1e-3 floor; |delta| per row, an array like dfeatures, is held to the tighter of the two figures, 1e-4 of the
largest |delta|.  With no option given every output is ocrl_dqn_td_fwd_bwd's bit for bit.  The priority store: a stored priority lies within
1 + q * 2^-20 of the float64 rule (1 for a rounding boundary, 2^-20 for fp32 powf and one product) and is exact at alpha 0 and 1; sums
and sampled ids are exact integers; an importance weight lies within 8 x the numpy-float32 restatement's own worst deviation from float64
on the same inputs, and never less than 4 ulp, of the float64 value (device powf is specified to a few ulp only), and is exactly 1 at
beta 0."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import dqn_ref as R
from tests import replay_ext_ref as X
from tests.gpu_util import log
from tests.test_gpu_dqn import GAMMA, LAYOUTS, SHAPES, err, nanlike, run_td, td_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ 1. the n-step read and sampling
N, E = 7, 3
OBS = {"S20": ((5,), torch.float32), "S48": ((3, 4, 4), torch.uint8)}
GAMMA_N = 0.9


@functools.lru_cache(maxsize=None)
def ring(kind, pos):
    """a full ring on the CPU: env 0 finishes in slots 1 and 4, env 1 in the slot just before pos, env 2 never"""
    shape, dtype = OBS[kind]
    gen = torch.Generator().manual_seed(23)
    obs = torch.randint(0, 256, (N, E, *shape), generator=gen)
    obs = obs.to(dtype) if dtype == torch.uint8 else obs.float() / 7
    actions = torch.randint(0, 4, (N, E), generator=gen)
    rewards = torch.randn(N, E, generator=gen)
    dones = torch.zeros(N, E, dtype=torch.uint8)
    dones[1, 0] = dones[4, 0] = 1
    dones[(pos - 1) % N, 1] = 1
    return obs, actions, rewards, dones


def c_gather(r, ids, n, gamma):
    """ocrl_replay_gather_nstep (n >= 1) or ocrl_replay_gather (n None) on the ring r"""
    lib, L = _lib()
    obs, actions, rewards, dones = (t.cuda() for t in r)
    S = obs[0, 0].numel() * obs.element_size()
    idx = torch.as_tensor(ids, dtype=torch.int64).cuda()
    B = idx.numel()
    o, nx = (torch.full((B, *obs.shape[2:]), 77, device="cuda", dtype=obs.dtype) for _ in range(2))
    a, rw, dn, dc = torch.full((B,), -7, device="cuda", dtype=torch.int64), nanlike(B), torch.full((B,), 9, device="cuda", dtype=torch.uint8), nanlike(B)
    if n is None:
        lib.check(L.ocrl_replay_gather(lib.ptr(obs), lib.ptr(actions), lib.ptr(rewards), lib.ptr(dones), N, E, S, lib.ptr(idx), B, lib.ptr(o), lib.ptr(nx),
                                       lib.ptr(a), lib.ptr(rw), lib.ptr(dn), lib.stream()))
    else:
        lib.check(L.ocrl_replay_gather_nstep(lib.ptr(obs), lib.ptr(actions), lib.ptr(rewards), lib.ptr(dones), N, E, S, n, gamma, lib.ptr(idx), B,
                                             lib.ptr(o), lib.ptr(nx), lib.ptr(a), lib.ptr(rw), lib.ptr(dn), lib.ptr(dc), lib.stream()))
    torch.cuda.synchronize()
    return o.cpu(), nx.cpu(), a.cpu(), rw.cpu(), dn.cpu(), dc.cpu()


@pytest.mark.parametrize("full", [0, 1], ids=["filling", "full"])
@pytest.mark.parametrize("pos", [0, 3, 6])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("kind", ["S20", "S48"])
def test_nstep_gather_and_sample_follow_the_rules(kind, n, pos, full):
    lib, L = _lib()
    r = ring(kind, pos)
    obs, actions, rewards, dones = r
    ids = list(range(N * E)) + [-4, N * E, N * E + 100, 7, 7]                  # every id (every window wraps somewhere), ids outside, a repeat
    o, nx, a, rw, dn, dc = c_gather(r, ids, n, GAMMA_N)
    wR, wg, wstop, wm = X.nstep_walk(rewards.numpy(), dones.numpy(), N, E, n, GAMMA_N, ids)
    c = torch.as_tensor(ids).clamp(0, N * E - 1)
    t, e = c // E, c % E
    tn = (t + torch.as_tensor(wm)) % N
    assert torch.equal(o, obs[t, e]) and torch.equal(nx, obs[tn, e]) and torch.equal(a, actions[t, e])
    assert np.array_equal(rw.numpy().view(np.int32), wR.view(np.int32)) and np.array_equal(dc.numpy().view(np.int32), wg.view(np.int32))
    assert np.array_equal(dn.numpy(), wstop)
    stopped = wstop[:N * E].astype(bool)
    m = wm[:N * E]
    if n == 3:                                                            # a done on the window's first, middle and last step, and none
        assert (stopped & (m == 1)).any() and (stopped & (m == 2)).any() and (stopped & (m == 3)).any() and (~stopped).any()
    tl = (pos - n) % N                                                    # the newest step's done (the slot before pos) ends the window that ends there
    assert wstop[tl * E + 1] == 1 and wm[tl * E + 1] == n
    if n == 1:
        plain = c_gather(r, ids, None, 0.0)
        for got, want in zip((o, nx, a, dn), (plain[0], plain[1], plain[2], plain[4])):
            assert torch.equal(got, want)
        assert torch.equal(bits(rw), bits(plain[3])) and set(dc.tolist()) == {float(np.float32(GAMMA_N))}
    # sampling
    B = 4096
    idx = torch.full((B,), -1, device="cuda", dtype=torch.int64)
    rc = L.ocrl_replay_sample_nstep(21, 6, B, N, E, pos, full, n, lib.ptr(idx), lib.stream())
    if not full and pos < n:
        assert rc != 0 and "pos >= n while the ring is not full" in L.ocrl_last_error().decode()
        return
    lib.check(rc)
    got = idx.cpu().numpy()
    assert np.array_equal(got, X.sample_nstep_rule(21, 6, B, N, E, pos, full, n))
    assert set((got // E).tolist()) == X.valid_slots(N, pos, full, n) and set((got % E).tolist()) == {0, 1, 2}
    if n == 1:
        lib.check(L.ocrl_replay_sample(21, 6, B, N, E, pos, full, lib.ptr(idx), lib.stream()))
        assert np.array_equal(idx.cpu().numpy(), got)
    lib.check(L.ocrl_replay_sample_nstep(21, (1 << 32) + 6, 100, N, E, pos, full, n, lib.ptr(idx), lib.stream()))
    assert np.array_equal(idx.cpu().numpy()[:100], X.sample_nstep_rule(21, (1 << 32) + 6, 100, N, E, pos, full, n))


def test_replay_buffer_reads_nstep_batches():
    from ocrl_amd.sb3s import ReplayBuffer
    obs, actions, rewards, dones = ring("S48", 3)
    buf = ReplayBuffer(N * E, E, (3, 4, 4), "cuda", torch.uint8, seed=4, n_step=3)
    for k in range(N + 3):                                                 # wraps: pos = 3, full
        s = k % N
        buf.add(obs[s], obs[(s + 1) % N], actions[s], rewards[s], dones[s])
    assert (buf.pos, buf.full, len(buf)) == (3, True, (N - 3) * E) and buf.priorities is None
    idx = buf.sample_indices(64, 5, n_step=3)
    assert np.array_equal(idx.cpu().numpy(), X.sample_nstep_rule(4, 5, 64, N, E, 3, 1, 3))
    assert np.array_equal(buf.sample_indices(64, 5).cpu().numpy(), R.sample_rule(4, 5, 64, N, E, 3, 1))
    b = buf.gather(idx, 3, GAMMA_N)
    wR, wg, wstop, wm = X.nstep_walk(buf.rewards.cpu().numpy(), buf.dones.cpu().numpy(), N, E, 3, GAMMA_N, idx.cpu().numpy())
    t, e = idx.cpu() // E, idx.cpu() % E
    assert np.array_equal(b.rewards.cpu().numpy().view(np.int32), wR.view(np.int32)) and np.array_equal(b.discounts.cpu().numpy().view(np.int32), wg.view(np.int32))
    assert torch.equal(b.next_observations.cpu(), buf.observations.cpu()[(t + torch.as_tensor(wm)) % N, e]) and np.array_equal(b.dones.cpu().numpy(), wstop)
    plain = buf.gather(idx)
    assert plain.discounts is None and len(plain) == 6 and torch.equal(plain.observations, b.observations)
    with pytest.raises(ValueError, match="needs gamma"):
        buf.gather(idx, 3)
    with pytest.raises(RuntimeError, match="without prioritized=True"):
        buf.sample_prioritized(8, 0, 0.4)


# ------------------------------------------------------------------------------------------------------------ 2. the extended TD step
OPTIONS = {"online": (1, 0, 0), "discounts": (0, 1, 0), "weights": (0, 0, 1), "all": (1, 1, 1)}


@functools.lru_cache(maxsize=None)
def ext_case(B, F, A, lname):
    """td_case with a next_q whose first row rises with the action, and the optional inputs: an online Q whose first row is one tie over
    every action (the lowest index, 0, must win: next_q[0, 0] is the row's smallest) and whose other rows are random (their maxima differ
    from the target's), discounts in [0.5, 1) and weights in (0.1, 1]"""
    x, ps, next_q, actions, rewards, dones = td_case(B, F, A, lname)
    next_q = next_q.clone()
    next_q[0] = torch.arange(A, dtype=torch.float32)
    gen = torch.Generator().manual_seed(7 + B)
    online = torch.randn(B, A, generator=gen)
    online[0] = 2.0
    if B > 3 and A > 2:
        online[3, 1] = online[3, A - 1] = 5.0                                # a tie of two: the lower one
    disc = torch.rand(B, generator=gen) * 0.5 + 0.5
    wts = torch.rand(B, generator=gen) * 0.9 + 0.1
    return (x, ps, next_q, actions, rewards, dones), online, disc, wts


def run_td_ext(x, ps, layout, A, next_q, actions, rewards, dones, gamma, online=None, disc=None, wts=None, want_abs=True, want_dx=True):
    lib, L = _lib()
    B, F = x.shape
    d = lib.qnet_desc(B, F, A, *layout)
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd = x.cuda(), [p.cuda() for p in ps]
    dev = lambda t: None if t is None else t.cuda().contiguous()
    nq, on, ac, rw, dn, dc, wt = dev(next_q), dev(online), actions.cuda().long(), dev(rewards), dev(dones), dev(disc), dev(wts)
    scal, dw, dx, ws = nanlike(3), [nanlike(*p.shape) for p in ps], nanlike(B, F) if want_dx else None, nanlike(n)
    ad = nanlike(B) if want_abs else None
    lib.check(L.ocrl_dqn_td_fwd_bwd_ext(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(nq), lib.ptr(on), lib.ptr(ac), lib.ptr(rw), lib.ptr(dn), lib.ptr(dc),
                                        lib.ptr(wt), gamma, lib.ptr(scal), lib.ptr(ad), lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(scal=scal, dw=dw, dx=dx, abs_td=ad)


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A", SHAPES, ids=lambda v: str(v))
def test_td_ext_without_options_is_the_plain_step_bit_for_bit(B, F, A, lname):
    layout = LAYOUTS[lname]
    inp = td_case(B, F, A, lname)
    want = run_td(inp[0], inp[1], layout, A, *inp[2:], GAMMA)
    for want_abs in (False, True):
        got = run_td_ext(inp[0], inp[1], layout, A, *inp[2:], GAMMA, want_abs=want_abs)
        assert torch.equal(bits(got["scal"]), bits(want["scal"])) and torch.equal(bits(got["dx"]), bits(want["dx"]))
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got["dw"], want["dw"]))
    assert torch.isfinite(got["abs_td"]).all()
    nodx = run_td_ext(inp[0], inp[1], layout, A, *inp[2:], GAMMA, want_dx=False)
    assert nodx["dx"] is None and all(torch.equal(a, b) for a, b in zip(nodx["dw"], want["dw"]))


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
@pytest.mark.parametrize("B, F, A", SHAPES, ids=lambda v: str(v))
def test_td_ext_against_fp64(B, F, A, lname, option):
    layout = LAYOUTS[lname]
    inp, online, disc, wts = ext_case(B, F, A, lname)
    use = OPTIONS[option]
    kw = dict(online=online if use[0] else None, disc=disc if use[1] else None, wts=wts if use[2] else None)
    scal, dx, dw, ad = X.td_step_ext(inp[0], inp[1], layout[1], *inp[2:], GAMMA, kw["online"], kw["disc"], kw["wts"])
    got = run_td_ext(inp[0], inp[1], layout, A, *inp[2:], GAMMA, **kw)
    tag = f"B{B} F{F} A{A} {lname} {option}"
    if use[0] and A > 1:
        live = ~inp[5].bool()
        assert (online.argmax(dim=1) != inp[2].argmax(dim=1))[live].any(), tag           # the two networks disagree somewhere: row 0 at least
        plain = X.td_step_ext(inp[0], inp[1], layout[1], *inp[2:], GAMMA, None, kw["disc"], kw["wts"])
        assert (plain[3] - ad).abs().max().item() > 1e-2, tag                            # ... and the target shows it
    smax = scal.abs().max().item()
    worst_s = worst_g = 0.0
    for i, k in enumerate(("loss", "mean_q", "mean_target")):
        e = abs(got["scal"][i].item() - scal[i].item()) / max(abs(scal[i].item()), 1e-3 * smax, 1e-30)
        worst_s = max(worst_s, e)
        assert e <= 1e-4, (tag, k, e, got["scal"].tolist(), scal.tolist())
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    for nme, g, w in zip(["dx"] + [f"dw{i}" for i in range(len(dw))], [got["dx"]] + got["dw"], [dx] + dw):
        e = err(g, w, 1e-3 * gmax)
        worst_g = max(worst_g, e)
        assert e <= 3e-4, (tag, nme, e)
    e_ad = err(got["abs_td"], ad)
    log(f"dqn td ext {tag}: worst scalar rel err {worst_s:.2e} (bound 1e-4), worst gradient {worst_g:.2e} (bound 3e-4), |delta| {e_ad:.2e} (bound 1e-4)")
    assert e_ad <= 1e-4, (tag, e_ad)
    again = run_td_ext(inp[0], inp[1], layout, A, *inp[2:], GAMMA, **kw)
    assert torch.equal(again["scal"], got["scal"]) and torch.equal(again["dx"], got["dx"]) and torch.equal(again["abs_td"], got["abs_td"])


@pytest.mark.parametrize("lname", ["none", "mlp", "tanh"])
def test_an_ext_row_does_not_depend_on_its_position_or_on_the_batch(lname):
    """rows 0 .. 4 of the B = 17 case alone (B = 5) and at the end of the batch, every option given: |delta| bitwise, B * dfeatures to 1e-6
    relative (1 / B is the one operation that differs) and bitwise where only the position changed"""
    layout = LAYOUTS[lname]
    (x, ps, next_q, actions, rewards, dones), online, disc, wts = ext_case(17, 12, 3, lname)
    perm = torch.cat([torch.arange(5, 17), torch.arange(5)])
    sel = lambda p: run_td_ext(x[p], ps, layout, 3, next_q[p], actions[p], rewards[p], dones[p], GAMMA, online[p], disc[p], wts[p])
    full, head, moved = sel(torch.arange(17)), sel(torch.arange(5)), sel(perm)
    assert torch.equal(full["abs_td"][:5], head["abs_td"]) and torch.equal(moved["abs_td"][12:], head["abs_td"]) and torch.equal(moved["abs_td"][:12], full["abs_td"][5:])
    a, b, c = 17 * full["dx"][:5], 5 * head["dx"], 17 * moved["dx"][12:]
    scale = a.abs().max().item()
    assert scale > 0 and (a - b).abs().max().item() <= 1e-6 * scale and torch.equal(a, c)


def test_dqn_loss_routes_to_the_extended_step():
    import types
    from ocrl_amd.sb3s import DQNPolicy, dqn_loss
    B, F, A = 17, 12, 3
    (x, ps, next_q, actions, rewards, dones), online, disc, wts = ext_case(B, F, A, "mlp")
    torch.manual_seed(0)
    pol = DQNPolicy(types.SimpleNamespace(shape=(F,)), types.SimpleNamespace(n=A)).cuda()
    with torch.no_grad():
        for p, v in zip(pol.q_net._param_list(), ps):
            p.copy_(v)
    want = run_td_ext(x, ps, LAYOUTS["mlp"], A, next_q, actions, rewards, dones, GAMMA, online, disc, wts)
    feats = x.cuda().requires_grad_(True)
    loss, m, ad = dqn_loss(pol, feats, next_q.cuda(), actions.cuda(), rewards.cuda(), dones.cuda(), GAMMA, next_q_online=online.cuda(), discounts=disc.cuda(),
                           weights=wts.cuda(), return_abs_td=True)
    loss.backward()
    assert torch.equal(loss.detach(), want["scal"][0]) and torch.equal(ad, want["abs_td"]) and not ad.requires_grad and set(m) == {"loss", "mean_q", "mean_target"}
    assert torch.equal(feats.grad, want["dx"]) and all(torch.equal(p.grad, g) for p, g in zip(pol.q_net._param_list(), want["dw"]))
    # nothing set: the plain entry point's result, two values
    pol.zero_grad()
    out = dqn_loss(pol, x.cuda(), next_q.cuda(), actions.cuda(), rewards.cuda(), dones.cuda(), GAMMA)
    plain = run_td(x, ps, LAYOUTS["mlp"], A, next_q, actions, rewards, dones, GAMMA)
    assert len(out) == 2 and torch.equal(out[0].detach(), plain["scal"][0])
    out = dqn_loss(pol, x.cuda(), next_q.cuda(), actions.cuda(), rewards.cuda(), dones.cuda(), GAMMA, weights=wts.cuda())
    assert len(out) == 2 and not torch.equal(out[0].detach(), plain["scal"][0])


# ------------------------------------------------------------------------------------------------------------ 3. the priority store
F_ = X.FAN
STORE_SIZES = [21, F_ + 1, F_ * F_ + 1, F_ ** 3 + 1]                       # one, two, three and four levels; each a partial last node


class Store:
    """a priority store of NE ids on the GPU, driven through the C ABI and read back whole"""

    def __init__(self, NE):
        lib, L = _lib()
        self.NE, self.lib, self.L = NE, lib, L
        nbytes = L.ocrl_per_bytes(NE)
        assert nbytes == X.store_bytes(NE)
        self.raw = torch.full((nbytes // 8,), 0x5555555555555555, device="cuda", dtype=torch.int64)      # every word must be written by init
        lib.check(L.ocrl_per_init(lib.ptr(self.raw), NE, lib.stream()))

    def read(self):
        torch.cuda.synchronize()
        return X.parse_store(self.raw.cpu().numpy().view(np.uint8), self.NE)

    def check_sums(self):
        leaves, maxq, levels = self.read()
        assert levels == X.level_sums(leaves)
        return leaves, maxq

    def set_range(self, first, count, mode):
        self.lib.check(self.L.ocrl_per_set_range(self.lib.ptr(self.raw), self.NE, first, count, mode, self.lib.stream()))

    def update(self, idx, abs_td, alpha, eps):
        i, a = torch.as_tensor(idx, dtype=torch.int64).cuda(), torch.as_tensor(abs_td, dtype=torch.float32).cuda()
        self.lib.check(self.L.ocrl_per_update(self.lib.ptr(self.raw), self.NE, self.lib.ptr(i), self.lib.ptr(a), i.numel(), alpha, eps, self.lib.stream()))

    def sample(self, B, beta, seed=0, update=0, targets=None):
        t = None if targets is None else torch.as_tensor(np.asarray(targets, dtype=np.uint64).view(np.int64)).cuda()
        idx, w = torch.full((B,), -5, device="cuda", dtype=torch.int64), nanlike(B)
        self.lib.check(self.L.ocrl_per_sample(self.lib.ptr(self.raw), self.NE, seed, update, B, beta, self.lib.ptr(t), self.lib.ptr(idx), self.lib.ptr(w),
                                              self.lib.stream()))
        torch.cuda.synchronize()
        return idx.cpu().numpy(), w.cpu().numpy()


def runs(NE):
    """two runs of leaves to fill, [a0, a1) and [b0, b1): zero leaves stay at the start, in the middle and at the end"""
    return (3, NE // 3 + 2), (NE // 2 + 2, NE - 2)


def error_of(NE, ids):
    """|TD error| of an id: a function of the id, so that a repeated id carries one value"""
    table = np.abs(np.random.default_rng(NE).normal(size=NE)).astype(np.float32) * 3
    return table[np.asarray(ids)]


def filled(NE, alpha):
    """a store whose two runs were filled and then updated with a batch that has zero and non-zero leaves, a repeat, errors of 0, 1e4 and
    inf; returns (store, ids, errors)"""
    s = Store(NE)
    (a0, a1), (b0, b1) = runs(NE)
    s.set_range(a0, a1 - a0, 1)
    s.set_range(b0, b1 - b0, 1)
    fixed = [0, a0, a1 - 1, b0, b1 - 1, NE - 1, a0 + 1, a0 + 1]
    drawn = np.random.default_rng(NE + 1).integers(0, NE, 29)
    drawn[np.isin(drawn, fixed)] = a0 + 2                                   # the ids below get errors of their own
    ids = np.concatenate([drawn, fixed])
    errs = error_of(NE, ids)
    errs[29] = 40.0                                                         # the largest finite error sits on a zero leaf (id 0)
    errs[30], errs[31], errs[32] = 0.0, 1e4, np.inf
    s.update(ids, errs, alpha, 1e-6)
    return s, ids, errs


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("NE", STORE_SIZES)
def test_priority_store_leaves_maxq_and_sums(NE, alpha):
    s = Store(NE)
    leaves, maxq, levels = s.read()
    assert not leaves.any() and maxq == X.Q_ONE and all(v == 0 for lv in levels for v in lv) and [len(lv) for lv in levels] == X.level_sizes(NE)
    (a0, a1), (b0, b1) = runs(NE)
    s.set_range(a0, a1 - a0, 1)
    s.set_range(b0, b1 - b0, 1)
    leaves, maxq = s.check_sums()
    want = np.zeros(NE, dtype=np.int64)
    want[a0:a1] = want[b0:b1] = X.Q_ONE
    assert np.array_equal(leaves, want) and maxq == X.Q_ONE
    s, ids, errs = filled(NE, alpha)
    leaves, maxq = s.check_sums()
    q32, q64 = X.quantise(errs, alpha, 1e-6), X.quantise64(errs, alpha, 1e-6)
    tol = 1 + q64 * 2.0 ** -20
    live = want[ids] != 0
    assert live.any() and (~live).any()
    assert (np.abs(leaves[ids[live]] - q64[live]) <= tol[live]).all(), (leaves[ids[live]], q64[live])
    assert not leaves[ids[~live]].any() and not leaves[want == 0].any()                   # a zero leaf stays zero
    untouched = np.setdiff1d(np.nonzero(want)[0], ids)
    assert (leaves[untouched] == X.Q_ONE).all()
    if alpha in (0.0, 1.0):
        assert np.array_equal(leaves[ids[live]], q32[live])
        assert maxq == max(X.Q_ONE, int(q32.max()))
    assert maxq == (X.Q_MAX if alpha else X.Q_ONE)                                      # the infinite error, over every row
    log(f"per NE{NE} alpha{alpha}: worst |q - q64| {np.abs(leaves[ids[live]] - q64[live]).max()} of q up to {q64[live].max()}")
    # maxq follows rows whose leaf is zero, to the same tolerance: a fresh store, finite errors only
    t = Store(NE)
    t.set_range(a0, a1 - a0, 1)
    t.update(ids[:30], errs[:30], alpha, 1e-6)
    want_max = max(X.Q_ONE, int(X.quantise64(errs[:30], alpha, 1e-6).max()))
    _, maxq = t.check_sums()
    assert abs(maxq - want_max) <= 1 + want_max * 2.0 ** -20 and (alpha == 0 or maxq > X.Q_ONE)
    # new leaves take the running maximum; mode 0 clears; the last leaf alone in its node
    t.set_range(b0, b1 - b0, 1)
    t.set_range(a0, 2, 0)
    t.set_range(NE - 1, 1, 1)
    leaves, m2 = t.check_sums()
    assert m2 == maxq and (leaves[b0:b1] == maxq).all() and not leaves[a0:a0 + 2].any() and leaves[NE - 1] == maxq and not leaves[b1:NE - 1].any()
    idx, _ = t.sample(2, 0.0, targets=[0, int(leaves.sum()) - 1])
    assert idx.tolist() == [a0 + 2, NE - 1]


@pytest.mark.parametrize("NE", STORE_SIZES)
def test_priority_store_sampling_is_the_exact_prefix_search(NE):
    s, ids, errs = filled(NE, 0.6)
    leaves, _ = s.check_sums()
    prefix = np.cumsum(leaves)
    total = int(prefix[-1])
    nz = np.nonzero(leaves)[0]
    u64 = lambda v: np.asarray(v, dtype=np.uint64)
    targets = np.concatenate([u64([0, total - 1]), u64(prefix[nz] - 1), u64(prefix[nz]), u64([total, total + 5, 2 ** 63])])      # past the total: clamped
    idx, w = s.sample(targets.size, 0.0, targets=targets)
    assert np.array_equal(idx, X.search(leaves, targets)) and leaves[idx].all() and (w == 1.0).all()
    assert idx[0] == nz[0] and idx[1] == nz[-1] and set(idx.tolist()) == set(nz.tolist())
    for seed, update in ((3, 0), (11, (1 << 32) + 7)):
        idx, w = s.sample(512, 0.0, seed=seed, update=update)
        assert np.array_equal(idx, X.search(leaves, X.draw_targets(seed, update, 512, total))), (seed, update)
        assert np.array_equal(s.sample(64, 0.0, seed=seed, update=update)[0], idx[:64])             # a pure function of (seed, update, row)
    # an empty store cannot be sampled: ids -1, weights 0
    idx, w = Store(NE).sample(5, 0.4)
    assert idx.tolist() == [-1] * 5 and w.tolist() == [0.0] * 5


@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
def test_importance_weights(beta):
    NE = F_ * F_ + 1
    s, ids, errs = filled(NE, 0.6)
    rng = np.random.default_rng(5)
    extra = rng.integers(3, NE // 3, 200)
    s.update(extra, error_of(NE, extra), 0.6, 1e-6)                        # a spread of priorities
    leaves, _ = s.check_sums()
    idx, w = s.sample(1024, beta, seed=9, update=1)
    q = leaves[idx]
    assert len(set(q.tolist())) > 20
    w64, w32 = X.weights_rule(q, beta, np.float64), X.weights_rule(q, beta, np.float32)
    assert w.dtype == np.float32 and (w > 0).all() and (w <= 1).all() and w.max() == 1.0
    if beta == 0.0:
        assert (w == 1.0).all()
        return
    dev32 = (np.abs(w32.astype(np.float64) - w64) / w64).max()
    rel = np.abs(w.astype(np.float64) - w64) / w64
    bound = np.maximum(8 * dev32, 4 * np.spacing(w64.astype(np.float32)).astype(np.float64) / w64)
    log(f"per weights beta {beta}: worst rel err {rel.max():.3e} (numpy float32 {dev32:.3e}; bound {bound.min():.3e} .. {bound.max():.3e})")
    assert (rel <= bound).all(), (rel.max(), dev32)
    if beta == 1.0:
        assert np.array_equal(w, w32)                                        # one correctly rounded division


def test_replay_buffer_keeps_the_leaves_valid():
    from ocrl_amd.sb3s import ReplayBuffer
    Nb, Eb, n = 6, 4, 3
    buf = ReplayBuffer(Nb * Eb, Eb, (5,), "cuda", torch.float32, seed=2, prioritized=True, n_step=n)
    assert buf.priorities.numel() == X.store_bytes(Nb * Eb) and buf.priorities.data_ptr() % 8 == 0
    with pytest.raises(RuntimeError, match="no whole window"):
        buf.sample_prioritized(4, 0, 0.4)
    gen = torch.Generator().manual_seed(1)
    for k in range(2 * Nb + 1):
        buf.add(torch.rand(Eb, 5, generator=gen), torch.rand(Eb, 5, generator=gen), torch.zeros(Eb), torch.rand(Eb, generator=gen), torch.zeros(Eb))
        torch.cuda.synchronize()
        leaves, maxq, levels = X.parse_store(buf.priorities.cpu().numpy(), Nb * Eb)
        slots = {int(t) for t in np.nonzero(leaves.reshape(Nb, Eb).any(axis=1))[0]}
        assert slots == X.valid_slots(Nb, buf.pos, buf.full, n) and len(buf) == len(slots) * Eb, k
        assert levels == X.level_sums(leaves) and (k > 4 or set(leaves[leaves != 0].tolist()) <= {maxq})
        if k == 4:                                                          # raise the maximum: later slots enter with it
            idx, w = buf.sample_prioritized(8, 0, 0.4)
            assert np.array_equal(idx.cpu().numpy(), X.search(leaves, X.draw_targets(2, 0, 8, int(leaves.sum()))))
            buf.update_priorities(idx, torch.full((8,), 3.0), 1.0, 0.0)
            buf.update_priorities(idx, torch.full((8,), 0.5), 1.0, 0.0)
            torch.cuda.synchronize()
            l2, m2, _ = X.parse_store(buf.priorities.cpu().numpy(), Nb * Eb)
            assert m2 == 3 * X.Q_ONE and set(l2[idx.cpu().numpy()].tolist()) == {X.Q_ONE // 2}
    assert maxq == 3 * X.Q_ONE and (leaves == maxq).sum() >= Eb


# ------------------------------------------------------------------------------------------------------------ 4. the loop
LOOP = ["sb3.algo_kwargs.buffer_size=256", "sb3.algo_kwargs.learning_starts=16", "sb3.algo_kwargs.train_freq=4", "sb3.algo_kwargs.target_update_interval=8",
        "sb3.algo_kwargs.batch_size=8", "+sb3.algo_kwargs.log_interval=1", "sb3.algo_kwargs.learning_rate=1e-3", "env.max_steps=6"]
TOTAL = 96


def build_loop(sb3="dqn_per", *over):
    import train_sb3
    from ocrl_amd.utils.config import compose
    c = compose(CFG, "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0"] + LOOP + list(over))
    return train_sb3.build(c)[2]


def run_per_loop():
    model = build_loop()
    assert (model.n_step, model.double_q, model.prioritized_replay) == (3, True, True)
    rows = []

    def cb(loc):
        w = model.last_weights
        rows.append((loc["train"]["loss"], None if w is None else w.cpu().numpy().copy(), model.beta()))
    model.learn(TOTAL, callback=cb)
    return model, rows


def test_the_loop_with_all_three_extensions(tmp_path):
    model, rows = run_per_loop()
    assert model.n_updates == 5 and model.num_timesteps == TOTAL and rows[0][1] is None and np.isnan(rows[0][0])
    for loss, w, beta in rows[1:]:
        assert np.isfinite(loss) and w.shape == (8,) and (w > 0).all() and (w <= 1).all() and w.max() == 1.0
    assert [r[2] for r in rows] == pytest.approx([0.4 + 0.6 * t / TOTAL for t in range(16, TOTAL + 1, 16)])          # beta: linear in num_timesteps / total
    buf = model.replay_buffer
    assert buf.n_slots == 64 and buf.pos == 24 and not buf.full and buf.prioritized and buf.n_step == 3
    leaves, maxq, levels = X.parse_store(buf.priorities.cpu().numpy(), 64 * 4)
    slots = {int(t) for t in np.nonzero(leaves.reshape(64, 4).any(axis=1))[0]}
    assert slots == set(range(22)) and not leaves.reshape(64, 4)[22:].any()            # never the n newest slots (22, 23 and pos = 24)
    assert levels == X.level_sums(leaves) and len(set(leaves[leaves != 0].tolist())) > 1 and maxq >= leaves.max()
    twin, rows2 = run_per_loop()
    assert torch.equal(twin.flat_p, model.flat_p) and torch.equal(twin.flat_v, model.flat_v) and torch.equal(twin.replay_buffer.priorities, buf.priorities)
    assert [r[0] for r in rows2[1:]] == [r[0] for r in rows[1:]] and all(np.array_equal(a[1], b[1]) for a, b in zip(rows[1:], rows2[1:]))
    # checkpoints carry the new hyper-parameters; one without them leaves the constructor's values
    path = str(tmp_path / "per.pt")
    model.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    new = dict(double_q=True, n_step=3, prioritized_replay=True, prioritized_replay_alpha=0.6, prioritized_replay_beta0=0.4,
               prioritized_replay_beta_final=1.0, prioritized_replay_eps=1e-6)
    assert {k: ck["hyper"][k] for k in new} == new
    other = build_loop("dqn_per", "sb3.algo_kwargs.n_step=2", "sb3.algo_kwargs.prioritized_replay_alpha=0.5", "sb3.algo_kwargs.double_q=False")
    other.collect_step()
    assert other.replay_buffer.n_step == 2
    other.load(path)
    assert {k: getattr(other, k) for k in new} == new and torch.equal(other.flat_p, model.flat_p)
    assert other.replay_buffer is None                                     # built for another n_step: the next collect_step builds one that fits
    other.collect_step()
    assert other.replay_buffer.n_step == 3 and other.replay_buffer.prioritized
    for k in new:
        del ck["hyper"][k]
    old = str(tmp_path / "old.pt")
    torch.save(ck, old)
    other = build_loop("dqn_per", "sb3.algo_kwargs.n_step=2", "sb3.algo_kwargs.prioritized_replay_alpha=0.5")
    other.load(old)
    assert (other.n_step, other.prioritized_replay_alpha, other.double_q) == (2, 0.5, True) and torch.equal(other.flat_p, model.flat_p)


def test_default_kwargs_change_nothing():
    """passes before this feature too, without the explicit arguments: the guard of `no behaviour change`"""
    plain = build_loop("dqn")
    explicit = build_loop("dqn", "+sb3.algo_kwargs.double_q=False", "+sb3.algo_kwargs.n_step=1", "+sb3.algo_kwargs.prioritized_replay=False",
                          "+sb3.algo_kwargs.prioritized_replay_alpha=0.6", "+sb3.algo_kwargs.prioritized_replay_beta0=0.4",
                          "+sb3.algo_kwargs.prioritized_replay_beta_final=1.0", "+sb3.algo_kwargs.prioritized_replay_eps=1e-6")
    plain.learn(TOTAL)
    explicit.learn(TOTAL)
    assert plain.n_updates == explicit.n_updates == 5 and getattr(plain.replay_buffer, "priorities", None) is None and getattr(explicit, "last_weights", None) is None
    assert torch.equal(plain.flat_p, explicit.flat_p) and torch.equal(plain.flat_target, explicit.flat_target) and torch.equal(plain.flat_v, explicit.flat_v)
    used = plain.replay_buffer.pos + 1                                     # the slots written so far (the ring has not wrapped)
    assert used == 25 and torch.equal(plain.replay_buffer.observations[:used], explicit.replay_buffer.observations[:used])


@pytest.mark.parametrize("option", ["sb3.algo_kwargs.n_step=1", "sb3.algo_kwargs.double_q=False", "sb3.algo_kwargs.prioritized_replay=False"])
def test_the_loop_with_one_extension_off(option):
    model = build_loop("dqn_per", option)
    model.learn(48)
    assert model.n_updates == 2 and np.isfinite(model.train_stats()["loss"]) and (model.last_weights is None) == (option.endswith("replay=False"))


def test_learning_starts_must_leave_a_whole_window():
    model = build_loop("dqn_per", "sb3.algo_kwargs.n_step=5", "sb3.algo_kwargs.learning_starts=0")
    for _ in range(4):
        model.collect_step()
    with pytest.raises(RuntimeError, match="learning_starts = 0 leaves 4 vec steps .* fewer than n_step = 5"):
        model.train_step()
    model.collect_step()
    assert torch.isfinite(model.train_step())
