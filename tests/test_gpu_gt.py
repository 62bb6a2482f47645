"""GPU checks of the ground-truth-state encoder (ocr=gt): the state observations (ocrl_sprite_state_obs, SpriteEnv in render_mode
state), the fused per-object MLP (ocrl_gt_mlp_fwd / _bwd), GT_Module against the reference's fixture, the extractor over every pooling
head, and train_sb3 end to end.

Bounds.  State observations: bitwise against tests/gt_ref.state_obs (copies and comparisons, no arithmetic).  The MLP, for the output and
every gradient tensor: err = max|. - fp64| / max|fp64| with the fp64 restatement of tests/gt_ref.py, and

    err_kernel <= 4 err_eager + 4 * 2^-24

where err_eager is torch's own fp32 chain (F.linear, relu, autograd: the reference's arithmetic) on the same GPU and inputs.  The kernel
sums the same <= 256 terms in another order, hence the factor; the floor is for tensors eager happens to get exactly.  A wrong or missing
term shows at 1e-2.  Before that the test asserts in fp64 that every ReLU pre-activation has |z| >= 1e-4 max|z| of its layer, so that no
ReLU decision is within three orders of magnitude of fp32 rounding and both fp32 runs take the fp64 run's branches."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from ocrl_amd.utils.config import compose
from tests import gt_ref as G
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
BASE = ["ocr=gt", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "device=cuda:0"]
F = np.float32
STATE = ["env.num_objects_range=[2,4]", "env.SCALES=[0.15,0.22]", "env.render_mode=state"]


def config(*over, env="target-N4C4S3S1"):
    return compose(CFG, "train_sb3", BASE + [f"env={env}"] + list(over))


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. state observations
def check_obs(env, obs):
    assert obs.dtype == torch.float32 and obs.is_cuda and tuple(obs.shape) == (env.num_envs, env.rows, 5)
    rows = env.get_state()["rows"]
    assert np.array_equal(bits(obs), bits(G.state_obs(rows.cpu().numpy())))
    assert torch.equal(env.render("state"), rows) and torch.equal(env.observe(), obs)      # render("state") stays the raw rows


@pytest.mark.parametrize("E", [1, 3, 64, 130])
def test_state_observations_of_the_target_task(E):
    from ocrl_amd import envs
    env = envs.TargetEnv(config(*STATE, "env.max_steps=3").env, E, seed=E, device="cuda")
    assert env.observation_space.shape == (5, 5) and env.observation_space.dtype == np.float32
    assert np.all(np.asarray(env.observation_space.low) == 0) and np.all(np.asarray(env.observation_space.high) == 1)
    obs = env.reset()
    check_obs(env, obs)
    seen = obs.clone()
    g = torch.Generator().manual_seed(E)
    for t in range(5):                                         # max_steps = 3: auto-resets fall inside the five steps
        obs, rewards, dones, ex = env.step_device(torch.randint(0, 4, (E,), generator=g).cuda())
        check_obs(env, obs)
        assert rewards.shape == (E,) and dones.dtype == torch.bool and obs.data_ptr() not in (seen.data_ptr(), env._rows.data_ptr())
    n = env.get_state()["n"]
    if E >= 64:                                                # both scales, and padding rows after the agent, do occur
        assert set(obs[..., 2].unique().tolist()) == {0.0, 1.0} and int(n.min()) < 4
        pad = torch.arange(5, device="cuda")[None, :] > n[:, None]
        assert not obs[pad].any()
    obs2, _, _, _ = env.step(np.zeros(E, dtype=np.int64))      # the gym-style call hands out the same kind of observation
    check_obs(env, obs2)


def test_state_observations_of_the_odd_one_out_task():
    from ocrl_amd import envs
    env = envs.OddOneOutEnv(config("env.render_mode=state", env="odd-one-out-N4C2S2S2").env, 33, seed=2, device="cuda")
    assert env.observation_space.shape == (5, 5)
    check_obs(env, env.reset())
    assert torch.equal(env.state_obs(env.get_state()["rows"].cpu()), env.observe())       # hand-made rows take the same kernel
    for t in range(3):
        check_obs(env, env.step_device(torch.full((33,), t, dtype=torch.int64, device="cuda"))[0])


def hand_rows(E, R):
    """the CPU test's cases cycled over E x R rows: both scales, empty rows, colour -1 with a position, an agent-like row, another scale"""
    kinds = np.array([[1, 2, F(0.15), 0.25, 0.75], [3, 0, F(0.22), 0.5, 0.125], [-1, 1, F(0.22), 0.375, 0.625], [3, 3, F(0.15), 0.5, 0.5],
                      [0, 0, 0, 0, 0], [0, 0, F(0.15), 0, 0], [2, 1, F(0.3), 0.5, 0.5], [-1, -1, -1, 0.5, 0.5], [0, 0, 0, 0, 0.5]], dtype=F)
    idx = (np.arange(E * R) * 7 + np.arange(E * R) // 9) % len(kinds)
    rows = kinds[idx].reshape(E, R, 5).copy()
    rows[..., 3] += (np.arange(E * R).reshape(E, R) % 5).astype(F) / 16
    return rows


@pytest.mark.parametrize("E,R", [(1, 1), (2, 6), (7, 16), (13, 5), (64, 4), (200, 11)])
def test_state_obs_entry_on_hand_made_rows(E, R):
    from ocrl_amd import _lib
    rows = hand_rows(E, R)
    want = G.state_obs(rows)
    assert {-1.0, 0.0, 1.0} <= set(want[..., 2].flatten().tolist()) or E * R < 9
    d_rows = torch.from_numpy(rows).cuda()
    out = torch.full((E * R * 5 + 64,), 7.0, device="cuda")    # a guard after the output: one thread per row writes its five floats only
    _lib.check(_lib.lib().ocrl_sprite_state_obs(_lib.ptr(d_rows), E, R, _lib.ptr(out), _lib.stream()))
    assert np.array_equal(bits(out[:E * R * 5].view(E, R, 5)), bits(want)) and bool((out[E * R * 5:] == 7.0).all())
    assert torch.equal(d_rows, torch.from_numpy(rows).cuda())


def test_an_image_mode_environment_is_unchanged():
    from ocrl_amd import envs
    c = config("env.num_objects_range=[2,4]", "env.SCALES=[0.15,0.22]")
    a, b = envs.TargetEnv(c.env, 6, seed=5, device="cuda"), envs.TargetEnv(c.env, 6, seed=5, device="cuda")
    fa, fb = a.reset(), b.reset()
    assert fa.dtype == torch.uint8 and tuple(fa.shape) == (6, 3, 64, 64) and torch.equal(fa, fb) and a.observation_space.shape == (3, 64, 64)
    assert torch.equal(a.observe(), fa) and torch.equal(fa, a.render("image"))
    act = torch.tensor([0, 1, 2, 3, 0, 1], device="cuda")
    assert torch.equal(a.step_device(act)[0], b.step_device(act)[0])
    s = envs.TargetEnv(config(*STATE).env, 6, seed=5, device="cuda")       # the state-mode twin walks the same episodes
    s.reset()
    s.step_device(act)
    assert torch.equal(s.get_state()["rows"], a.get_state()["rows"]) and torch.equal(s.render("image"), a.render("image"))


# ---------------------------------------------------------------------------------------------------------------- 2. MLP parity
# (B, K, dims, acts, seed)
# seeds: the first, counting up from the one the case was written with, at which this file's draw order passes the ReLU margin below
MLP_CASES = [(1, 5, [4], ["relu"], 0), (7, 5, [8, 12], ["relu", "relu"], 1), (7, 5, [64, 64, 128], ["relu", "relu", "none"], 3),
             (67, 5, [8], ["relu"], 0), (3, 5, [20, 256], ["relu", "none"], 1)]
RELU_MARGIN = 1e-4


def draw(B, K, dims, seed, D=5):
    """a seeded state [B, K, 5] (ids, a scale index, uniform positions) and the layers' parameters with torch's Linear bounds
    (uniform in +- 1 / sqrt(fan_in)), drawn in the order state, then W and b of each layer"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randint(0, 7, (B, K), generator=g), torch.randint(0, 4, (B, K), generator=g), torch.randint(0, 2, (B, K), generator=g)], -1).float()
    x = torch.cat([ids, torch.rand(B, K, 2, generator=g)], -1)
    params, fan_in = [], D
    for d in dims:
        bound = 1.0 / math.sqrt(fan_in)
        params += [(torch.rand(d, fan_in, generator=g) * 2 - 1) * bound, (torch.rand(d, generator=g) * 2 - 1) * bound]
        fan_in = d
    return x, params


def relu_margins(x, params, acts):
    """min |z| / max |z| over each ReLU layer's pre-activations, in fp64"""
    _, zs = G.gt_mlp(x.numpy(), [p.numpy() for p in params], acts)
    return [float(np.abs(z).min() / np.abs(z).max()) for z, a in zip(zs, acts) if a == "relu"]


def relmax(got, ref):
    return float(np.abs(got.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max())


def eager(x, params, acts):
    h = x
    for l, a in enumerate(acts):
        h = Fn.linear(h, params[2 * l], params[2 * l + 1])
        h = torch.relu(h) if a == "relu" else h
    return h


def run_both(x, params, acts, cot, need_dx=True):
    """(kernel, eager) -> [out, dx, dW_0, db_0, ..] each"""
    from ocrl_amd.ocrs.gt import gt_mlp
    res = []
    for fn in (gt_mlp, eager):
        xs = x.clone().cuda().requires_grad_(need_dx)
        ps = [p.clone().cuda().requires_grad_(True) for p in params]
        out = fn(xs, ps, acts)
        (out * cot.cuda()).sum().backward()
        res.append([out.detach(), xs.grad] + [p.grad for p in ps])
    return res


@pytest.mark.parametrize("B,K,dims,acts,seed", MLP_CASES, ids=[f"B{c[0]}-{'x'.join(map(str, c[2]))}" for c in MLP_CASES])
def test_mlp_parity(B, K, dims, acts, seed):
    x, params = draw(B, K, dims, seed)
    margins = relu_margins(x, params, acts)
    assert min(margins) >= RELU_MARGIN, margins
    cot = torch.randn(B, K, dims[-1], generator=torch.Generator().manual_seed(1000 + seed))
    np_params = [p.numpy() for p in params]
    hs, _ = G.gt_mlp(x.numpy(), np_params, acts)
    dx, grads = G.gt_mlp_grads(x.numpy(), np_params, acts, cot.numpy())
    refs = [hs[-1], dx] + grads
    names = ["out", "dX"] + [f"{'dW' if i % 2 == 0 else 'db'}{i // 2}" for i in range(len(grads))]
    kern, eag = run_both(x, params, acts, cot)
    rows = []
    for name, k, e, ref in zip(names, kern, eag, refs):
        assert tuple(k.shape) == ref.shape and k.dtype == torch.float32
        rows.append((name, relmax(k, ref), relmax(e, ref)))
    log(f"gt_mlp M={B * K} dims {dims} (ReLU margin {min(margins):.1e}): " + ", ".join(f"{n} {ek:.2e}/{ee:.2e}" for n, ek, ee in rows))
    for name, ek, ee in rows:
        assert ek <= 4 * ee + 4 * 2.0 ** -24, (name, ek, ee)
    # two runs are the same bit for bit, and without a gradient for the input none is made
    again, _ = run_both(x, params, acts, cot)
    for name, a, b in zip(names, kern, again):
        assert torch.equal(a, b), name
    nodx, _ = run_both(x, params, acts, cot, need_dx=False)
    assert nodx[1] is None
    for name, a, b in zip(names[2:], kern[2:], nodx[2:]):
        assert torch.equal(a, b), name
    assert torch.equal(kern[0], nodx[0])


def test_mlp_rows_do_not_depend_on_their_neighbours_and_the_workspace_grows_with_m():
    import ctypes
    from ocrl_amd import _lib
    from ocrl_amd.ocrs.gt import gt_mlp
    dims, acts = [64, 64, 128], ["relu", "relu", "none"]
    x, params = draw(67, 5, dims, 3)
    ps = [p.cuda() for p in params]
    full = gt_mlp(x.cuda(), ps, acts)
    for lo, hi in ((0, 1), (3, 10), (60, 67)):                 # a row's output is its own: other batch sizes, other tiles, the same bits
        assert torch.equal(gt_mlp(x[lo:hi].cuda(), ps, acts), full[lo:hi])
    L = _lib.lib()
    sizes = [L.ocrl_gt_mlp_ws_floats(M, 5, 3, (ctypes.c_int * 3)(*dims)) for M in range(1, 400)] + \
            [L.ocrl_gt_mlp_ws_floats(M, 5, 3, (ctypes.c_int * 3)(*dims)) for M in (1000, 1024, 1025, 5000, 100000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    with pytest.raises(ValueError, match="multiple of 4"):
        gt_mlp(x.cuda(), [torch.zeros(6, 5).cuda(), torch.zeros(6).cuda()], ["relu"])
    with pytest.raises(RuntimeError, match="GPU"):
        gt_mlp(x, params, acts)


# ---------------------------------------------------------------------------------------------------------------- 3. the module
@pytest.mark.parametrize("tag", ["small", "wide", "wide_push", "short_acts"])
def test_module_reproduces_the_fixture(tag):
    from ocrl_amd import ocrs
    from tests.golden import make_golden_gt as MK
    fx = np.load(MK.FIXTURE)
    inv = json.loads(str(fx["inventory"]))[tag]
    m = ocrs.GT_Module(*MK.configs(tag))
    m.load_state_dict({k: torch.from_numpy(fx[f"{tag}:w:{k}"]) for k, _ in inv["params"]})
    m.cuda()
    acts = list(m._acts)
    params = [fx[f"{tag}:w:{k}"] for k, _ in inv["params"]]
    state, cot = fx[f"{tag}:state"], MK.cotangent(tag, fx[f"{tag}:out"].shape)
    hs, zs = G.gt_mlp(state, params, acts)
    margins = [float(np.abs(z).min() / np.abs(z).max()) for z, a in zip(zs, acts) if a == "relu"]
    assert min(margins) >= RELU_MARGIN, margins               # the maker's state seeds are chosen for this
    dx, grads = G.gt_mlp_grads(state, params, acts, cot.numpy())
    s = torch.from_numpy(state).cuda().requires_grad_(True)
    out = m(s)
    (out * cot.cuda()).sum().backward()
    got = [out, s.grad] + [p.grad for p in m._param_list()]
    fixture = [fx[f"{tag}:out"], fx[f"{tag}:dstate"]] + [fx[f"{tag}:g:{k}"] for k, _ in inv["params"]]
    refs = [hs[-1], dx] + grads
    worst = 0.0
    for g, f, r in zip(got, fixture, refs):                   # the fixture is the reference's own fp32 run: the eager side of the rule
        ek, ee = relmax(g, r), float(np.abs(f.astype(np.float64) - r).max() / np.abs(r).max())
        worst = max(worst, ek)
        assert ek <= 4 * ee + 4 * 2.0 ** -24, (tag, ek, ee)
    log(f"GT_Module [{tag}] vs fp64: worst {worst:.2e} (ReLU margins {['%.1e' % v for v in margins]})")
    assert m.rep_dim == inv["rep_dim"] and out.shape[-1] == fx[f"{tag}:out"].shape[-1]


def test_the_identity_module_returns_its_input():
    from ocrl_amd import ocrs
    c = config()
    ocr = ocrs.GT(c.ocr, c.env)
    ocr.to("cuda:0")
    x = torch.rand(3, 5, 5, device="cuda")
    assert list(ocr._module.parameters()) == [] and torch.equal(ocr(x), x) and ocr.get_loss(x) == {}
    assert torch.equal(ocr.get_loss(x, with_rep=True)[1], x)


# ---------------------------------------------------------------------------------------------------------------- 4. the extractor
POOLINGS = {
    "transformer": lambda: config().pooling,
    "transformer-push": lambda: config("pooling.push_embedding=True", "pooling.d_model=128").pooling,
    "mlp": lambda: types.SimpleNamespace(name="MLP", dims=[64, 32], acts=["relu", "relu"]),
    "rn": lambda: types.SimpleNamespace(name="RN", g_dims=[64, 64], f_dims=[64, 32]),
}


# push_embedding reads its input as a state (ids to index its embedding tables with, positions to discretise): it goes with the identity
# encoder only, and no gradient passes it
EXTRACTOR_CASES = [(p, d) for p in POOLINGS for d in ([], [8, 12]) if not (p == "transformer-push" and d)]


@pytest.mark.parametrize("pooling,dims", EXTRACTOR_CASES, ids=[f"{p}-{'x'.join(map(str, d)) or 'identity'}" for p, d in EXTRACTOR_CASES])
def test_extractor_over_every_pooling_head(pooling, dims, tmp_path):
    from ocrl_amd import envs, ocrs
    from ocrl_amd.sb3s import OCRExtractor
    c = config(*STATE, f"ocr.dims={dims}".replace(" ", ""), f"ocr.acts={['relu'] * len(dims)}".replace(" ", "").replace("'", ""), "num_envs=3")
    pc = POOLINGS[pooling]()
    cfg = types.SimpleNamespace(ocr=c.ocr, env=c.env, pooling=pc, num_envs=3, device="cuda:0")
    env = envs.TargetEnv(c.env, 3, seed=1, device="cuda")
    obs = env.reset()
    ex = OCRExtractor(env.observation_space, cfg).to("cuda:0")
    assert ex._trainable and isinstance(ex._ocr, ocrs.GT_Module) and len(list(ex._ocr.parameters())) == 2 * len(dims)
    feats = ex(obs)
    assert tuple(feats.shape) == (3, ex.features_dim) and ex.features_dim == ex._pooling.rep_dim and torch.isfinite(feats).all()
    feats.sum().backward()
    for n, p in ex.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    for n, p in ex._ocr.named_parameters():
        assert p.grad.abs().max() > 0, n
    if pooling != "transformer":
        return
    # a pre-trained checkpoint (local_file, no finetuning): the wrapper, frozen, the same features
    src = ocrs.GT(c.ocr, c.env)
    src._module.load_state_dict(ex._ocr.state_dict())
    path = str(tmp_path / "gt.pth")
    torch.save(src.save(), path)
    pc2 = config(f"pooling.ocr_checkpoint.local_file={path}").pooling
    fz = OCRExtractor(env.observation_space, types.SimpleNamespace(ocr=c.ocr, env=c.env, pooling=pc2, num_envs=3, device="cuda:0")).to("cuda:0")
    assert not fz._trainable and isinstance(fz._ocr, ocrs.GT) and not any(n.startswith("_ocr") for n, _ in fz.named_parameters())
    fz._pooling.load_state_dict(ex._pooling.state_dict())
    ex.eval(), fz.eval()
    with torch.no_grad():
        assert torch.equal(fz(obs), ex(obs))


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("algo,over,steps", [("ppo", ["sb3.algo_kwargs.n_steps=32", "max_steps=64", "eval.freq=32"], [32, 64]),
                                             ("a2c", ["max_steps=8", "eval.freq=4"], [4, 8])])
def test_train_sb3_end_to_end(algo, over, steps, tmp_path):
    import train_sb3
    args = ["ocr=gt", "pooling=transformer", f"sb3={algo}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "device=cuda:0", "num_envs=4",
            "eval.n_episodes=4", "env.max_steps=6", "env.rew_type=dense"] + over
    finals = []
    for run in ("a", "b"):
        model = train_sb3.main(args + [f"run_dir={tmp_path / run}"])
        assert model.env.render_mode == "state" and tuple(model.env.observation_space.shape) == (5, 5)
        finals.append(model.flat_p.clone())
    assert torch.equal(finals[0], finals[1]) and torch.isfinite(finals[0]).all()
    lines = [json.loads(l) for l in open(tmp_path / "a" / "metrics.jsonl")]
    assert [l["step"] for l in lines] == steps and [l["iteration"] for l in lines] == [1, 2]
    for l in lines:
        for k in ("train/loss", "eval/success_rate", "eval/mean_reward", "eval/mean_ep_length"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
        assert 0 <= l["eval/success_rate"] <= 1
    _, _, fresh = train_sb3.build(compose(CFG, "train_sb3", args + ["seed=7"]))
    assert type(fresh).__name__ == algo.upper() and not torch.equal(fresh.flat_p, finals[0])
    for name in ("model_latest.pth", "model_best.pth"):
        fresh.load(str(tmp_path / "a" / "checkpoints" / name))
        assert fresh.num_timesteps in steps and torch.isfinite(fresh.flat_p).all()
    fresh.load(str(tmp_path / "a" / "checkpoints" / "model_latest.pth"))
    assert torch.equal(fresh.flat_p, finals[0])
