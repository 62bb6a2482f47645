"""GPU checks of the sprite environment (ocrl_sprite_env_*, ocrl_sprite_render, ocrl_amd.envs.TargetEnv), of PPO's on-device rollout path
and of train_sb3.py, against the numpy restatement of tests/sprite_env_ref.py.

Bounds.  States, rewards, dones, episode returns and lengths: exact (the restatement follows the kernel's fp32 operations one rounding
at a time and is fed the very uniforms the kernel drew, ocrl_sprite_env_uniforms).  Frames: byte for byte against the fp32 restatement,
except pixels whose float64 decision margin to some sprite's edge is below 1e-5 (two correct fp32 evaluations may order the operations
of a predicate differently there); those are left out and must be at most 0.1 % of the pixels compared."""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from ocrl_amd.utils.config import compose
from tests import sprite_env_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
BASE = ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "env=target-N4C4S3S1", "device=cuda:0"]
F = np.float32


def config(*over):
    return compose(CFG, "train_sb3", BASE + list(over))


def make(E, seed=0, *over):
    from ocrl_amd import envs
    return envs.TargetEnv(config(*over).env, E, seed=seed, device="cuda")


def dump(seed, env0, n_envs, episode, n=1024):
    from ocrl_amd.envs import sprite_env_uniforms
    u = sprite_env_uniforms(seed, env0, n_envs, episode, 0, n).cpu().numpy()
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    return u


def ref_reset(s, seed, e, k, u=None):
    """the restatement's episode k of environment e from the dumped uniforms (a longer dump when the first 1024 do not suffice)"""
    try:
        return R.reset(s, dump(seed, e, 1, k)[0] if u is None else u)
    except IndexError:
        return R.reset(s, dump(seed, e, 1, k, 80000)[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. the renderer
def hand_rows(e, R_rows=16):
    """rows [16, 5] of hand-placed sprites; e picks the kind: agent alone, one object, up to 15 objects with padding rows and a -1 colour,
    overlaps, sprites cut by the frame edge"""
    rs = np.random.RandomState(100 + e)
    rows = np.zeros((R_rows, 5), dtype=np.float32)
    kind = e % 5
    agent = (3, 3, 0.15, rs.uniform(0.075, 0.925), rs.uniform(0.075, 0.925))
    if kind == 0:
        rows[0] = agent
    elif kind == 1:
        rows[0] = (rs.randint(7), rs.randint(4), (0.15, 0.22)[rs.randint(2)], rs.uniform(0.2, 0.8), rs.uniform(0.2, 0.8))
        rows[1] = agent
    elif kind == 2:
        n = 15 if e % 10 == 2 else rs.randint(9, 15)
        for i in range(n):
            rows[i] = (rs.randint(7), rs.randint(4), (0.15, 0.22)[rs.randint(2)], rs.uniform(0, 1), rs.uniform(0, 1))
        rows[rs.randint(n), 0] = -1
        rows[n] = agent
    elif kind == 3:
        cx, cy = rs.uniform(0.3, 0.7, size=2)
        for i in range(4):
            rows[i] = (i, (i + e) % 4, 0.22 if i < 2 else 0.15, cx + rs.uniform(-0.03, 0.03), cy + rs.uniform(-0.03, 0.03))
        rows[4] = (3, 3, 0.15, cx, cy)
    else:
        spots = [(0.0, 0.0), (1.0, 1.0), (0.0, 0.5), (0.5, 1.0), (1.0, 0.02), (0.98, 0.5)]
        for i, (x, y) in enumerate(spots):
            rows[i] = (4 + i % 3, (i + e) % 4, 0.22, x, y)
        rows[len(spots)] = (3, 3, 0.15, 0.075, 0.925)
    return rows


@pytest.mark.parametrize("H", [16, 36, 64])
@pytest.mark.parametrize("E", [1, 5, 67])
def test_render_equals_the_restatement(E, H):
    env = make(1, 0, f"env.obs_size={H}")
    rows = np.stack([hand_rows(e if E > 1 else 2) for e in range(E)])
    dev = torch.from_numpy(rows)
    chw, hwc, masks = (env.render_rows(dev, m).cpu().numpy() for m in ("image", "rgb_array", "mask"))
    assert chw.shape == (E, 3, H, H) and hwc.shape == (E, H, H, 3) and masks.shape == (E, 17, H, H, 1)
    assert np.array_equal(chw, hwc.transpose(0, 3, 1, 2))
    left_out = 0
    for e in range(E):
        img, msk, marg = R.render(rows[e], H, np.float32, with_margin=True)
        sure = marg >= 1e-5
        left_out += int((~sure).sum())
        assert np.array_equal(hwc[e][sure], img[sure]), e
        assert np.array_equal(masks[e][:, sure], msk[:, sure]), e
    share = left_out / (E * H * H)
    log(f"render E{E} H{H}: {left_out} of {E * H * H} pixels within 1e-5 of an edge ({share:.2e})")
    assert share <= 1e-3
    assert masks.max() == 1 and (masks[:, :-1].sum(1) + masks[:, -1] >= 1).all()
    if E == 67:                                                       # every kind drew something, and the -1 row nothing
        assert all(hwc[e].any() for e in range(E))
        e2 = 2
        skipped = int(np.nonzero(rows[e2, :, 0] == -1)[0][0])
        assert not masks[e2, skipped].any()


def test_render_of_the_environments_own_state_and_modes():
    env = make(5, 3)
    obs = env.reset()
    assert obs.dtype == torch.uint8 and tuple(obs.shape) == (5, 3, 64, 64) and obs.is_cuda
    state = env.render("state")
    assert tuple(state.shape) == (5, 5, 5) and torch.equal(state, env.get_state()["rows"])
    assert torch.equal(env.render("image"), obs) and torch.equal(env.render("rgb_array").permute(0, 3, 1, 2), obs)
    masks = env.render("mask")
    assert tuple(masks.shape) == (5, 6, 64, 64, 1) and (masks.sum(1) == 1).all()       # sprites kept apart: the masks partition the frame
    colours = {tuple(c) for c in obs.permute(0, 2, 3, 1).reshape(-1, 3).cpu().tolist()}
    assert colours <= {(0, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0)} and (255, 0, 0) in colours
    with pytest.raises(ValueError, match="render mode"):
        env.render("video")


# ---------------------------------------------------------------------------------------------------------------- 2. reset
RESET_CASES = [("easy", False, 4, 4), ("normal", False, 4, 4), ("hard", False, 4, 4), ("hard", True, 4, 4), ("normal", True, 4, 4), ("hard", True, 1, 9)]


@pytest.mark.parametrize("E", [1, 3, 64, 130])
@pytest.mark.parametrize("mode,occlusion,lo,hi", RESET_CASES, ids=[f"{m}-{'occl' if o else 'apart'}-{a}{b}" for m, o, a, b in RESET_CASES])
def test_reset_equals_the_restatement_and_respects_the_task(mode, occlusion, lo, hi, E):
    seed = 11 + E
    env = make(E, seed, f"env.mode={mode}", f"env.occlusion={occlusion}", f"env.num_objects_range=[{lo},{hi}]")
    env.reset()
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    s = R.spec_from_desc(env._desc)
    u = dump(seed, 0, E, 0)
    worst = 0
    for e in range(E):
        rows, n, target, used = ref_reset(s, seed, e, 0, u[e])
        worst = max(worst, used)
        assert np.array_equal(bits(st["rows"][e]), bits(rows)), (e, st["rows"][e], rows)
        assert (st["n"][e], st["target"][e], st["step_count"][e], st["episode"][e], st["episode_length"][e]) == (n, target, 0, 0, 0)
        assert st["episode_return"][e] == 0.0
    log(f"reset {mode} occlusion={occlusion} [{lo},{hi}] E{E}: at most {worst} draws per episode")
    # independently of the restatement
    thr_o, thr_a = (0.15, 0.15) if occlusion else (0.15 + 0.08, 0.15 + 0.08)
    for e in range(E):
        q, n = st["rows"][e].astype(np.float64), int(st["n"][e])
        assert lo <= n <= hi and tuple(q[n]) == (3.0, 3.0, float(F(0.15)), 0.5, 0.5) and not q[n + 1:].any()
        is_target = [(q[i, 0], q[i, 1], F(q[i, 2])) == (0.0, 0.0, F(0.15)) for i in range(n)]
        assert is_target == [i == st["target"][e] for i in range(n)]
        assert set(q[:n, 0]) <= {0.0, 1.0, 2.0, 3.0} and set(q[:n, 1]) <= {0.0, 1.0, 2.0}
        for i in range(n):
            b = [float(v) for v in R.box(s.mode, n, i)]
            pad = 0.0 if mode == "easy" else 0.075 + 0.08
            assert b[0] + pad - 1e-6 <= q[i, 3] <= b[1] - pad + 1e-6 and b[2] + pad - 1e-6 <= q[i, 4] <= b[3] - pad + 1e-6, (e, i, q[i])
            assert math.hypot(q[i, 3] - 0.5, q[i, 4] - 0.5) >= thr_a - 1e-6
            for j in range(i):
                assert math.hypot(q[i, 3] - q[j, 3], q[i, 4] - q[j, 4]) >= thr_o - 1e-6
    if hi > lo and E >= 64:
        assert len(set(st["n"].tolist())) >= 5


# ---------------------------------------------------------------------------------------------------------------- 3. streams
def test_streams_depend_on_seed_environment_and_episode_only():
    def episodes(E, seed, k=3):
        env = make(E, seed)
        out = []
        for _ in range(k):
            env.reset()
            out.append(env.get_state())
        return out
    small, big, again, other = episodes(3, 5), episodes(64, 5), episodes(64, 5), episodes(64, 6)
    for k in range(3):
        assert (small[k]["episode"] == k).all() and (big[k]["episode"] == k).all()
        for key in ("rows", "n", "target"):
            assert torch.equal(small[k][key], big[k][key][:3]), (k, key)
            assert torch.equal(big[k][key], again[k][key]), (k, key)
        assert not torch.equal(big[k]["rows"], other[k]["rows"])
    assert not torch.equal(big[0]["rows"], big[1]["rows"]) and not torch.equal(big[0]["rows"][0], big[0]["rows"][1])
    # a masked reset moves the selected environments on and leaves the others alone
    env = make(4, 5)
    env.reset()
    before = env.get_state()
    env.reset(mask=[0, 1, 0, 1])
    after = env.get_state()
    assert after["episode"].tolist() == [0, 1, 0, 1]
    assert torch.equal(after["rows"][0::2], before["rows"][0::2]) and torch.equal(after["rows"][1], big[1]["rows"][1])
    u = dump(5, 2, 2, 1, 8)
    assert np.array_equal(u[1], dump(5, 3, 1, 1, 8)[0]) and not np.array_equal(u[0], u[1])


# ---------------------------------------------------------------------------------------------------------------- 4. step
def scripted_layouts():
    """rows [4, 5, 5] (n = 2 objects, the agent in row 2) whose first steps hit the target, a non-target, a wall and the time-out"""
    z = F(0.15)
    rows = np.zeros((4, 5, 5), dtype=np.float32)
    for e, (t_xy, o_xy, a_xy) in enumerate((((0.5, 0.72), (0.1, 0.1), (0.5, 0.5)), ((0.1, 0.1), (0.72, 0.5), (0.5, 0.5)),
                                            ((0.8, 0.8), (0.8, 0.2), (0.1, 0.1)), ((0.1, 0.9), (0.9, 0.1), (0.5, 0.5)))):
        rows[e, 0] = (0, 0, z, *t_xy)
        rows[e, 1] = (1, 1, z, *o_xy)
        rows[e, 2] = (3, 3, z, *a_xy)
    script = np.array([[0, 3, 1, 0], [0, 3, 1, 2], [0, 3, 2, 0], [1, 1, 2, 2], [1, 1, 1, 0], [2, 2, 2, 2], [3, 3, 1, 0]])
    return rows, script


@pytest.mark.parametrize("rew_type", ["sparse", "normal", "dense"])
def test_forty_scripted_steps_equal_the_restatement(rew_type):
    E, seed, T = 5, 21, 40
    env = make(E, seed, "env.max_steps=7", f"env.rew_type={rew_type}")
    env.reset()
    s = R.spec_from_desc(env._desc)
    cache = {}

    def uniforms_of(e):
        def get(k):
            if k not in cache:
                cache[k] = dump(seed, 0, E, k, 4096)
            return cache[k][e]
        return get
    refs = [R.Env(s, uniforms_of(e)) for e in range(E)]
    rows, script = scripted_layouts()
    st = env.get_state()
    st["rows"][:4] = torch.from_numpy(rows).cuda()
    st["n"][:4], st["target"][:4] = 2, 0
    env.set_state(rows=st["rows"], n=st["n"], target=st["target"])
    for e in range(4):
        refs[e].rows, refs[e].n, refs[e].target = rows[e].copy(), 2, 0
    rs = np.random.RandomState(7)
    seen = dict(target=0, other=0, timeout=0, wall=0)
    for t in range(T):
        actions = rs.randint(0, 4, size=E)
        if t < len(script):
            actions[:4] = script[t]
        obs, rewards, dones, infos = env.step(actions if t % 2 else torch.from_numpy(actions).cuda())
        got = {k: v.cpu().numpy() for k, v in env.get_state().items()}
        assert rewards.dtype == np.float32 and dones.dtype == bool and obs.is_cuda and tuple(obs.shape) == (E, 3, 64, 64)
        for e in range(E):
            reward, done, success, ret, length = refs[e].step(int(actions[e]))
            assert (rewards[e], dones[e], infos[e]["is_success"]) == (reward, done, success), (t, e, rewards[e], reward)
            assert infos[e].get("episode") == ({"r": ret, "l": length} if done else None), (t, e)
            assert np.array_equal(bits(got["rows"][e]), bits(refs[e].rows)), (t, e)
            assert (got["n"][e], got["target"][e], got["step_count"][e], got["episode"][e], got["episode_length"][e]) == \
                   (refs[e].n, refs[e].target, refs[e].step_count, refs[e].episode, refs[e].ep_length), (t, e)
            assert got["episode_return"][e] == refs[e].ep_return
            seen["target"] += success
            seen["other"] += done and not success and length < 7
            seen["timeout"] += done and length == 7
            q = refs[e].rows[refs[e].n]
            seen["wall"] += bool(q[3] == F(0.075) or q[4] == F(0.075))
        if t == T - 1:
            assert torch.equal(obs, env.render("image"))
    log(f"step {rew_type}: {seen}")
    assert seen["target"] >= 1 and seen["other"] >= 1 and seen["timeout"] >= 1 and seen["wall"] >= 1
    before = env.get_state()
    for bad in ([0, 1, 2, 3, 4], [0, -1, 0, 0, 0]):
        with pytest.raises(ValueError, match="action must be one of"):
            env.step(np.array(bad))
    after = env.get_state()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # the library itself leaves the agent where it is for such an action (the restatement's rule)
    _, _, _, _ = env.step_device(torch.tensor([9, -3, 4, 2 ** 40, 7], device="cuda"))
    moved = env.get_state()
    for e in range(E):
        refs[e].step(9)
        assert np.array_equal(bits(moved["rows"][e].cpu().numpy()), bits(refs[e].rows)), e


# ---------------------------------------------------------------------------------------------------------------- 5. PPO
class HostView:
    """the same environment without ``on_device``: PPO then takes its host path through ``step``"""

    def __init__(self, env):
        self.env, self.num_envs, self.observation_space, self.action_space = env, env.num_envs, env.observation_space, env.action_space

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        return self.env.step(actions)


def test_ppo_device_path_fills_the_buffers_of_the_host_path():
    from ocrl_amd.sb3s import PPO, CustomActorCriticPolicy
    from tests.test_gpu_acnet import _acnet_cfg

    def build(host):
        env = make(4, 31, "env.obs_size=16", "env.max_steps=5", "env.rew_type=dense")
        kw = dict(n_steps=8, batch_size=8, n_epochs=1, seed=13, learning_rate=1e-3, ent_coef=0.01,
                  policy_kwargs=dict(config=types.SimpleNamespace(sb3_acnet=_acnet_cfg("mlp"))))
        return PPO(CustomActorCriticPolicy, HostView(env) if host else env, **kw)
    dev, host = build(False), build(True)
    assert getattr(dev.env, "on_device", False) and not getattr(host.env, "on_device", False)
    for it in range(2):
        a, b = dev.collect_rollouts(), host.collect_rollouts()
        for k in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (it, k)
        assert a.observations.dtype == torch.uint8 and a.observations.any() and a.rewards.abs().max() > 0
        assert list(dev._episodes) == list(host._episodes) and len(dev._episodes) >= 4 * (it + 1)
        assert dev.num_timesteps == host.num_timesteps == 32 * (it + 1)
        sa, sb = dev.train(), host.train()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert sa[k] == sb[k] or (math.isnan(sa[k]) and math.isnan(sb[k])), (it, k, sa[k], sb[k])
        assert torch.equal(dev.flat_p, host.flat_p)
    assert len(dev._successes) == len(dev._episodes) and 0.0 <= dev.success_rate <= 1.0
    assert math.isnan(host.success_rate)                              # the host path is as it was: it does not read is_success
    log(f"ppo device path: {len(dev._episodes)} episodes, ep_rew_mean {dev.ep_rew_mean:.3f}, success_rate {dev.success_rate:.2f}")


# ---------------------------------------------------------------------------------------------------------------- 6. the entry point
SMOKE_SLATE = ["ocr.dvae.vocab_size=256", "ocr.slotattr.num_slots=6", "ocr.slotattr.num_iterations=3", "ocr.tfdec.num_dec_blocks=2", "env.obs_size=16"]


def test_train_sb3_runs_end_to_end_in_a_child_process(tmp_path):
    from ocrl_amd import ocrs
    over = SMOKE_SLATE + ["num_envs=4", "max_steps=64", "sb3.algo_kwargs.n_steps=32", "eval.freq=32", "eval.n_episodes=4", "env.max_steps=6",
                          "env.rew_type=dense", f"run_dir={tmp_path / 'run'}"]
    c = config(*over)
    src = ocrs.SLATE(c.ocr, c.env)
    src.to("cuda:0")
    ckpt = str(tmp_path / "slate.pth")
    torch.save(src.save(), ckpt)
    over.append(f"pooling.ocr_checkpoint.local_file={ckpt}")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_sb3.py")] + BASE + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert [l["step"] for l in lines] == [32, 64] and [l["iteration"] for l in lines] == [1, 2]
    for l in lines:
        for k in ("train/loss", "train/policy_loss", "train/value_loss", "train/approx_kl", "train/explained_variance", "rollout/ep_rew_mean",
                  "rollout/success_rate", "eval/success_rate", "eval/mean_reward", "eval/mean_ep_length"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
        assert 0 <= l["eval/success_rate"] <= 1 and 1 <= l["eval/mean_ep_length"] <= 6
    import train_sb3
    _, _, model = train_sb3.build(config(*over))
    start = model.flat_p.clone()
    for name in ("model_latest.pth", "model_best.pth"):
        model.flat_p.copy_(start)
        model.load(str(tmp_path / "run" / "checkpoints" / name))
        assert model.num_timesteps in (32, 64) and model.adam_step > 0 and not torch.equal(model.flat_p, start)
        assert torch.isfinite(model.flat_p).all()
