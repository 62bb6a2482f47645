"""GPU checks of the Odd-One-Out task (ocrl_sprite_env_* with task 1, ocrl_amd.envs.OddOneOutEnv), of PPO's rollout on it and of
train_sb3.py / test_sb3.py on the unseen-combination pair, against the numpy restatement of tests/oddoneout_ref.py.

Bounds.  States, unique kinds, rewards, dones, episode returns and lengths: exact (the restatement follows the kernel's fp32 operations one
rounding at a time and is fed the very uniforms the kernel drew, ocrl_sprite_env_uniforms).  Frames: byte for byte against the fp32
restatement of the renderer, except pixels whose float64 decision margin to some sprite's edge is below 1e-5 (two correct fp32 evaluations
may order the operations of a predicate differently there); those are left out and must be at most 0.1 % of the pixels compared.

Shapes.  The crowded cases ([3, 9], 7 and 15 objects) are placed with ``occlusion`` (one 0.15 threshold), the 15 also without a wall
distance: kept apart, 15 sprites need some 10 000 position draws an episode, which the restatement takes a third of a second per
environment to follow; the properties, which this file is about, draw the same either way."""
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
from tests import oddoneout_ref as O
from tests import sprite_env_ref as R
from tests.gpu_util import log
from tests.test_oddoneout_cpu import CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
BASE = ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "device=cuda:0"]
F = np.float32
COLOURS = ["blue", "green", "yellow", "red", "cyan", "pink", "brown"]
SHAPE_NAMES = ["square", "triangle", "star_4", "circle"]
PLACING = {"N3-9C4S4S2": ["env.occlusion=True"], "N7C3S1S1": ["env.occlusion=True"], "N15C7S4S2": ["env.occlusion=True", "env.distance_to_wall=0.0"]}


def config(env, *over):
    return compose(CFG, "train_sb3", BASE + [f"env={env}"] + list(over))


def case_overrides(name):
    """the overrides that turn configs/env/odd-one-out-N4C2S2S1.yaml into a case of tests/test_oddoneout_cpu.py"""
    kw = dict(lo=4, hi=4, colors=(0, 1), shapes=(0, 1), scales=(0.15,), obj_comp=False, unseen_mode=None, unseen_colors=(0, 0))
    kw.update(CASES[name])
    over = [f"env.num_objects_range=[{kw['lo']},{kw['hi']}]", "env.COLORS=[" + ",".join(COLOURS[c] for c in kw["colors"]) + "]",
            "env.SHAPES=[" + ",".join(SHAPE_NAMES[h] for h in kw["shapes"]) + "]", "env.SCALES=[" + ",".join(str(z) for z in kw["scales"]) + "]",
            f"env.obj_comp={kw['obj_comp']}"]
    if kw["unseen_mode"]:
        over += [f"env.unseen_combi_mode={kw['unseen_mode']}", "env.unseen_combi=[" + ",".join(COLOURS[c] for c in kw["unseen_colors"]) + "]"]
    return over + PLACING.get(name, [])


def make(E, seed=0, *over, env="odd-one-out-N4C2S2S1"):
    from ocrl_amd import envs
    return envs.OddOneOutEnv(config(env, *over).env, E, seed=seed, device="cuda")


def dump(seed, env0, n_envs, episode, n=1024):
    from ocrl_amd.envs import sprite_env_uniforms
    return sprite_env_uniforms(seed, env0, n_envs, episode, 0, n).cpu().numpy()


def ref_reset(s, seed, e, k, u=None):
    """the restatement's episode k of environment e from the dumped uniforms (a longer dump when the first 1024 do not suffice)"""
    try:
        return O.reset(s, dump(seed, e, 1, k)[0] if u is None else u)
    except IndexError:
        return O.reset(s, dump(seed, e, 1, k, 80000)[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(state):
    return {k: v.cpu().numpy() for k, v in state.items()}


AUX = ("n", "target", "unique_kind", "step_count", "episode", "episode_length")


# ---------------------------------------------------------------------------------------------------------------- 1. reset
@pytest.mark.parametrize("E", [1, 3, 64, 130])
@pytest.mark.parametrize("case", list(CASES))
def test_reset_equals_the_restatement_and_respects_the_task(case, E):
    seed = 11 + E
    env = make(E, seed, *case_overrides(case))
    obs = env.reset()
    assert tuple(obs.shape) == (E, 3, 64, 64) and obs.dtype == torch.uint8
    st = host(env.get_state())
    assert set(st) == {"rows", "episode_return"} | set(AUX)
    s = O.spec_from_desc(env._desc)
    want = O.spec(**CASES[case])
    assert (s.lo, s.hi, s.colors, s.shapes, s.scales, s.obj_comp, s.unseen_mode) == \
           (want.lo, want.hi, want.colors, want.shapes, want.scales, want.obj_comp, want.unseen_mode)
    assert not s.unseen_mode or s.unseen_colors == want.unseen_colors
    u = dump(seed, 0, E, 0)
    worst = 0
    for e in range(E):
        rows, n, target, kind, used = ref_reset(s, seed, e, 0, u[e])
        worst = max(worst, used)
        assert np.array_equal(bits(st["rows"][e]), bits(rows)), (e, st["rows"][e], rows)
        assert tuple(st[k][e] for k in AUX) == (n, target, kind, 0, 0, 0), e
        assert st["episode_return"][e] == 0.0
    log(f"odd-one-out reset {case} E{E}: at most {worst} draws per episode")
    # independently of the restatement: the task's invariants on the device state
    kinds = set()
    for e in range(E):
        q, n = st["rows"][e], int(st["n"][e])
        O.check_episode(want, q, n, int(st["target"][e]), int(st["unique_kind"][e]))
        kinds.add(int(st["unique_kind"][e]))
        assert tuple(q[n]) == (3.0, 3.0, F(0.15), 0.5, 0.5) and not q[n + 1:].any()
        thr = 0.15 if s.occlusion else None
        for i in range(n):
            pad = float(q[i, 2]) / 2 + float(s.dist_wall)
            assert pad - 1e-6 <= q[i, 3] <= 1 - pad + 1e-6 and pad - 1e-6 <= q[i, 4] <= 1 - pad + 1e-6, (e, i, q[i])
            assert math.hypot(q[i, 3] - 0.5, q[i, 4] - 0.5) >= (thr or float(q[i, 2]) / 2 + 0.075 + 0.08) - 1e-6
            for j in range(i):
                assert math.hypot(q[i, 3] - q[j, 3], q[i, 4] - q[j, 4]) >= (thr or float(q[i, 2] + q[j, 2]) / 2 + 0.08) - 1e-6
    if E >= 64:
        assert kinds == {K for K, l in enumerate((want.colors, want.shapes, want.scales)) if len(l) > 1}
        assert want.hi == want.lo or len(set(st["n"].tolist())) >= 5


# ---------------------------------------------------------------------------------------------------------------- 2. step and auto-reset
def scripted_layouts():
    """rows [4, 5, 5] (n = 3 objects: the odd one by colour, two others; the agent in row 3) whose first steps reach the odd object, another
    one, a wall and the time-out"""
    z = F(0.15)
    rows = np.zeros((4, 5, 5), dtype=np.float32)
    for e, (t_xy, o_xy, p_xy, a_xy) in enumerate((((0.5, 0.72), (0.1, 0.1), (0.9, 0.9), (0.5, 0.5)), ((0.1, 0.1), (0.72, 0.5), (0.1, 0.9), (0.5, 0.5)),
                                                  ((0.8, 0.8), (0.8, 0.2), (0.2, 0.8), (0.1, 0.1)), ((0.1, 0.9), (0.9, 0.1), (0.9, 0.9), (0.5, 0.5)))):
        rows[e, 0] = (0, 0, z, *t_xy)
        rows[e, 1] = (1, 0, z, *o_xy)
        rows[e, 2] = (1, 0, z, *p_xy)
        rows[e, 3] = (3, 3, z, *a_xy)
    script = np.array([[0, 3, 1, 0], [0, 3, 1, 2], [0, 3, 2, 0], [1, 1, 2, 2], [1, 1, 1, 0], [2, 2, 2, 2], [3, 3, 1, 0]])
    return rows, script


@pytest.mark.parametrize("rew_type", ["normal", "dense"])
def test_forty_steps_equal_the_restatement(rew_type):
    E, seed, T = 5, 21, 40
    env = make(E, seed, "env.max_steps=7", f"env.rew_type={rew_type}")
    env.reset()
    s = O.spec_from_desc(env._desc)
    cache = {}

    def uniforms_of(e):
        def get(k):
            if k not in cache:
                cache[k] = dump(seed, 0, E, k, 4096)
            return cache[k][e]
        return get
    refs = [O.Env(s, uniforms_of(e)) for e in range(E)]
    rows, script = scripted_layouts()
    st = env.get_state()
    st["rows"][:4] = torch.from_numpy(rows).cuda()
    st["n"][:4], st["target"][:4], st["unique_kind"][:4] = 3, 0, 0
    env.set_state(rows=st["rows"], n=st["n"], target=st["target"], unique_kind=st["unique_kind"])
    for e in range(4):
        refs[e].rows, refs[e].n, refs[e].target, refs[e].unique_kind = rows[e].copy(), 3, 0, 0
    rs = np.random.RandomState(7)
    seen = dict(odd=0, other=0, timeout=0, wall=0)
    first = {}
    for t in range(T):
        actions = rs.randint(0, 4, size=E)
        if t < len(script):
            actions[:4] = script[t]
        obs, rewards, dones, infos = env.step(actions if t % 2 else torch.from_numpy(actions).cuda())
        got = host(env.get_state())
        assert rewards.dtype == np.float32 and dones.dtype == bool and obs.is_cuda and tuple(obs.shape) == (E, 3, 64, 64)
        for e in range(E):
            reward, done, success, ret, length = refs[e].step(int(actions[e]))
            assert (rewards[e], dones[e], infos[e]["is_success"]) == (reward, done, success), (t, e, rewards[e], reward)
            assert infos[e].get("episode") == ({"r": ret, "l": length} if done else None), (t, e)
            assert np.array_equal(bits(got["rows"][e]), bits(refs[e].rows)), (t, e)
            assert tuple(got[k][e] for k in AUX) == (refs[e].n, refs[e].target, refs[e].unique_kind, refs[e].step_count, refs[e].episode,
                                                     refs[e].ep_length), (t, e)
            assert got["episode_return"][e] == refs[e].ep_return
            if done:                                                  # the rows now are the next Odd-One-Out episode of this stream
                O.check_episode(s, got["rows"][e], int(got["n"][e]), int(got["target"][e]), int(got["unique_kind"][e]))
                nxt = ref_reset(s, seed, e, int(got["episode"][e]))
                assert np.array_equal(bits(got["rows"][e]), bits(nxt[0])) and got["n"][e] >= 3
            if done and e < 4 and e not in first:
                first[e] = (float(reward), bool(success), int(length))
            seen["odd"] += success
            seen["other"] += done and not success and length < 7
            seen["timeout"] += done and length == 7
            q = refs[e].rows[refs[e].n]
            seen["wall"] += bool(q[3] == F(0.075) or q[4] == F(0.075))
        if t == T - 1:
            assert torch.equal(obs, env.render("image"))
    log(f"odd-one-out step {rew_type}: {seen}, scripted {first}")
    assert first[0] == (1.0, True, 2) and first[1] == (float(F(0.1)) if rew_type == "normal" else 0.0, False, 2) and first[3][1:] == (False, 7)
    assert seen["odd"] >= 1 and seen["other"] >= 1 and seen["timeout"] >= 1 and seen["wall"] >= 1


# ---------------------------------------------------------------------------------------------------------------- 3. streams
def test_streams_depend_on_seed_environment_and_episode_only():
    def episodes(E, seed, k=3):
        env = make(E, seed)
        out = []
        for _ in range(k):
            env.reset()
            out.append(env.get_state())
        return out
    small, big, other = episodes(3, 5), episodes(64, 5), episodes(64, 6)
    for k in range(3):
        assert (small[k]["episode"] == k).all() and (big[k]["episode"] == k).all()
        for key in ("rows", "n", "target", "unique_kind"):
            assert torch.equal(small[k][key], big[k][key][:3]), (k, key)
        assert not torch.equal(big[k]["rows"], other[k]["rows"])
    assert not torch.equal(big[0]["rows"], big[1]["rows"]) and not torch.equal(big[0]["rows"][0], big[0]["rows"][1])


def test_both_tasks_in_one_process_each_equal_their_own_restatement():
    from ocrl_amd import envs
    seed, E = 9, 3
    odd = make(E, seed)
    tgt = envs.TargetEnv(config("target-N4C4S3S1").env, E, seed=seed, device="cuda")
    so, stt = O.spec_from_desc(odd._desc), R.spec_from_desc(tgt._desc)
    for k in range(2):                                                  # interleaved: odd, target, odd, target
        odd.reset()
        tgt.reset()
        go, gt = host(odd.get_state()), host(tgt.get_state())
        assert set(gt) == {"rows", "episode_return", "n", "target", "step_count", "episode", "episode_length"}
        u = dump(seed, 0, E, k)
        for e in range(E):
            rows, n, target, kind, _ = O.reset(so, u[e])
            assert np.array_equal(bits(go["rows"][e]), bits(rows)) and (go["n"][e], go["target"][e], go["unique_kind"][e], go["episode"][e]) == (n, target, kind, k)
            rows, n, target, _ = R.reset(stt, u[e])
            assert np.array_equal(bits(gt["rows"][e]), bits(rows)) and (gt["n"][e], gt["target"][e], gt["episode"][e]) == (n, target, k)
    assert (tgt._aux[:, 5] == 0).all()                                  # aux word 5 stays 0 for the Target task


# ---------------------------------------------------------------------------------------------------------------- 4. frames
def test_reset_frames_equal_the_restated_renderer():
    E, H = 8, 64
    env = make(E, 3, env="odd-one-out-N4C2S2S2")
    obs = env.reset()
    rows = env.get_state()["rows"].cpu().numpy()
    hwc, masks = env.render("rgb_array").cpu().numpy(), env.render("mask").cpu().numpy()
    assert np.array_equal(obs.cpu().numpy(), hwc.transpose(0, 3, 1, 2)) and masks.shape == (E, 6, H, H, 1)
    assert {F(0.15), F(0.22)} == set(rows[:, :4, 2].reshape(-1).tolist())            # both scales are drawn
    left_out = 0
    for e in range(E):
        img, msk, marg = R.render(rows[e], H, np.float32, with_margin=True)
        sure = marg >= 1e-5
        left_out += int((~sure).sum())
        assert np.array_equal(hwc[e][sure], img[sure]), e
        assert np.array_equal(masks[e][:, sure], msk[:, sure]), e
    log(f"odd-one-out frames: {left_out} of {E * H * H} pixels within 1e-5 of an edge")
    assert left_out / (E * H * H) <= 1e-3
    assert (masks.sum(1) == 1).all()                                    # sprites kept apart: the masks partition the frame


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

    def build(as_host):
        env = make(4, 31, "env.obs_size=16", "env.max_steps=5", "env.rew_type=dense")
        kw = dict(n_steps=8, batch_size=8, n_epochs=1, seed=13, learning_rate=1e-3, ent_coef=0.01,
                  policy_kwargs=dict(config=types.SimpleNamespace(sb3_acnet=_acnet_cfg("mlp"))))
        return PPO(CustomActorCriticPolicy, HostView(env) if as_host else env, **kw)
    dev, hst = build(False), build(True)
    assert getattr(dev.env, "on_device", False) and not getattr(hst.env, "on_device", False)
    for it in range(2):
        a, b = dev.collect_rollouts(), hst.collect_rollouts()
        for k in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (it, k)
        assert a.observations.dtype == torch.uint8 and a.observations.any() and a.rewards.abs().max() > 0
        assert list(dev._episodes) == list(hst._episodes) and len(dev._episodes) >= 4 * (it + 1)
        assert dev.num_timesteps == hst.num_timesteps == 32 * (it + 1)
        dev.train(), hst.train()
        assert torch.equal(dev.flat_p, hst.flat_p)
    assert 0.0 <= dev.success_rate <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 6. the entry points
SMOKE_SLATE = ["ocr.dvae.vocab_size=256", "ocr.slotattr.num_slots=6", "ocr.slotattr.num_iterations=3", "ocr.tfdec.num_dec_blocks=2", "env.obs_size=16"]


def test_train_on_the_unseen_combination_train_side_then_test_sb3_on_the_test_side(tmp_path):
    from ocrl_amd import ocrs
    train_env, test_env = "odd-one-out-N4C3S1S1-ood-unseen-combi-train1", "odd-one-out-N4C3S1S1-ood-unseen-combi-test1"
    shared = SMOKE_SLATE + ["num_envs=4", "env.max_steps=6", "env.rew_type=dense"]
    c = config(train_env, *shared)
    src = ocrs.SLATE(c.ocr, c.env)
    src.to("cuda:0")
    ckpt = str(tmp_path / "slate.pth")
    torch.save(src.save(), ckpt)
    shared.append(f"pooling.ocr_checkpoint.local_file={ckpt}")
    over = shared + ["max_steps=64", "sb3.algo_kwargs.n_steps=32", "eval.freq=32", "eval.n_episodes=4", f"run_dir={tmp_path / 'run'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_sb3.py")] + BASE + [f"env={train_env}"] + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert [l["step"] for l in lines] == [32, 64]
    for l in lines:
        for k in ("train/loss", "train/policy_loss", "train/value_loss", "rollout/ep_rew_mean", "rollout/success_rate", "eval/success_rate",
                  "eval/mean_reward", "eval/mean_ep_length"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
    agent = tmp_path / "run" / "checkpoints" / "model_latest.pth"
    assert agent.exists() and (tmp_path / "run" / "checkpoints" / "model_best.pth").exists()
    over = shared + [f"agent_checkpoint.local_file={agent}", "n_eval_episodes=4", f"run_dir={tmp_path / 'test'}"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "test_sb3.py")] + BASE + [f"env={test_env}"] + over, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(l) for l in open(tmp_path / "test" / "eval.jsonl")]
    assert len(rows) == 1 and set(rows[0]) == {"env", "episodes", "success_rate", "mean_reward", "mean_ep_length"}
    row = rows[0]
    assert row["env"] == "OddOneOutN4C3S1S1Env" and row["episodes"] == 4 and math.isfinite(row["mean_reward"])
    assert 0 <= row["success_rate"] <= 1 and 1 <= row["mean_ep_length"] <= 6
    log(f"test_sb3 on the unseen combination: {row}")
