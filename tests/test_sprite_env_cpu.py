"""CPU-only checks of the sprite environment's host side: hand-worked transitions of the numpy restatement (tests/sprite_env_ref.py,
the reference the GPU tests hold the kernels to), the restated renderer against the pre-training scenes, the composed config, the new
C symbols with their rejections, and every refusal of ocrl_amd.envs."""
import ctypes
import os

import numpy as np
import pytest

from ocrl_amd import envs
from ocrl_amd.utils.config import compose
from tests import sprite_env_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
F = np.float32
OVERRIDES = ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=16", "device=cuda:0"]


def uniforms(k, n=4096):
    """24-bit uniforms of episode k, as the library's dump has them"""
    return (np.floor(np.random.RandomState(1000 + k).rand(n) * 2 ** 24) / 2 ** 24).astype(np.float32)


def placed(s, objs, agent_xy, target=0):
    """an environment of the restatement holding hand-placed sprites: objs = [(colour, shape, x, y)], all at scale 0.15"""
    env = R.Env(s, uniforms)
    env.rows[:] = 0
    for i, (c, h, x, y) in enumerate(objs):
        env.rows[i] = (c, h, F(0.15), x, y)
    env.rows[len(objs)] = (3, 3, F(0.15), agent_xy[0], agent_xy[1])
    env.n, env.target, env.episode = len(objs), target, 0
    return env


# ---------------------------------------------------------------------------------------------------------------- transitions by hand
@pytest.mark.parametrize("is_target", [True, False])
def test_contact_fires_below_the_agent_scale_and_not_at_it(is_target):
    """the agent moves up from (0.3, 0.45) to (0.3, Y); fp32(0.3) - fp32(0.15) is fp32(0.15) exactly, so an object at (fp32(0.15), Y) is at
    distance exactly AGENT scale: no contact.  One ulp closer: contact."""
    s = R.spec(rew_type="normal")
    Y = F(F(0.45) + F(0.05))
    assert F(F(0.3) - F(0.15)) == F(0.15) and R.dist(F(0.15), Y, F(0.3), Y) == F(0.15)
    far = (0, 0, F(0.9), F(0.9))
    at = (1, 1, F(0.15), Y)
    objs, target = ([at, far], 0) if is_target else ([far, at], 0)
    env = placed(s, objs, (F(0.3), F(0.45)), target)
    assert env.step(0) == (F(0), False, False, 0.0, 0) and env.rows[2, 4] == Y and env.step_count == 1
    near = (1, 1, np.nextafter(F(0.15), F(1)), Y)
    objs = [near, far] if is_target else [far, near]
    env = placed(s, objs, (F(0.3), F(0.45)), target)
    reward, done, success, ret, length = env.step(0)
    assert done and success == is_target and reward == (F(1) if is_target else F(0.1)) and length == 1 and ret == float(reward)
    # the finished environment holds the next episode of its stream
    want, n, t, _ = R.reset(s, uniforms(1))
    assert env.episode == 1 and np.array_equal(env.rows, want) and (env.n, env.target, env.step_count, env.ep_length) == (n, t, 0, 0)


def test_the_first_object_in_index_order_decides_a_double_contact():
    s = R.spec(rew_type="normal")
    env = placed(s, [(1, 1, F(0.55), F(0.5)), (0, 0, F(0.5), F(0.55))], (F(0.5), F(0.45)), target=1)
    assert env.step(0)[:3] == (F(0.1), True, False)
    env = placed(s, [(0, 0, F(0.5), F(0.55)), (1, 1, F(0.55), F(0.5))], (F(0.5), F(0.45)), target=0)
    assert env.step(0)[:3] == (F(1), True, True)


def test_walls_clip_the_agent_to_its_radius():
    s = R.spec()
    far = [(0, 0, F(0.5), F(0.5))]
    r = F(0.075)
    for start, act, want in (((F(0.1), F(0.3)), 1, (r, F(0.3))), ((F(0.3), F(0.1)), 2, (F(0.3), r)), ((F(0.9), F(0.3)), 3, (F(1) - r, F(0.3))),
                             ((F(0.3), F(0.9)), 0, (F(0.3), F(1) - r))):
        env = placed(s, far, start)
        assert env.step(act)[:2] == (F(0), False)
        assert (env.rows[1, 3], env.rows[1, 4]) == want
    env = placed(s, far, (F(0.3), F(0.3)))
    env.step(7)                                                # outside 0..3: the agent stays
    assert (env.rows[1, 3], env.rows[1, 4]) == (F(0.3), F(0.3)) and env.step_count == 1


def test_time_out_at_max_steps():
    s = R.spec(max_steps=3, rew_type="dense")
    env = placed(s, [(0, 0, F(0.9), F(0.9))], (F(0.2), F(0.2)))
    assert env.step(1) == (F(-0.01), False, False, 0.0, 0)
    assert env.step(3) == (F(0.01), False, False, 0.0, 0)
    reward, done, success, ret, length = env.step(3)
    assert (reward, done, success, length) == (F(0.01), True, False, 3)
    assert ret == float(F(-0.01)) + float(F(0.01)) + float(F(0.01))            # the fp32 rewards summed in double
    assert env.episode == 1 and env.step_count == 0


def test_dense_reward_follows_the_distance_to_the_target():
    s = R.spec(rew_type="dense")
    env = placed(s, [(1, 1, F(0.2), F(0.8)), (0, 0, F(0.8), F(0.5))], (F(0.5), F(0.5)), target=1)
    assert env.step(3)[0] == F(0.01) and env.step(1)[0] == F(-0.01)
    assert env.step(0)[0] == F(-0.01) and env.step(2)[0] == F(0.01)           # straight up from level with the target: away, then back
    env = placed(s, [(0, 0, F(0.5), F(0.075))], (F(0.075), F(0.5)))
    assert env.step(1)[0] == F(-0.01)                                          # held by the wall: the distance did not shrink


@pytest.mark.parametrize("rew_type,want", [("sparse", 0.0), ("normal", 0.1), ("dense", 0.0)])
def test_non_target_contact_reward(rew_type, want):
    s = R.spec(rew_type=rew_type)
    env = placed(s, [(0, 0, F(0.9), F(0.9)), (1, 1, F(0.5), F(0.6))], (F(0.5), F(0.45)))
    reward, done, success, ret, length = env.step(0)
    assert (reward, done, success, length) == (F(want), True, False, 1) and ret == float(F(want))


# ---------------------------------------------------------------------------------------------------------------- reset by hand
@pytest.mark.parametrize("kw", [dict(), dict(mode="normal"), dict(mode="easy"), dict(mode="easy", lo=2, hi=3), dict(occlusion=True),
                                dict(lo=1, hi=9, occlusion=True)], ids=["hard", "normal", "easy", "easy23", "occl", "occl1-9"])
def test_restated_reset_respects_the_task(kw):
    s = R.spec(**kw)
    seen = set()
    for k in range(40):
        rows, n, target, used = R.reset(s, uniforms(k))
        seen.add(n)
        assert s.lo <= n <= s.hi and 0 <= target < n and used <= 4096
        assert tuple(rows[n]) == (3, 3, F(0.15), F(0.5), F(0.5)) and not rows[n + 1:].any()
        for i in range(n):
            c, h, z, x, y = rows[i]
            assert ((c, h, z) == s.target) == (i == target)
            b = R.box(s.mode, n, i)
            pad = 0.0 if s.mode == 0 else float(z) / 2 + 0.08
            assert b[0] + pad - 1e-6 <= x <= b[1] - pad + 1e-6 and b[2] + pad - 1e-6 <= y <= b[3] - pad + 1e-6
            assert np.hypot(x - 0.5, y - 0.5) >= (0.15 if s.occlusion else 0.15 + 0.08) - 1e-6
            for j in range(i):
                assert np.hypot(x - rows[j, 3], y - rows[j, 4]) >= (0.15 if s.occlusion else 0.15 + 0.08) - 1e-6
    assert seen == set(range(s.lo, s.hi + 1)) or s.hi - s.lo > 5


def test_a_degenerate_interval_takes_no_draw():
    st = R._Stream(uniforms(0))
    assert R._pos(st, 0, F(0.25), F(0.25), F(0.075), F(0.08)) == F(0.25) and st.j == 0
    assert R._pos(st, 0, F(0.2), F(0.3), F(0.075), F(0.08)) == F(F(0.2) + F(F(F(0.3) - F(0.2)) * uniforms(0)[0])) and st.j == 1


# ---------------------------------------------------------------------------------------------------------------- the renderer
def test_restated_renderer_reproduces_the_pretraining_scenes():
    """float64 restatement from the object states random_sprite_scenes returns: the very images, byte for byte, and the masks wherever no
    later object occludes (the scenes' masks are visibility masks; the environment's are unoccluded)"""
    from ocrl_amd.utils.data import SCALES, random_sprite_scenes
    img, masks, objs = random_sprite_scenes(32, 64, with_masks=True, with_objs=True)
    for i in range(32):
        rows = objs[i].astype(np.float64)
        rows[:, 2] = [SCALES[int(k)] for k in objs[i, :, 2]]
        got, gm = R.render(rows, 64, np.float64)
        assert np.array_equal(got, img[i]), i
        assert np.array_equal(gm[-1], masks[i, -1].astype(np.uint8))
        assert (gm[:-1] >= masks[i, :-1].astype(np.uint8)).all()
        assert np.array_equal(gm[4], masks[i, 4].astype(np.uint8))             # nothing is painted over the last object


def test_renderer_order_skips_and_colours():
    rows = np.zeros((4, 5), dtype=np.float32)
    rows[0] = (5, 0, 0.5, 0.5, 0.5)          # a pink square under ...
    rows[1] = (-1, 0, 0.9, 0.5, 0.5)         # ... a skipped one and ...
    rows[2] = (6, 3, 0.25, 0.5, 0.5)         # ... a brown circle; row 3 is empty
    img, masks = R.render(rows, 16)
    assert tuple(img[8, 8]) == (165, 42, 42) and tuple(img[4, 4]) == (255, 192, 203) and tuple(img[0, 0]) == (0, 0, 0)
    assert masks[0, 8, 8, 0] == 1 and masks[2, 8, 8, 0] == 1 and not masks[1].any() and not masks[3].any()
    assert masks[4, 0, 0, 0] == 1 and masks[4, 8, 8, 0] == 0 and np.array_equal(masks[4, :, :, 0], 1 - masks[0, :, :, 0])
    tri, _ = R.render(np.array([[1, 1, 0.5, 0.5, 0.5]], dtype=np.float32), 16)
    assert 0 < tri[5, :, 1].sum() < tri[11, :, 1].sum()                      # the apex lies in the rows of small y


# ---------------------------------------------------------------------------------------------------------------- config
def test_target_env_config_composes_to_the_reference_key_set():
    c = compose(CFG, "train_sb3", OVERRIDES)
    assert set(c.env.keys()) == {"num_objects_range", "state_size", "mode", "rew_type", "distance_to_agent", "distance_to_objs", "distance_to_wall",
                                 "num_stacked_obss", "tags", "obs_size", "obs_channels", "moving_step_size", "wo_agent", "skewed", "occlusion",
                                 "render_mode", "max_steps", "agent_pos", "SHAPES", "COLORS", "SCALES", "AGENT", "background", "unseen_combi_mode",
                                 "unseen_combi", "obj_comp", "name", "env", "target"}
    assert set(c.env.background.keys()) == {"use_bg", "img_paths"}
    assert c.env.name == "TargetN4C4S3S1Env" and c.env.env == "TargetEnv" and c.env.target == ["blue", "square", 0.15]
    assert c.env.COLORS == ["blue", "green", "yellow", "red"] and c.env.SHAPES == ["square", "triangle", "star_4"] and c.env.SCALES == [0.15]
    assert c.env.AGENT == ["red", "circle", 0.15] and c.env.agent_pos == [0.5, 0.5] and c.env.num_objects_range == [4, 4]
    assert (c.env.mode, c.env.rew_type, c.env.max_steps, c.env.moving_step_size, c.env.obs_size) == ("hard", "sparse", 100, 0.05, 64)
    assert c.num_envs == 16 and c.max_steps == 2e6 and c.eval.freq == 1000 and c.eval.n_episodes == 100 and c.sb3.algo_kwargs.n_steps == 2048
    assert {"video", "viz_interval", "model_name", "session_name", "wandb", "ocr", "pooling", "sb3", "sb3_acnet"} <= set(c.keys())
    d = envs.env_desc(c.env, c.num_envs)
    s = R.spec_from_desc(d)
    want = R.spec()
    assert vars(s) == vars(want)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def _desc(**over):
    c = compose(CFG, "train_sb3", OVERRIDES)
    d = envs.env_desc(c.env, 4)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_new_symbols_are_exported_and_bad_descriptors_are_rejected():
    from ocrl_amd import _lib
    L = _lib.lib()
    for name in ("ocrl_sprite_env_state_floats", "ocrl_sprite_env_reset", "ocrl_sprite_env_step", "ocrl_sprite_render", "ocrl_sprite_env_uniforms",
                 "ocrl_sprite_env_desc_size"):
        assert hasattr(L, name), name
    assert L.ocrl_abi_version() == 5 and L.ocrl_sprite_env_desc_size() == ctypes.sizeof(_lib.SpriteEnvDesc)
    d = _desc()
    n = L.ocrl_sprite_env_state_floats(ctypes.byref(d))
    assert n >= 4 * 5 * 5 + 4 * 8 and n % 64 == 0
    for over, words in ((dict(hi=16), ("num_objects_range", "16")), (dict(H=30), ("obs_size", "30")), (dict(H=62), ("multiple of 4", "62"))):
        assert L.ocrl_sprite_env_state_floats(ctypes.byref(_desc(**over))) == 0
        msg = L.ocrl_last_error().decode()
        assert all(w in msg for w in words), msg
    bad = _desc()
    bad.shapes[1] = 5
    assert L.ocrl_sprite_env_state_floats(ctypes.byref(bad)) == 0 and "shape id 5" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_env_state_floats(ctypes.byref(_desc(mode=1, lo=3))) == 0 and "normal mode" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_env_state_floats(ctypes.byref(_desc(mode=0, hi=5))) == 0 and "easy mode" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_env_state_floats(None) == 0
    # the argument checks of the launching entry points come before any launch
    assert L.ocrl_sprite_render(None, 1, 5, 64, 0, None, None) != 0 and "null" in L.ocrl_last_error().decode()
    assert L.ocrl_sprite_env_step(ctypes.byref(d), None, 0, None, None, None, None, None, None, None) != 0
    assert L.ocrl_sprite_env_reset(ctypes.byref(_desc(hi=16)), None, 0, None, 0, None) != 0
    assert L.ocrl_sprite_env_uniforms(0, 0, 1, 0, 0, 0, None, None) != 0


# ---------------------------------------------------------------------------------------------------------------- refusals
def _cfg(**over):
    c = compose(CFG, "train_sb3", OVERRIDES + [f"{k}={v}" for k, v in over.items()])
    return c


@pytest.mark.parametrize("over,key", [({"env.agent_pos": "null"}, "agent_pos"), ({"env.skewed": "True"}, "skewed"),
                                      ({"env.background.use_bg": "True"}, "background.use_bg"), ({"env.wo_agent": "True"}, "wo_agent"),
                                      ({"env.num_stacked_obss": "2"}, "num_stacked_obss")])
def test_what_is_not_built_raises_and_names_the_key(over, key):
    c = _cfg(**over)
    with pytest.raises(NotImplementedError, match=key):
        envs.TargetEnv(c.env, 4, seed=0, device="cuda")
    with pytest.raises(NotImplementedError, match=key):
        envs.make_env(c)


def test_other_environments_and_shapes_are_refused_by_name():
    with pytest.raises(NotImplementedError, match="env: PushEnv"):
        envs.make_env(_cfg(**{"env.env": "PushEnv"}))
    with pytest.raises(ValueError, match="pentagon"):
        envs.TargetEnv(_cfg(**{"env.SHAPES": "[square,pentagon]"}).env, 4)
    with pytest.raises(ValueError, match="hexagon"):
        envs.TargetEnv(_cfg(**{"env.AGENT": "[red,hexagon,0.15]"}).env, 4)
    with pytest.raises(ValueError, match="purple"):
        envs.TargetEnv(_cfg(**{"env.target": "[purple,square,0.15]"}).env, 4)
    with pytest.raises(ValueError, match="mode"):
        envs.TargetEnv(_cfg(**{"env.mode": "extreme"}).env, 4)


def test_spaces_and_the_ppo_contract():
    """what PPO reads of an environment before any step: the spaces (no GPU needed to build them)"""
    from ocrl_amd.envs.sprite import Box, Discrete
    a, o = Discrete(4), Box(0, 255, (3, 64, 64), np.uint8)
    assert a.n == 4 and isinstance(a.n, int) and tuple(o.shape) == (3, 64, 64) and np.dtype(o.dtype) == np.uint8
    assert envs.TargetEnv.on_device is True
