"""CPU-only checks of the Odd-One-Out task's host side: two hand-worked episodes of the numpy restatement (tests/oddoneout_ref.py, the
reference the GPU tests hold the kernels to), the task's invariants and draw frequencies over 4000 episodes per case, the seven composed
configs, the descriptor's new fields with the library's rejections, and every refusal of ocrl_amd.envs.

Frequency bound: a frequency estimated from M draws of probability p has standard deviation sqrt(p (1 - p) / M); each must lie within
5 of them (a fair source fails one such check with probability 6e-7)."""
import ctypes
import math
import os

import numpy as np
import pytest

from ocrl_amd import envs
from ocrl_amd.utils.config import compose
from tests import oddoneout_ref as O
from tests import sprite_env_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
F = np.float32
BASE = ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "num_envs=16", "device=cuda:0"]
M = 4000

# name -> spec keywords: the cases of the GPU reset test too (tests/test_gpu_oddoneout.py)
CASES = {
    "N4C2S2S1": dict(),
    "N4C2S2S1-oc": dict(obj_comp=True),
    "N3C2S2S1": dict(lo=3, hi=3),
    "N3-9C4S4S2": dict(lo=3, hi=9, colors=(0, 1, 2, 3), shapes=(0, 1, 2, 3), scales=(0.15, 0.22)),
    "N6C2S2S1-oc": dict(lo=6, hi=6, obj_comp=True),
    "N7C3S1S1": dict(lo=7, hi=7, colors=(0, 1, 2), shapes=(0,)),
    "N15C7S4S2": dict(lo=15, hi=15, colors=(0, 1, 2, 3, 4, 5, 6), shapes=(0, 1, 2, 3), scales=(0.15, 0.22)),
    "unseen-train": dict(colors=(0, 1, 2), shapes=(0,), unseen_mode="train", unseen_colors=(0, 2)),
    "unseen-test": dict(colors=(0, 1, 2), shapes=(0,), unseen_mode="test", unseen_colors=(0, 2)),
}


def uniforms(k, n=4096):
    """24-bit uniforms of episode k, as the library's dump has them (those of tests/test_sprite_env_cpu.py)"""
    return (np.floor(np.random.RandomState(1000 + k).rand(n) * 2 ** 24) / 2 ** 24).astype(np.float32)


def by_hand(head, n=4096):
    """the given uniforms floored to k / 2^24; the positions, which draw after them, take uniforms(0)"""
    u = uniforms(0, n).astype(np.float64)
    u[:len(head)] = head
    return (np.floor(u * 2 ** 24) / 2 ** 24).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- episodes by hand
def test_hand_worked_episode_on_the_shape():
    """n = 4 (draw 0); target = below(4) at .5 = 2; kinds (colour, shape), below(2) at .6 = shape; u = shapes[below(2) at .1] = 0.
    Colour, all four, A = [0, 1]: v = A[1] (.9), g = 2 + below(3) at .4 = 3: objects 1 (.3 of 4), 0 (0 of 3), 3 (.99 of 2); object 2 is the
    last one and takes 1 too.  Shape, objects 0, 1, 3, A = [1]: v = 1 (.2), g = 2 + below(2) at .7 = 3, three picks (.1, .1, .1).  Scale,
    all four, A = [0.15]: v (0), g = 2 (0): objects 2 (.5 of 4), 1 (.5 of 3); again v (0), g = 2 + below(1) = 2 (0): objects 3 (.9 of 2),
    0 (0 of 1).  22 draws."""
    s = O.spec(lo=4, hi=4, colors=(0, 1), shapes=(0, 1), scales=(0.15,))
    u = by_hand([0, .5, .6, .1, .9, .4, .3, 0, .99, .2, .7, .1, .1, .1, 0, 0, .5, .5, 0, 0, .9, 0])
    rows, n, target, kind, used, props = O.reset(s, u, with_property_draws=True)
    assert (n, target, O.KINDS[kind], props) == (4, 2, "shape", 22) and used > props
    assert rows[:4, 0].tolist() == [1, 1, 1, 1] and rows[:4, 1].tolist() == [1, 1, 0, 1] and (rows[:4, 2] == F(0.15)).all()
    assert tuple(rows[4]) == (3, 3, F(0.15), F(0.5), F(0.5))
    O.check_episode(s, rows, n, target, kind)


def test_hand_worked_episode_with_object_composition():
    """n = 3 + below(3) at .5 = 4; target = below(4) at .3 = 1; kinds (colour, scale), below(2) at 0 = colour; u = colours[below(3) at .7]
    = 2.  obj_comp: shape = shapes[below(1)] = 2 (.9, a draw although the list has one entry), scale = scales[below(2) at .9] = 0.22.
    Colour, objects 0, 2, 3, A = [0, 1]: v = A[1] (.99), g = 2 + below(2) at 0 = 2: objects 0 (0 of 3), 3 (.6 of 2); object 2 is the last
    one.  Shape and scale take no draw.  10 draws."""
    s = O.spec(lo=3, hi=5, colors=(0, 1, 2), shapes=(2,), scales=(0.15, 0.22), obj_comp=True)
    rows, n, target, kind, used, props = O.reset(s, by_hand([.5, .3, 0, .7, .9, .9, .99, 0, 0, .6]), with_property_draws=True)
    assert (n, target, O.KINDS[kind], props) == (4, 1, "colour", 10)
    assert rows[:4, 0].tolist() == [1, 2, 1, 1] and rows[:4, 1].tolist() == [2, 2, 2, 2] and (rows[:4, 2] == F(0.22)).all()
    assert tuple(rows[4]) == (3, 3, F(0.15), F(0.5), F(0.5)) and not rows[5:].any()
    O.check_episode(s, rows, n, target, kind)


def test_positions_are_the_target_tasks():
    """rule 7: from the first position draw on, an episode is placed as a Target episode with the same scales is"""
    s = O.spec()
    u = uniforms(3)
    rows, n, target, kind, used, props = O.reset(s, u, with_property_draws=True)
    t = R.spec(colors=(0, 1), shapes=(0, 1), target=(5, 3, 0.15))               # a target triple no draw can equal: 3 draws per object
    want, n_t, target_t, used_t = R.reset(t, np.concatenate([by_hand([0, 0], 2), np.zeros(9, np.float32), u[props:]]))
    assert n_t == n == 4 and np.array_equal(rows[:5, 3:], want[:5, 3:]) and used - props == used_t - 11


def test_the_env_steps_as_the_base_task_and_starts_the_next_odd_one_out_episode():
    s = O.spec(rew_type="normal")
    env = O.Env(s, uniforms)
    first, n, target, kind, _ = O.reset(s, uniforms(0))
    assert np.array_equal(env.rows, first) and (env.n, env.target, env.unique_kind, env.episode) == (n, target, kind, 0)
    env.rows[:] = 0
    env.rows[0] = (0, 0, F(0.15), F(0.9), F(0.9))
    env.rows[1] = (1, 0, F(0.15), F(0.5), F(0.6))
    env.rows[2] = (0, 0, F(0.15), F(0.1), F(0.9))
    env.rows[3] = (3, 3, F(0.15), F(0.5), F(0.45))
    env.n, env.target = 3, 1
    assert env.step(0) == (F(1), True, True, 1.0, 1)                           # the odd object: reward 1, success
    want, n, target, kind, _ = O.reset(s, uniforms(1))
    assert env.episode == 1 and np.array_equal(env.rows, want) and (env.n, env.target, env.unique_kind, env.step_count) == (n, target, kind, 0)
    env.rows[env.n, 3:] = env.rows[(env.target + 1) % env.n, 3:] + F(0.01)     # beside an object that is not the odd one
    assert env.step(9)[:3] == (F(0.1), True, False) and env.episode == 2


# ---------------------------------------------------------------------------------------------------------------- invariants, frequencies
@pytest.fixture(scope="module")
def episodes():
    """case -> M episodes (n, target, kind, property lists, property draws) of the restatement, made once"""
    out = {}
    for name, kw in CASES.items():
        s = O.spec(**kw)
        eps = []
        for k in range(M):
            st = R._Stream(uniforms(k, 128))
            eps.append(O.objects(s, st) + (st.j,))
        out[name] = (s, eps)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_invariants_over_4000_episodes(episodes, case):
    s, eps = episodes[case]
    lists = (list(s.colors), list(s.shapes), list(s.scales))
    for n, target, T, prop, draws in eps:
        assert s.lo <= n <= s.hi and 0 <= target < n and len(lists[T]) > 1 and draws <= 6 + 6 * n
        rows = np.zeros((n, 5), dtype=np.float32)
        rows[:, :3] = np.array(prop, dtype=np.float32).T
        O.check_episode(s, rows, n, target, T)                                  # on rows, as the GPU test applies it to the device state
        u = prop[T][target]
        assert prop[T].count(u) == 1
        for K in range(3):
            assert all(v in lists[K] for v in prop[K])
            assert all(prop[K].count(v) >= 2 for v in prop[K] if not (K == T and v == u)), (K, prop[K])
            if s.obj_comp and K != T:
                assert len(set(prop[K])) == 1
        others = set(prop[0]) - {u}
        if s.unseen_mode:
            assert target == 0 and T == 0
        if s.unseen_mode == 1:
            assert {u} | others != set(s.unseen_colors)
        if s.unseen_mode == 2:
            assert {u} | others == set(s.unseen_colors) and len(others) == 1


@pytest.mark.parametrize("case", list(CASES))
def test_frequencies_over_4000_episodes(episodes, case):
    s, eps = episodes[case]
    kinds = [K for K, l in enumerate((s.colors, s.shapes, s.scales)) if len(l) > 1]
    worst = 0.0

    def check(count, total, p, what):
        nonlocal worst
        if p == 1.0:
            assert count == total, what
            return
        dev = abs(count / total - p) / math.sqrt(p * (1 - p) / total)
        worst = max(worst, dev)
        assert dev <= 5, (what, count, total, p, dev)
    for K in kinds:
        check(sum(e[2] == K for e in eps), M, 1 / len(kinds), f"kind {K}")
    assert all(e[2] in kinds for e in eps)
    for n in range(s.lo, s.hi + 1):
        check(sum(e[0] == n for e in eps), M, 1 / (s.hi - s.lo + 1), f"n {n}")
    at_lo = [e for e in eps if e[0] == s.lo]
    if not s.unseen_mode:                                                      # the unseen modes take no target draw
        for t in range(s.lo):
            check(sum(e[1] == t for e in at_lo), len(at_lo), 1 / s.lo, f"target {t}")
    print(f"{case}: worst deviation {worst:.2f} standard deviations")


# ---------------------------------------------------------------------------------------------------------------- configs
SEVEN = {
    "odd-one-out-N4C2S2S1": dict(name="OddOneOutN4C2S2S1Env", COLORS=["blue", "green"], SHAPES=["square", "triangle"], SCALES=[0.15]),
    "odd-one-out-N4C2S2S1-oc": dict(name="OddOneOutN4C2S2S1EnvOC", COLORS=["blue", "green"], SHAPES=["square", "triangle"], SCALES=[0.15], obj_comp=True),
    "odd-one-out-N4C3S1S1": dict(name="OddOneOutN4C3S1S1Env", COLORS=["blue", "green", "yellow"], SHAPES=["square"], SCALES=[0.15]),
    "odd-one-out-N6C2S2S1-oc": dict(name="OddOneOutN6C2S2S1EnvOC", COLORS=["blue", "green"], SHAPES=["square", "triangle"], SCALES=[0.15], obj_comp=True,
                                    num_objects_range=[6, 6]),
    "odd-one-out-N4C2S2S2": dict(name="OddOneOutN4C2S2S2Env", COLORS=["blue", "green"], SHAPES=["square", "triangle"], SCALES=[0.15, 0.22]),
    "odd-one-out-N4C3S1S1-ood-unseen-combi-train1": dict(name="OddOneOutN4C3S1S1Env", COLORS=["blue", "green", "yellow"], SHAPES=["square"], SCALES=[0.15],
                                                         unseen_combi_mode="train", unseen_combi=["blue", "yellow"]),
    "odd-one-out-N4C3S1S1-ood-unseen-combi-test1": dict(name="OddOneOutN4C3S1S1Env", COLORS=["blue", "green", "yellow"], SHAPES=["square"], SCALES=[0.15],
                                                        unseen_combi_mode="test", unseen_combi=["blue", "yellow"]),
}
DEFAULTS = dict(num_objects_range=[4, 4], state_size=5, mode="hard", rew_type="sparse", distance_to_agent=0.08, distance_to_objs=0.08, distance_to_wall=0.08,
                num_stacked_obss=1, tags="", obs_size=64, obs_channels=3, moving_step_size=0.05, wo_agent=False, skewed=False, occlusion=False,
                render_mode="image", max_steps=100, agent_pos=[0.5, 0.5], AGENT=["red", "circle", 0.15], unseen_combi_mode=None, unseen_combi=[],
                obj_comp=False, env="OddOneOutEnv")


def cfg(env="odd-one-out-N4C2S2S1", **over):
    return compose(CFG, "train_sb3", BASE + [f"env={env}"] + [f"{k}={v}" for k, v in over.items()])


@pytest.mark.parametrize("name", list(SEVEN))
def test_the_seven_configs_compose_to_the_reference_keys_and_values(name):
    c = cfg(name)
    got = c.env.to_dict()
    assert got.pop("background") == {"use_bg": False, "img_paths": ["../dtd/images/braided", "../dtd/images/stratified"]}
    assert got == dict(DEFAULTS, **SEVEN[name])                                # no `target`: the reference's files have none either
    d = envs.env_desc(c.env, 16)
    want = SEVEN[name]
    assert (d.task, d.E, d.H, d.lo, d.hi, d.mode, d.rew_type, d.max_steps) == (1, 16, 64, *want.get("num_objects_range", [4, 4]), 2, 0, 100)
    assert list(d.colors)[:d.n_colors] == [envs.COLORS.index(v) for v in want["COLORS"]]
    assert list(d.shapes)[:d.n_shapes] == [envs.SHAPES.index(v) for v in want["SHAPES"]]
    assert list(d.scales)[:d.n_scales] == [F(v) for v in want["SCALES"]]
    assert d.obj_comp == int(want.get("obj_comp", False)) and d.unseen_mode == (None, "train", "test").index(want.get("unseen_combi_mode"))
    assert list(d.unseen_colors) == ([0, 2] if d.unseen_mode else [0, 0])
    assert (d.agent_color, d.agent_shape, d.agent_scale, d.agent_x, d.agent_y) == (3, 3, F(0.15), 0.5, 0.5)
    s = O.spec_from_desc(d)
    assert (s.obj_comp, s.unseen_mode, s.unseen_colors) == (bool(d.obj_comp), d.unseen_mode, tuple(d.unseen_colors))


def test_test_sb3_config_composes():
    c = compose(CFG, "test_sb3", BASE + ["env=odd-one-out-N4C3S1S1-ood-unseen-combi-test1", "agent_checkpoint.local_file=/x/model_best.pth",
                                         "agent_checkpoint.run_id=abc"])
    assert (c.viz_interval, c.n_eval_episodes, c.video.interval, c.video.length) == (100, 100, 100, 100)
    assert c.agent_checkpoint.to_dict() == {"entity": "", "project": "", "run_id": "abc", "file": "models/best_model.zip", "local_file": "/x/model_best.pth"}
    assert c.wandb.project == "test_sb3" and c.run_dir == "./outputs/test_sb3/abc-OddOneOutN4C3S1S1Env"
    assert {"ocr", "pooling", "sb3", "sb3_acnet", "env", "wandb", "seed", "device", "num_envs"} <= set(c.keys())


# ---------------------------------------------------------------------------------------------------------------- C ABI
def desc(env="odd-one-out-N4C2S2S1", **over):
    d = envs.env_desc(cfg(env).env, 4)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def rejected(d, *words):
    from ocrl_amd import _lib
    L = _lib.lib()
    assert L.ocrl_sprite_env_state_floats(ctypes.byref(d)) == 0
    msg = L.ocrl_last_error().decode()
    assert all(w in msg for w in words), msg
    assert L.ocrl_sprite_env_reset(ctypes.byref(d), None, 0, None, 0, None) != 0
    assert L.ocrl_sprite_env_step(ctypes.byref(d), None, 0, None, None, None, None, None, None, None) != 0


def test_descriptor_tail_and_rejections():
    from ocrl_amd import _lib
    L = _lib.lib()
    assert L.ocrl_abi_version() == 5 and L.ocrl_sprite_env_desc_size() == ctypes.sizeof(_lib.SpriteEnvDesc)
    names = [f[0] for f in _lib.SpriteEnvDesc._fields_]
    assert names[-5:-1] == ["dist_wall", "task", "obj_comp", "unseen_mode"] and names[-1] == "unseen_colors"
    assert ctypes.sizeof(_lib.SpriteEnvDesc) == _lib.SpriteEnvDesc.dist_wall.offset + 4 + 5 * 4
    # a zeroed tail is the Target task, accepted as before
    t = envs.env_desc(cfg("target-N4C4S3S1").env, 4)
    assert (t.task, t.obj_comp, t.unseen_mode, list(t.unseen_colors)) == (0, 0, 0, [0, 0])
    n = L.ocrl_sprite_env_state_floats(ctypes.byref(t))
    assert n >= 4 * 5 * 5 + 4 * 8 and n % 64 == 0
    for name in SEVEN:
        assert L.ocrl_sprite_env_state_floats(ctypes.byref(desc(name))) >= n, name
    rejected(desc(task=2), "task", "2")
    rejected(desc(task=-1), "task", "-1")
    rejected(desc("target-N4C4S3S1", obj_comp=1), "task 0", "obj_comp")
    rejected(desc("target-N4C4S3S1", unseen_mode=1), "task 0", "unseen_mode")
    rejected(desc(lo=2), "num_objects_range", "lo >= 3", "2")
    rejected(desc(n_colors=1, n_shapes=1), "COLORS, SHAPES or SCALES")
    rejected(desc(unseen_mode=3), "unseen_mode", "3")
    rejected(desc(unseen_mode=-1), "unseen_mode", "-1")
    train = "odd-one-out-N4C3S1S1-ood-unseen-combi-train1"
    two_shapes = desc(train, n_shapes=2)
    two_shapes.shapes[1] = 1
    rejected(two_shapes, "unseen_mode", "SHAPES and SCALES")
    two_scales = desc(train, n_scales=2)
    two_scales.scales[1] = 0.22
    rejected(two_scales, "unseen_mode", "SHAPES and SCALES")
    same = desc(train)
    same.unseen_colors[1] = 0
    rejected(same, "unseen_colors", "0, 0")
    absent = desc(train)
    absent.unseen_colors[1] = 3
    rejected(absent, "unseen_colors", "0, 3")
    rejected(desc(train, n_colors=2), "unseen_mode", "3 or more COLORS")
    twice = desc()
    twice.colors[1] = twice.colors[0]
    rejected(twice, "distinct entries")
    # target_* is ignored for task 1: values the Target task rejects pass
    assert L.ocrl_sprite_env_state_floats(ctypes.byref(desc(target_color=99, target_shape=-1, target_scale=5.0))) == n
    rejected(desc("target-N4C4S3S1", target_color=99), "colour id 99")


# ---------------------------------------------------------------------------------------------------------------- Python
TRAIN = "odd-one-out-N4C3S1S1-ood-unseen-combi-train1"


@pytest.mark.parametrize("env,over,key", [
    ("target-N4C4S3S1", {"env.obj_comp": "True"}, "obj_comp"),
    ("target-N4C4S3S1", {"env.unseen_combi_mode": "train"}, "unseen_combi_mode"),
    ("odd-one-out-N4C2S2S1", {"env.num_objects_range": "[2,4]"}, "num_objects_range"),
    ("odd-one-out-N4C2S2S1", {"env.COLORS": "[blue]", "env.SHAPES": "[square]"}, "COLORS, SHAPES or SCALES"),
    ("odd-one-out-N4C2S2S1", {"env.unseen_combi_mode": "validate"}, "unseen_combi_mode"),
    (TRAIN, {"env.SHAPES": "[square,triangle]"}, "unseen_combi_mode.*SHAPES"),
    (TRAIN, {"env.SCALES": "[0.15,0.22]"}, "unseen_combi_mode.*SCALES"),
    (TRAIN, {"env.unseen_combi": "[blue,blue]"}, "unseen_combi "),
    (TRAIN, {"env.unseen_combi": "[blue,red]"}, "unseen_combi "),
    (TRAIN, {"env.unseen_combi": "[blue]"}, "unseen_combi "),
    (TRAIN, {"env.COLORS": "[blue,yellow]"}, "unseen_combi_mode.*COLORS"),
    ("odd-one-out-N4C2S2S1", {"env.COLORS": "[blue,blue]"}, "COLORS"),
])
def test_value_errors_name_the_key_before_the_library_is_touched(env, over, key):
    c = cfg(env, **over)
    with pytest.raises(ValueError, match=key):
        envs.env_desc(c.env, 4)
    with pytest.raises(ValueError, match=key):
        envs.make_env(c)


def test_make_env_resolves_the_task_and_refuses_the_others():
    assert envs.OddOneOutEnv.on_device is True and envs.TargetEnv.on_device is True
    assert issubclass(envs.OddOneOutEnv, envs.SpriteEnv) and issubclass(envs.TargetEnv, envs.SpriteEnv)
    assert envs.OddOneOutEnv.step_device is envs.TargetEnv.step_device and envs.OddOneOutEnv.reset is envs.TargetEnv.reset
    assert set(envs.OddOneOutEnv._AUX) - set(envs.TargetEnv._AUX) == {"unique_kind"}
    seen = []
    saved = envs._ENVS["OddOneOutEnv"]
    envs._ENVS["OddOneOutEnv"] = lambda *a: seen.append(a) or "built"
    try:
        c = cfg()
        assert envs.make_env(c, num_envs=3, seed=5, device="cuda:0") == "built" and seen == [(c.env, 3, 5, "cuda:0")]
    finally:
        envs._ENVS["OddOneOutEnv"] = saved
    assert envs._ENVS == {"TargetEnv": envs.TargetEnv, "OddOneOutEnv": envs.OddOneOutEnv}
    for name in ("PushEnv", "MazeEnv"):
        with pytest.raises(NotImplementedError, match=f"env: {name} is not built"):
            envs.make_env(cfg(**{"env.env": name}))
    # a class is not built from the other task's config, and the task needs no `target` key
    with pytest.raises(ValueError, match="another task"):
        envs.TargetEnv(cfg().env, 4)
    with pytest.raises(ValueError, match="another task"):
        envs.OddOneOutEnv(cfg("target-N4C4S3S1").env, 4)
    assert "target" not in cfg().env
    with pytest.raises(NotImplementedError, match="agent_pos"):
        envs.OddOneOutEnv(cfg(**{"env.agent_pos": "null"}).env, 4)
    with pytest.raises(ValueError, match="pentagon"):
        envs.OddOneOutEnv(cfg(**{"env.SHAPES": "[square,pentagon]"}).env, 4)
