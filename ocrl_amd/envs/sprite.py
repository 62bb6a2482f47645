"""The sprite tasks (Target, Odd-One-Out) as vectorised environments that live on the GPU (the reference's
envs/synthetic_envs/{base,target,oddoneout}.py run one spriteworld / PIL environment per host process).  State, transition, reward,
auto-reset and frames are the library's (``ocrl_sprite_env_*`` / ``ocrl_sprite_render``, include/ocrl_hip.h: the rules are written
there); this module checks the config, owns the buffers and offers both calling conventions: ``step`` (gym / VecEnv style, host rewards
and infos) and ``step_device`` (device tensors only, no host read: what ``PPO.collect_rollouts`` uses)."""
import ctypes

import numpy as np
import torch

from .. import _lib

COLORS = ["blue", "green", "yellow", "red", "cyan", "pink", "brown"]
SHAPES = ["square", "triangle", "star_4", "circle", "pentagon", "hexagon", "octagon", "star_5", "star_6", "spoke_4", "spoke_5", "spoke_6"]
DRAWN_SHAPES = SHAPES[:4] + ["star_5", "spoke_4"]    # the predicates of ocrl_amd.utils.data._mask: ids 0..3, 7 and 9
COLOR_BYTES = ((0, 0, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0), (0, 255, 255), (255, 192, 203), (165, 42, 42))
MODES, REW_TYPES = ("easy", "normal", "hard"), ("sparse", "normal", "dense")
RENDER_MODES = {"image": 0, "rgb_array": 1, "mask": 2}
TASKS = {"TargetEnv": 0, "OddOneOutEnv": 1}     # config.env -> ocrl_sprite_env_desc.task
UNSEEN_MODES = (None, "train", "test")
STATE_SCALES = (0.15, 0.22)                     # the reference's global SCALES list: a state observation carries a scale as its index here

try:                                            # gym's spaces when importable
    from gym.spaces import Box, Discrete
except Exception:                               # pragma: no cover - gym is not in this image
    class Discrete:
        def __init__(self, n):
            self.n, self.shape, self.dtype = int(n), (), np.int64

        def __repr__(self):
            return f"Discrete({self.n})"

    class Box:
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype

        def __repr__(self):
            return f"Box({self.low}, {self.high}, {self.shape}, {np.dtype(self.dtype).name})"


def _index(names, name, what, allowed=None):
    allowed = names if allowed is None else allowed
    if name not in allowed:
        raise ValueError(f"ocrl_amd.envs: {what} {name!r} is not drawn here (supported: {', '.join(allowed)})")
    return names.index(name)


def env_desc(config, num_envs):
    """SpriteEnvDesc of an env config (configs/env/*.yaml).  Raises NotImplementedError, naming the key, for what is not built and
    ValueError for a name or a value outside the task's lists (a shape outside DRAWN_SHAPES: square, triangle, star_4, circle, star_5
    and spoke_4 are drawn, the reference's six other names are not); touches neither the library nor the GPU."""
    who = "ocrl_amd.envs"
    name = getattr(config, "env", "TargetEnv")
    if name not in TASKS:
        raise NotImplementedError(f"{who}: env: {name} is not built (built: {', '.join(TASKS)})")
    task = TASKS[name]
    if getattr(config, "agent_pos", None) is None:
        raise NotImplementedError(f"{who}: agent_pos: null (a randomly placed agent) is not built; give agent_pos: [x, y]")
    for key in ("skewed", "wo_agent"):
        if getattr(config, key, False):
            raise NotImplementedError(f"{who}: {key}: True is not built")
    bg = getattr(config, "background", None)
    if bg is not None and getattr(bg, "use_bg", False):
        raise NotImplementedError(f"{who}: background.use_bg: True (image backgrounds) is not built; frames have a black background")
    if int(getattr(config, "num_stacked_obss", 1)) > 1:
        raise NotImplementedError(f"{who}: num_stacked_obss > 1 (frame stacking) is not built")
    if config.mode not in MODES:
        raise ValueError(f"{who}: mode {config.mode!r} is not one of {MODES}")
    if config.rew_type not in REW_TYPES:
        raise ValueError(f"{who}: rew_type {config.rew_type!r} is not one of {REW_TYPES}")
    lo, hi = (int(v) for v in config.num_objects_range)
    d = _lib.SpriteEnvDesc(E=int(num_envs), H=int(config.obs_size), lo=lo, hi=hi, mode=MODES.index(config.mode), rew_type=REW_TYPES.index(config.rew_type),
                           occlusion=int(bool(config.occlusion)), max_steps=int(config.max_steps))
    lists = (("COLORS", "colour", COLORS, None, d.colors), ("SHAPES", "shape", SHAPES, DRAWN_SHAPES, d.shapes))
    for key, what, names, allowed, dst in lists:
        vals = list(getattr(config, key))
        if not 1 <= len(vals) <= 8:
            raise ValueError(f"{who}: {key} needs 1 to 8 entries (got {len(vals)})")
        for i, v in enumerate(vals):
            dst[i] = _index(names, v, what, allowed)
    scales = [float(v) for v in config.SCALES]
    if not 1 <= len(scales) <= 8:
        raise ValueError(f"{who}: SCALES needs 1 to 8 entries (got {len(scales)})")
    for i, v in enumerate(scales):
        d.scales[i] = v
    d.n_colors, d.n_shapes, d.n_scales = len(config.COLORS), len(config.SHAPES), len(scales)
    d.task = task
    obj_comp, unseen = bool(getattr(config, "obj_comp", False)), getattr(config, "unseen_combi_mode", None)
    if unseen not in UNSEEN_MODES:
        raise ValueError(f"{who}: unseen_combi_mode {unseen!r} is not one of null, train, test")
    if task == 0:
        if obj_comp or unseen is not None:
            raise ValueError(f"{who}: obj_comp and unseen_combi_mode belong to env: OddOneOutEnv, not to env: {name}")
        d.target_color, d.target_shape, d.target_scale = (_index(COLORS, config.target[0], "colour"), _index(SHAPES, config.target[1], "shape", DRAWN_SHAPES),
                                                          float(config.target[2]))
    else:
        _odd_one_out_fields(d, config, obj_comp, unseen, scales)
    d.agent_color, d.agent_shape, d.agent_scale = _index(COLORS, config.AGENT[0], "colour"), _index(SHAPES, config.AGENT[1], "shape", DRAWN_SHAPES), float(config.AGENT[2])
    d.agent_x, d.agent_y = float(config.agent_pos[0]), float(config.agent_pos[1])
    d.step_size, d.dist_agent, d.dist_objs, d.dist_wall = (float(config.moving_step_size), float(config.distance_to_agent), float(config.distance_to_objs),
                                                           float(config.distance_to_wall))
    return d


def _odd_one_out_fields(d, config, obj_comp, unseen, scales):
    """the Odd-One-Out part of env_desc: obj_comp, the unseen mode and its two colours, with the library's rejections by config key"""
    who = "ocrl_amd.envs"
    if d.lo < 3:
        raise ValueError(f"{who}: num_objects_range: OddOneOutEnv needs at least 3 objects, two others must share a value (got [{d.lo}, {d.hi}])")
    if max(d.n_colors, d.n_shapes, d.n_scales) < 2:
        raise ValueError(f"{who}: OddOneOutEnv needs more than one entry in COLORS, SHAPES or SCALES to pick the odd value from")
    for key, vals in (("COLORS", list(config.COLORS)), ("SHAPES", list(config.SHAPES)), ("SCALES", scales)):
        if len(set(vals)) != len(vals):
            raise ValueError(f"{who}: {key}: OddOneOutEnv needs distinct entries (got {vals})")
    d.obj_comp, d.unseen_mode = int(obj_comp), UNSEEN_MODES.index(unseen)
    if unseen is None:
        return
    if d.n_shapes != 1 or d.n_scales != 1:
        raise ValueError(f"{who}: unseen_combi_mode: {unseen} needs one entry each in SHAPES and SCALES, the odd kind must be the colour "
                         f"(got {d.n_shapes}, {d.n_scales})")
    if d.n_colors < 3:
        raise ValueError(f"{who}: unseen_combi_mode: {unseen} needs 3 or more COLORS (got {d.n_colors})")
    pair = list(getattr(config, "unseen_combi", None) or [])
    if len(pair) != 2 or pair[0] == pair[1] or any(c not in list(config.COLORS) for c in pair):
        raise ValueError(f"{who}: unseen_combi must be two different entries of COLORS (got {pair})")
    d.unseen_colors[0], d.unseen_colors[1] = COLORS.index(pair[0]), COLORS.index(pair[1])


def _check_state_scales(config, task):
    """render_mode: state writes every scale as its index in STATE_SCALES; the reference raises from list.index at the first render of
    another one, here the config is refused by key"""
    known = [np.float32(v) for v in STATE_SCALES]
    keys = [("SCALES", list(config.SCALES)), ("AGENT", [config.AGENT[2]])] + ([("target", [config.target[2]])] if task == 0 else [])
    for key, vals in keys:
        for v in vals:
            if np.float32(float(v)) not in known:
                raise ValueError(f"ocrl_amd.envs: {key}: scale {v} has no index in the state observation (render_mode: state knows {list(STATE_SCALES)})")


class SpriteEnv:
    """``num_envs`` sprite tasks stepping together on ``device``; a subclass names the task (``TASK``, a key of TASKS).  Observations are
    uint8 frames [E, 3, H, W] (what stable-baselines3 hands the policy after its image transpose), or with ``render_mode: state`` the
    reference's state observation, fp32 [E, hi + 1, 5] (ocrl_sprite_state_obs; no frame is rendered); actions 0..3 = up, left, down, right.
    A finished environment starts its next episode inside the step that finished it: the observation returned for it is the new
    episode's first frame, and the finished episode's return and length come back with that step."""
    on_device = True
    TASK = None

    def __init__(self, config_env, num_envs, seed=0, device="cuda"):
        self.config, self.num_envs, self.seed = config_env, int(num_envs), int(seed)
        self._desc = env_desc(config_env, num_envs)               # refusals first: nothing below runs for a config that is not built
        d = self._desc
        if d.task != TASKS[self.TASK]:
            raise ValueError(f"ocrl_amd.envs.{self.TASK}: the config's env: {getattr(config_env, 'env', 'TargetEnv')} is another task")
        self.obs_size, self.rows = d.H, d.hi + 1
        self.render_mode = getattr(config_env, "render_mode", "image")
        self._state_obs = self.render_mode == "state"
        if self._state_obs:
            _check_state_scales(config_env, d.task)
            self.observation_space = Box(0, 1, (d.hi + 1, 5), np.float32)       # the reference's space, bounds included (base.py)
        else:
            self.observation_space = Box(0, 255, (3, d.H, d.H), np.uint8)
        self.action_space = Discrete(4)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"ocrl_amd.envs.{self.TASK} runs on the GPU (device={device!r}); there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        n = L.ocrl_sprite_env_state_floats(ctypes.byref(d))
        if n == 0:
            raise ValueError("ocrl_hip: " + L.ocrl_last_error().decode())
        E, R = self.num_envs, self.rows
        self._state = torch.zeros(n, device=self.device)
        off = (E * R * 5 + 63) & ~63
        self._rows = self._state[:E * R * 5].view(E, R, 5)
        self._rows_ptr = _lib.ptr(self._rows)
        self._aux = self._state[off:off + 8 * E].view(torch.int32).view(E, 8)
        self._ret = self._state[off:off + 8 * E].view(torch.float64).view(E, 4)[:, 3]
        self._started = False

    # ---- the library calls
    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            _lib.check(fn(*args, _lib.stream(self.device)))

    def _frames(self, mode=0, rows=None):
        rows = self._rows if rows is None else rows.to(device=self.device, dtype=torch.float32).contiguous()
        E, R, H = rows.shape[0], rows.shape[1], self.obs_size
        shape = {0: (E, 3, H, H), 1: (E, H, H, 3), 2: (E, R + 1, H, H, 1)}[mode]
        out = torch.empty(shape, device=self.device, dtype=torch.uint8)
        self._call(_lib.lib().ocrl_sprite_render, _lib.ptr(rows), E, R, H, mode, _lib.ptr(out))
        return out

    def state_obs(self, rows):
        """the state observation (render(mode="state") of the reference) of hand-made rows [E', R, 5], R <= 16"""
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(rows)
        self._call(_lib.lib().ocrl_sprite_state_obs, _lib.ptr(rows), rows.shape[0], rows.shape[1], _lib.ptr(out))
        return out

    def observe(self):
        """the observation of the current state in the environment's mode, a fresh tensor: what reset and the steps return"""
        if not self._state_obs:
            return self._frames()
        out = torch.empty_like(self._rows)
        self._call(_lib.lib().ocrl_sprite_state_obs, self._rows_ptr, self.num_envs, self.rows, _lib.ptr(out))
        return out

    def reset(self, mask=None):
        """new episodes for every environment (or those ``mask`` [E] selects) -> observations.  The first reset starts episode 0
        of every environment's stream; later ones the episode after the current one."""
        m = None if mask is None else torch.as_tensor(mask).to(device=self.device).ne(0).to(torch.uint8).contiguous()
        self._call(_lib.lib().ocrl_sprite_env_reset, ctypes.byref(self._desc), _lib.ptr(self._state), self.seed, _lib.ptr(m), -1 if self._started else 0)
        self._started = True
        return self.observe()

    def step_device(self, actions):
        """actions int64 [E] on the device -> (observations, rewards fp32, dones bool, extras) as fresh device tensors; extras has ``is_success``
        (bool), ``episode_return`` (float64) and ``episode_length`` (int32) of the episodes this step finished.  No host read."""
        if not self._started:
            raise RuntimeError(f"ocrl_amd.envs.{self.TASK}: step before reset()")
        E = self.num_envs
        a = actions.to(device=self.device, dtype=torch.int64).reshape(E).contiguous()
        rewards = torch.empty(E, device=self.device)
        flags = torch.empty(2, E, device=self.device, dtype=torch.uint8)
        ret = torch.empty(E, device=self.device, dtype=torch.float64)
        length = torch.empty(E, device=self.device, dtype=torch.int32)
        self._call(_lib.lib().ocrl_sprite_env_step, ctypes.byref(self._desc), _lib.ptr(self._state), self.seed, _lib.ptr(a), _lib.ptr(rewards),
                   _lib.ptr(flags[0]), _lib.ptr(flags[1]), _lib.ptr(ret), _lib.ptr(length))
        flags = flags.view(torch.bool)
        return self.observe(), rewards, flags[0], {"is_success": flags[1], "episode_return": ret, "episode_length": length}

    def step(self, actions):
        """the gym-style call: actions as a numpy array or a tensor -> (observations tensor, rewards, dones as numpy arrays, infos)"""
        a = actions.detach().cpu().numpy() if isinstance(actions, torch.Tensor) else np.asarray(actions)
        a = a.reshape(self.num_envs)
        if ((a < 0) | (a > 3)).any() or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"action must be one of 0, 1, 2, 3 (up, left, down, right), not {a.tolist()}")
        obs, rewards, dones, ex = self.step_device(torch.as_tensor(a.astype(np.int64)))
        host = torch.stack([rewards.double(), dones.double(), ex["is_success"].double(), ex["episode_return"], ex["episode_length"].double()]).cpu().numpy()
        dones_h = host[1] != 0
        infos = [{"is_success": bool(host[2, e])} for e in range(self.num_envs)]
        for e in np.nonzero(dones_h)[0]:
            infos[e]["episode"] = {"r": float(host[3, e]), "l": int(host[4, e])}
        return obs, host[0].astype(np.float32), dones_h, infos

    def render(self, mode=None):
        """``image``: uint8 [E, 3, H, W]; ``rgb_array``: [E, H, W, 3]; ``state``: fp32 [E, hi + 1, 5] rows of (colour id, shape id, scale,
        x, y), the agent after the objects, zero rows last; ``mask``: uint8 [E, hi + 2, H, W, 1], each row alone, the background last"""
        mode = self.render_mode if mode is None else mode
        if mode == "state":
            return self._rows.clone()
        if mode not in RENDER_MODES:
            raise ValueError(f"ocrl_amd.envs: render mode {mode!r} is not one of image, rgb_array, state, mask")
        return self._frames(RENDER_MODES[mode])

    def render_rows(self, rows, mode="image"):
        """frames or masks of hand-made rows [E', R, 5] (R <= 16) at this environment's frame size.  A row is painted when its colour id
        is in 0..6, its shape id one of DRAWN_SHAPES' (0 square, 1 triangle, 2 star_4, 3 circle, 7 star_5, 9 spoke_4) and its scale > 0;
        any other row stays blank"""
        return self._frames(RENDER_MODES[mode], rows)

    _AUX = {"n": 0, "target": 1, "step_count": 2, "episode": 3, "episode_length": 4}

    def get_state(self):
        """copies: rows [E, hi + 1, 5], n, target, step_count, episode, episode_length (int32 [E]; an OddOneOutEnv adds unique_kind) and
        episode_return (float64 [E])"""
        out = {"rows": self._rows.clone(), "episode_return": self._ret.clone()}
        out.update({k: self._aux[:, i].clone() for k, i in self._AUX.items()})
        return out

    def set_state(self, **fields):
        """overwrite any of get_state()'s fields (tensors or arrays of the same shapes), e.g. to place sprites by hand"""
        for k, v in fields.items():
            v = torch.as_tensor(v)
            if k == "rows":
                self._rows.copy_(v.to(self.device, torch.float32))
            elif k == "episode_return":
                self._ret.copy_(v.to(self.device, torch.float64))
            elif k in self._AUX:
                self._aux[:, self._AUX[k]].copy_(v.to(self.device, torch.int32))
            else:
                raise KeyError(f"ocrl_amd.envs.{self.TASK}.set_state: no field {k!r}")
        self._started = True

    def close(self):
        pass


class TargetEnv(SpriteEnv):
    """the Target task: reach the object that carries ``config.target``"""
    TASK = "TargetEnv"


class OddOneOutEnv(SpriteEnv):
    """the Odd-One-Out task: reach the object that alone carries some value of one property kind (``unique_kind``: 0 colour, 1 shape,
    2 scale), with ``obj_comp`` and the unseen-combination train / test modes of the reference"""
    TASK = "OddOneOutEnv"
    _AUX = dict(SpriteEnv._AUX, unique_kind=5)


def sprite_env_uniforms(seed, env0, n_envs, episode, first, n, device="cuda"):
    """[n_envs, n] fp32: the uniforms of draws first .. first + n - 1 of ``episode`` of environments env0 .. (ocrl_sprite_env_uniforms)"""
    out = torch.empty(n_envs, n, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().ocrl_sprite_env_uniforms(int(seed), int(env0), int(n_envs), int(episode), int(first), int(n), _lib.ptr(out), _lib.stream(out.device)))
    return out
