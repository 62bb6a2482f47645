"""numpy restatement of the sprite environment (include/ocrl_hip.h: ocrl_sprite_env_*, ocrl_sprite_render), written from the rules in
the header, one environment at a time.  Positions follow the kernel's fp32 operations one rounding at a time (np.float32 scalars: numpy
rounds every operation and never fuses), so states are compared bit for bit.  The restatement draws nothing itself: ``reset`` consumes
the uniforms handed to it (the dump of ocrl_sprite_env_uniforms, or hand-made ones), draw j of the episode = u[j]."""
import types

import numpy as np

F = np.float32
COLOR_BYTES = np.array([(0, 0, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0), (0, 255, 255), (255, 192, 203), (165, 42, 42)], dtype=np.uint8)
TRIPLE_TRIES, CANDIDATES, RESTARTS = 64, 256, 8
MODES, REW_TYPES = ("easy", "normal", "hard"), ("sparse", "normal", "dense")


def spec(lo=4, hi=4, mode="hard", rew_type="sparse", occlusion=False, max_steps=100, colors=(0, 1, 2, 3), shapes=(0, 1, 2), scales=(0.15,),
         target=(0, 0, 0.15), agent=(3, 3, 0.15), agent_pos=(0.5, 0.5), step_size=0.05, dist_agent=0.08, dist_objs=0.08, dist_wall=0.08):
    """the task's numbers (ids, not names), defaults = configs/env/target-N4C4S3S1.yaml"""
    return types.SimpleNamespace(lo=lo, hi=hi, mode=MODES.index(mode), rew_type=REW_TYPES.index(rew_type), occlusion=bool(occlusion), max_steps=max_steps,
                                 colors=list(colors), shapes=list(shapes), scales=[F(s) for s in scales], target=(target[0], target[1], F(target[2])),
                                 agent=(agent[0], agent[1], F(agent[2])), agent_pos=(F(agent_pos[0]), F(agent_pos[1])), step_size=F(step_size),
                                 dist_agent=F(dist_agent), dist_objs=F(dist_objs), dist_wall=F(dist_wall))


def spec_from_desc(d):
    """the same from an ocrl_amd._lib.SpriteEnvDesc"""
    return types.SimpleNamespace(lo=d.lo, hi=d.hi, mode=d.mode, rew_type=d.rew_type, occlusion=bool(d.occlusion), max_steps=d.max_steps,
                                 colors=list(d.colors)[:d.n_colors], shapes=list(d.shapes)[:d.n_shapes], scales=[F(s) for s in list(d.scales)[:d.n_scales]],
                                 target=(d.target_color, d.target_shape, F(d.target_scale)), agent=(d.agent_color, d.agent_shape, F(d.agent_scale)),
                                 agent_pos=(F(d.agent_x), F(d.agent_y)), step_size=F(d.step_size), dist_agent=F(d.dist_agent), dist_objs=F(d.dist_objs),
                                 dist_wall=F(d.dist_wall))


def box(mode, n, i):
    """[x_min, x_max, y_min, y_max] of object i"""
    if mode == 2:
        return [F(0), F(1), F(0), F(1)]
    left, low = i < 2, i in (1, 2)
    if mode == 1:
        q = (0.0, 0.5, 0.5, 1.0)
    elif n == 4:
        q = (0.2, 0.3, 0.7, 0.8)
    else:
        q = (0.15, 0.35, 0.65, 0.85)
    x = q[:2] if left else q[2:]
    y = q[:2] if low else q[2:]
    return [F(x[0]), F(x[1]), F(y[0]), F(y[1])]


def agent_start(s):
    return s.agent_pos if s.mode == 2 else (F(0.5), F(0.5))


def dist(ax, ay, bx, by):
    dx, dy = F(ax - bx), F(ay - by)
    return np.sqrt(F(F(dx * dx) + F(dy * dy)))


class _Stream:
    def __init__(self, u):
        self.u, self.j = np.asarray(u, dtype=np.float32), 0

    def bits(self):
        if self.j >= len(self.u):
            raise IndexError(f"the episode needs more than {len(self.u)} uniforms")
        b = int(self.u[self.j] * 16777216.0)
        self.j += 1
        return b

    def below(self, m):
        return (self.bits() * m) >> 24

    def u01(self):
        return F(self.bits()) * F(1.0 / 16777216.0)


def _pos(st, mode, lo, hi, r, wall):
    if lo == hi:
        return lo
    a, b = lo, hi
    if mode != 0:
        a, b = F(F(lo + r) + wall), F(F(hi - r) - wall)
    return F(a + F(F(b - a) * st.u01()))


def reset(s, u):
    """one episode from the uniforms u -> (rows [hi + 1, 5] fp32, n, target, draws used)"""
    st = _Stream(u)
    n = s.lo + st.below(s.hi - s.lo + 1)
    target = st.below(n)
    objs = []
    for i in range(n):
        c, h, z = s.target
        if i != target:
            for _ in range(TRIPLE_TRIES):
                c, h, z = s.colors[st.below(len(s.colors))], s.shapes[st.below(len(s.shapes))], s.scales[st.below(len(s.scales))]
                if (c, h, z) != s.target:
                    break
        objs.append((c, h, z))
    ax, ay = agent_start(s)
    ra = F(s.agent[2] * F(0.5))
    px, py = [F(0)] * n, [F(0)] * n
    for attempt in range(RESTARTS + 1):
        dead = False
        for i in range(n):
            b = box(s.mode, n, i)
            r = F(objs[i][2] * F(0.5))
            ok = False
            for _ in range(CANDIDATES):
                x = _pos(st, s.mode, b[0], b[1], r, s.dist_wall)
                y = _pos(st, s.mode, b[2], b[3], r, s.dist_wall)
                ok = True
                for j in range(i):
                    thr = F(0.15) if s.occlusion else F(F(r + F(objs[j][2] * F(0.5))) + s.dist_objs)
                    if dist(px[j], py[j], x, y) < thr:
                        ok = False
                thr = F(0.15) if s.occlusion else F(F(r + ra) + s.dist_agent)
                if dist(ax, ay, x, y) < thr:
                    ok = False
                if ok:
                    break
            px[i], py[i] = x, y
            if not ok and attempt < RESTARTS:
                dead = True
                break
        if not dead:
            break
    rows = np.zeros((s.hi + 1, 5), dtype=np.float32)
    for i in range(n):
        rows[i] = (objs[i][0], objs[i][1], objs[i][2], px[i], py[i])
    rows[n] = (s.agent[0], s.agent[1], s.agent[2], ax, ay)
    return rows, n, target, st.j


class Env:
    """one environment: rows, n, target, step_count, episode, ep_return (a Python float: double), ep_length"""

    def __init__(self, s, uniforms):
        """uniforms(k) -> the uniforms of episode k"""
        self.s, self.uniforms, self.episode = s, uniforms, -1
        self.new_episode()

    def new_episode(self):
        self.episode += 1
        self.rows, self.n, self.target, _ = reset(self.s, self.uniforms(self.episode))
        self.step_count, self.ep_return, self.ep_length = 0, 0.0, 0

    def step(self, act):
        """-> (reward fp32, done, success, finished return, finished length); a finished episode is replaced by the next one"""
        s, q, n = self.s, self.rows, self.n
        x, y = q[n, 3], q[n, 4]
        tx, ty = q[self.target, 3], q[self.target, 4]
        before = dist(tx, ty, x, y)
        if act == 0:
            y = F(y + s.step_size)
        elif act == 1:
            x = F(x - s.step_size)
        elif act == 2:
            y = F(y - s.step_size)
        elif act == 3:
            x = F(x + s.step_size)
        ra = F(s.agent[2] * F(0.5))
        top = F(F(1) - ra)
        x, y = min(max(x, ra), top), min(max(y, ra), top)
        q[n, 3], q[n, 4] = x, y
        self.step_count += 1
        done, success, reward = self.step_count >= s.max_steps, False, F(0)
        if s.rew_type == 2:
            reward = F(0.01) if dist(tx, ty, x, y) < before else F(-0.01)
        for i in range(n):
            if dist(q[i, 3], q[i, 4], x, y) < s.agent[2]:
                if i == self.target:
                    reward, success = F(1), True
                else:
                    reward = F(0.1) if s.rew_type == 1 else F(0)
                done = True
                break
        self.ep_return += float(reward)
        self.ep_length += 1
        fin = (self.ep_return, self.ep_length) if done else (0.0, 0)
        if done:
            self.new_episode()
        return reward, done, success, fin[0], fin[1]


# ---------------------------------------------------------------------------------------------------------------- the renderer
def covers(shape, dx, dy, r):
    """the predicates of ocrl_amd.utils.data._mask in the dtype of the arguments (arrays dx, dy; scalar r)"""
    ax, ay = np.abs(dx), np.abs(dy)
    if shape == 0:
        return (ax <= r) & (ay <= r)
    if shape == 1:
        t = (dy + r) / (r + r)
        return (t >= 0) & (t <= 1) & (ax <= r * t)
    if shape == 2:
        return np.sqrt(ax) + np.sqrt(ay) <= np.sqrt(r) * type(r)(1.25)
    return dx * dx + dy * dy <= r * r


def margin(shape, dx, dy, r):
    """float64: how far each pixel's decision is from flipping.  A predicate is a conjunction of comparisons with slacks s_i (>= 0:
    satisfied).  A covered pixel flips when its smallest slack crosses zero; an uncovered one only when every violated comparison does,
    the most violated one last: either way the margin is |min_i s_i|.  The slacks are lengths in frame units (the circle's is its
    radius minus the distance to the centre, the triangle's heights are not divided by the side), the star's a difference of roots."""
    ax, ay = np.abs(dx), np.abs(dy)
    if shape == 0:
        return np.abs(np.minimum(r - ax, r - ay))
    if shape == 1:
        return np.abs(np.minimum(np.minimum(dy + r, r - dy), (dy + r) / 2 - ax))
    if shape == 2:
        return np.abs(np.sqrt(r) * 1.25 - np.sqrt(ax) - np.sqrt(ay))
    return np.abs(r - np.hypot(dx, dy))


def drawn(row):
    return 0 <= row[0] < 7 and 0 <= row[1] < 4 and row[2] > 0


def render(rows, H, dtype=np.float32, with_margin=False):
    """rows [R, 5] -> (image uint8 [H, H, 3], masks uint8 [R + 1, H, H, 1]) with the arithmetic in ``dtype``; with_margin adds the
    float64 decision margin of every pixel to the nearest sprite edge [H, H]"""
    T = dtype
    lin = (np.arange(H).astype(T) + T(0.5)) / T(H)
    xx, yy = np.meshgrid(lin, lin)
    img = np.zeros((H, H, 3), dtype=np.uint8)
    R = rows.shape[0]
    masks = np.zeros((R + 1, H, H, 1), dtype=np.uint8)
    marg = np.full((H, H), np.inf)
    for j in range(R):
        if not drawn(rows[j]):
            continue
        cx, cy, r = T(rows[j, 3]), T(rows[j, 4]), T(T(rows[j, 2]) * T(0.5))
        m = covers(int(rows[j, 1]), xx - cx, yy - cy, r)
        img[m] = COLOR_BYTES[int(rows[j, 0])]
        masks[j, :, :, 0] = m
        if with_margin:
            l64 = (np.arange(H) + 0.5) / H
            x64, y64 = np.meshgrid(l64, l64)
            marg = np.minimum(marg, margin(int(rows[j, 1]), x64 - float(rows[j, 3]), y64 - float(rows[j, 4]), float(rows[j, 2]) * 0.5))
    masks[R, :, :, 0] = masks[:R].sum(0)[:, :, 0] == 0
    return (img, masks, marg) if with_margin else (img, masks)
