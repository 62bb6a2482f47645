"""numpy restatement of the Odd-One-Out episode (include/ocrl_hip.h: "The Odd-One-Out episode", rules 1 to 7), written from the header,
one environment at a time.  Streams, boxes, positions, the transition and the renderer are those of tests/sprite_env_ref.py: the step is
the same for both tasks, only how an episode's objects are made differs.  Like that module it draws nothing itself: ``reset`` consumes
the uniforms handed to it, draw j of the episode = u[j]."""
import types

import numpy as np

from tests import sprite_env_ref as R

F = np.float32
KINDS = ("colour", "shape", "scale")
UNSEEN = (None, "train", "test")


def spec(lo=4, hi=4, colors=(0, 1), shapes=(0, 1), scales=(0.15,), obj_comp=False, unseen_mode=None, unseen_colors=(0, 0), **kw):
    """the task's numbers, defaults = configs/env/odd-one-out-N4C2S2S1.yaml; the other keys are sprite_env_ref.spec's"""
    s = R.spec(lo=lo, hi=hi, colors=colors, shapes=shapes, scales=scales, **kw)
    s.obj_comp, s.unseen_mode, s.unseen_colors = bool(obj_comp), UNSEEN.index(unseen_mode), tuple(unseen_colors)
    return s


def spec_from_desc(d):
    """the same from an ocrl_amd._lib.SpriteEnvDesc of task 1"""
    s = R.spec_from_desc(d)
    s.obj_comp, s.unseen_mode, s.unseen_colors = bool(d.obj_comp), d.unseen_mode, tuple(d.unseen_colors)
    return s


def _fill(st, todo, A, out):
    """rule 6: the objects of ``todo`` (indices in order) take values of A in groups of at least two"""
    todo = list(todo)
    while todo:
        v = A[st.below(len(A))]
        g = 2 + st.below(len(todo) - 1)
        for _ in range(g):
            out[todo.pop(st.below(len(todo)))] = v
        if len(todo) == 1:
            out[todo.pop()] = v


def objects(s, st):
    """rules 1 to 6 on the stream st -> (n, target, unique kind, [colours, shapes, scales] of the n objects)"""
    lists = (list(s.colors), list(s.shapes), list(s.scales))
    n = s.lo + st.below(s.hi - s.lo + 1)
    target = 0 if s.unseen_mode else st.below(n)
    kinds = [K for K in range(3) if len(lists[K]) > 1]
    T = kinds[st.below(len(kinds))]
    u = s.unseen_colors[st.below(2)] if s.unseen_mode == 2 else lists[T][st.below(len(lists[T]))]
    prop = [[None] * n for _ in range(3)]
    prop[T][target] = u
    if s.obj_comp:
        for K in range(3):
            if K != T:
                prop[K] = [lists[K][st.below(len(lists[K]))]] * n
    for K in range(3):
        if K != T:
            if not s.obj_comp:
                _fill(st, range(n), lists[K], prop[K])
            continue
        A = [v for v in lists[K] if v != u]
        if s.unseen_mode and u in s.unseen_colors:
            other = s.unseen_colors[1] if u == s.unseen_colors[0] else s.unseen_colors[0]
            A = [v for v in A if v != other] if s.unseen_mode == 1 else [other]
        _fill(st, [i for i in range(n) if i != target], A, prop[K])
    return n, target, T, prop


def place(s, st, n, scales):
    """rule 7, the Target episode's placement: boxes, candidates, restarts and thresholds of sprite_env_ref.reset -> (px, py)"""
    ax, ay = R.agent_start(s)
    ra = F(s.agent[2] * F(0.5))
    px, py = [F(0)] * n, [F(0)] * n
    for attempt in range(R.RESTARTS + 1):
        dead = False
        for i in range(n):
            b = R.box(s.mode, n, i)
            r = F(scales[i] * F(0.5))
            ok = False
            for _ in range(R.CANDIDATES):
                x = R._pos(st, s.mode, b[0], b[1], r, s.dist_wall)
                y = R._pos(st, s.mode, b[2], b[3], r, s.dist_wall)
                ok = True
                for j in range(i):
                    thr = F(0.15) if s.occlusion else F(F(r + F(scales[j] * F(0.5))) + s.dist_objs)
                    if R.dist(px[j], py[j], x, y) < thr:
                        ok = False
                thr = F(0.15) if s.occlusion else F(F(r + ra) + s.dist_agent)
                if R.dist(ax, ay, x, y) < thr:
                    ok = False
                if ok:
                    break
            px[i], py[i] = x, y
            if not ok and attempt < R.RESTARTS:
                dead = True
                break
        if not dead:
            break
    return px, py


def reset(s, u, with_property_draws=False):
    """one episode from the uniforms u -> (rows [hi + 1, 5] fp32, n, target, unique kind, draws used)"""
    st = R._Stream(u)
    n, target, kind, prop = objects(s, st)
    before_positions = st.j
    px, py = place(s, st, n, prop[2])
    rows = np.zeros((s.hi + 1, 5), dtype=np.float32)
    for i in range(n):
        rows[i] = (prop[0][i], prop[1][i], prop[2][i], px[i], py[i])
    ax, ay = R.agent_start(s)
    rows[n] = (s.agent[0], s.agent[1], s.agent[2], ax, ay)
    out = (rows, n, target, kind, st.j)
    return out + (before_positions,) if with_property_draws else out


class Env(R.Env):
    """one Odd-One-Out environment: sprite_env_ref.Env (the step is the base task's) whose episodes are made by ``reset`` above"""

    def new_episode(self):
        self.episode += 1
        self.rows, self.n, self.target, self.unique_kind, _ = reset(self.s, self.uniforms(self.episode))
        self.step_count, self.ep_return, self.ep_length = 0, 0.0, 0


def check_episode(s, rows, n, target, kind):
    """the task's invariants on one episode's rows, independent of how they were made; raises AssertionError"""
    lists = (list(s.colors), list(s.shapes), [F(z) for z in s.scales])
    assert s.lo <= n <= s.hi and 0 <= target < n and kind in range(3) and len(lists[kind]) > 1
    if s.unseen_mode:
        assert target == 0 and kind == 0
    for K in range(3):
        col = [F(v) for v in rows[:n, K]]
        assert all(v in [F(a) for a in lists[K]] for v in col), (K, col)
        counts = {v: col.count(v) for v in col}
        if K == kind:
            assert counts[col[target]] == 1, (K, col, target)
            assert all(c >= 2 for v, c in counts.items() if v != col[target]), (K, col)
        else:
            assert all(c >= 2 for c in counts.values()), (K, col)
            if s.obj_comp:
                assert len(counts) == 1, (K, col)
    if s.unseen_mode:
        pair, u = {F(c) for c in s.unseen_colors}, F(rows[target, 0])
        others = {F(v) for i, v in enumerate(rows[:n, 0]) if i != target}
        if s.unseen_mode == 1:
            assert not (u in pair and others & pair), (u, others)
        else:
            assert u in pair and others == pair - {u}, (u, others)
