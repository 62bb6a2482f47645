"""numpy restatement of a pre-training scene's objects (include/ocrl_hip.h: ocrl_scenes_batch, "The draws"), written from the rules in
the header, one scene at a time.  Positions follow the kernel's fp32 operations one rounding at a time (np.float32 scalars: numpy rounds
every operation and never fuses), so objs are compared bit for bit.  The restatement draws nothing itself: ``scene`` consumes the
uniforms handed to it (the dump of ocrl_scenes_uniforms, or hand-made ones), draw j of the scene = u[j]."""
import numpy as np

from tests.sprite_env_ref import _Stream, dist

F = np.float32
SCALES = (F(0.15), F(0.22))
CANDIDATES = 64
MAX_DRAWS = 15 * (1 + 2 * CANDIDATES + 2)      # what 15 objects can take at most


def interval(s):
    """[a, b] of a centre coordinate at scale index s, and r"""
    r = F(SCALES[s] * F(0.5))
    return F(r + F(0.08)), F(F(F(1.0) - r) - F(0.08)), r


def scene(u, K=5):
    """one scene from the uniforms u -> (objs [K, 5] fp32 = colour, shape, scale index, x, y; centres [K, 3] fp32 = x, y, real scale;
    draws used; exhausted: the objects, in order, whose 64 candidates were all rejected and whose last one stands)"""
    st = _Stream(u)
    objs = np.zeros((K, 5), dtype=np.float32)
    centres = np.zeros((K, 3), dtype=np.float32)
    exhausted = []
    for k in range(K):
        s = st.below(2)
        a, b, _ = interval(s)
        w = F(b - a)
        ok = False
        for _ in range(CANDIDATES):
            x = F(a + F(w * st.u01()))
            y = F(a + F(w * st.u01()))
            ok = not dist(F(0.5), F(0.5), x, y) < F(0.15)
            for j in range(k):
                if dist(centres[j, 0], centres[j, 1], x, y) < F(0.15):
                    ok = False
            if ok:
                break
        if not ok:
            exhausted.append(k)
        shape = st.below(4)
        colour = st.below(4)
        objs[k] = (colour, shape, s, x, y)
        centres[k] = (x, y, SCALES[s])
    return objs, centres, st.j, exhausted


def rows(objs):
    """objs [..., K, 5] -> the rows ocrl_sprite_render takes: the scale index replaced by the scale"""
    r = np.array(objs, dtype=np.float32, copy=True)
    r[..., 2] = np.where(r[..., 2] == 0, SCALES[0], SCALES[1])
    return r
