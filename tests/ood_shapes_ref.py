"""numpy restatement of the renderer with the two out-of-distribution shapes (ocrl_amd/csrc/sprite_shapes.h: sprite_row_drawn,
sprite_covers with ids 7 star_5 and 9 spoke_4), written from the geometry, in the dtype of its arguments: with np.float32 it follows
the kernel's operations one rounding at a time (numpy rounds every operation and never fuses).  Ids 0..3 are tests/sprite_env_ref.py's.

The geometry (r = scale / 2; up is -y).  star_5: the ten-vertex star polygon with tips at radius 1.25 r, 72 degrees apart from straight
up, and notches at 0.63 r halfway between them (``star5_polygon``; ``in_polygon`` is an independent float64 test of it).  The predicate
is the union of five triangles, one per tip, in the tip's frame (a along its axis, b the distance from the axis): the apex at a = 1.25 r,
the sides through the two neighbouring notches (a, b) = 0.63 r (cos 36, +-sin 36), cut off at a = 0.  spoke_4: an upright Greek cross of
two bars, half width 0.4 r, half length 1.25 r."""
import numpy as np

from tests import sprite_env_ref as R

DRAWN_IDS = (0, 1, 2, 3, 7, 9)
# (sin, cos) of the tips' angles 0, 72, 144, 216, 288 degrees from straight up, and 0.63 * (cos 36, sin 36), as the header writes them
STAR5_TIPS = ((0.0, 1.0), (0.95105654, 0.309017), (0.58778524, -0.809017), (-0.58778524, -0.809017), (-0.95105654, 0.309017))
STAR5_AN, STAR5_BN = 0.5096807, 0.3703047
STAR5_AREA, SPOKE4_AREA = 5 * 1.25 * 0.63 * np.sin(np.radians(36.0)), 3.36         # in units of r^2


def _star5_slacks(dx, dy, r):
    """per tip: (a, bn (tip - a) - b run), the two comparisons' slacks (>= 0: satisfied), in the dtype of r"""
    T = type(r)
    ny, tip, an, bn = -dy, T(1.25) * r, T(STAR5_AN) * r, T(STAR5_BN) * r
    run = tip - an
    out = []
    for s, c in STAR5_TIPS:
        a = dx * T(s) + ny * T(c)
        b = np.abs(dx * T(c) - ny * T(s))
        out.append((a, b * run, bn * (tip - a)))
    return out


def covers(shape, dx, dy, r):
    """arrays dx, dy = pixel centre - sprite centre; scalar r (np.float32 or np.float64: the arithmetic's dtype)"""
    if shape == 7:
        m = np.zeros(np.shape(dx), dtype=bool)
        for a, lhs, rhs in _star5_slacks(dx, dy, r):
            m |= (a >= 0) & (lhs <= rhs)
        return m
    if shape == 9:
        T = type(r)
        ax, ay, w, l = np.abs(dx), np.abs(dy), T(0.4) * r, T(1.25) * r
        return ((ax <= w) & (ay <= l)) | ((ay <= w) & (ax <= l))
    return R.covers(shape, dx, dy, r)


def margin(shape, dx, dy, r):
    """float64: how far each pixel's decision is from flipping, as tests/sprite_env_ref.py:margin has it for one conjunction.  A tip's
    triangle or a bar is a conjunction of comparisons with slacks s_i (>= 0: satisfied), covered when min_i s_i >= 0; the shape is
    their union, covered when V = max_k min_i s_ki >= 0.  Moving every slack by less than |V| leaves the sign of V as it is, so |V| is
    the margin: a comparison of a triangle that another one overrules does not count.  The slacks are lengths in frame units; the
    star's side comparison is divided by r, which is 0.83 of the distance to the side (the smaller figure)."""
    if shape == 7:
        v = np.full(np.shape(dx), -np.inf)
        for a, lhs, rhs in _star5_slacks(dx, dy, np.float64(r)):
            v = np.maximum(v, np.minimum(a, (rhs - lhs) / r))
        return np.abs(v)
    if shape == 9:
        ax, ay, w, l = np.abs(dx), np.abs(dy), 0.4 * r, 1.25 * r
        return np.abs(np.maximum(np.minimum(w - ax, l - ay), np.minimum(w - ay, l - ax)))
    return R.margin(shape, dx, dy, r)


def drawn(row):
    """the painted rows: a colour in 0..6, a drawn shape id (the value truncated) and a scale > 0"""
    return 0 <= row[0] < 7 and 0 <= row[1] < 10 and int(row[1]) in DRAWN_IDS and row[2] > 0


def render(rows, H, dtype=np.float32, with_margin=False):
    """rows [R, 5] -> (image uint8 [H, H, 3], masks uint8 [R + 1, H, H, 1]) with the arithmetic in ``dtype``, painted in row order;
    with_margin adds the float64 decision margin of every pixel over the drawn rows [H, H]"""
    T = dtype
    lin = (np.arange(H).astype(T) + T(0.5)) / T(H)
    xx, yy = np.meshgrid(lin, lin)
    l64 = (np.arange(H) + 0.5) / H
    x64, y64 = np.meshgrid(l64, l64)
    R_ = rows.shape[0]
    img = np.zeros((H, H, 3), dtype=np.uint8)
    masks = np.zeros((R_ + 1, H, H, 1), dtype=np.uint8)
    marg = np.full((H, H), np.inf)
    for j in range(R_):
        if not drawn(rows[j]):
            continue
        cx, cy, r = T(rows[j, 3]), T(rows[j, 4]), T(T(rows[j, 2]) * T(0.5))
        m = covers(int(rows[j, 1]), xx - cx, yy - cy, r)
        img[m] = R.COLOR_BYTES[int(rows[j, 0])]
        masks[j, :, :, 0] = m
        if with_margin:
            marg = np.minimum(marg, margin(int(rows[j, 1]), x64 - float(rows[j, 3]), y64 - float(rows[j, 4]), float(rows[j, 2]) * 0.5))
    masks[R_, :, :, 0] = masks[:R_].sum(0)[:, :, 0] == 0
    return (img, masks, marg) if with_margin else (img, masks)


# ---------------------------------------------------------------------------------------------------------------- the polygon itself
def star5_polygon(r):
    """the ten vertices (dx, dy) in order round the star, float64: tip 0 straight up (-y), then notch, tip, .."""
    k = np.arange(10)
    rad = np.where(k % 2 == 0, 1.25 * r, 0.63 * r)
    ang = np.radians(36.0 * k)
    return np.stack([rad * np.sin(ang), -rad * np.cos(ang)], axis=1)


def in_polygon(poly, dx, dy):
    """even-odd crossing test of the points (dx, dy) against the polygon's edges, float64; no use of the predicate's form"""
    inside = np.zeros(np.shape(dx), dtype=bool)
    for (x0, y0), (x1, y1) in zip(poly, np.roll(poly, -1, axis=0)):
        between = (y0 > dy) != (y1 > dy)
        with np.errstate(divide="ignore", invalid="ignore"):
            xc = x0 + (dy - y0) * (x1 - x0) / (y1 - y0)
        inside ^= between & (dx < xc)
    return inside


# ---------------------------------------------------------------------------------------------------------------- the GPU render test's rows
STAR_ROW, SPOKE_ROW, ID5_ROW = 4, 5, 13
RENDER_E, RENDER_H = (1, 5), (16, 36, 64)


def hand_rows(e):
    """rows [16, 5] of hand-placed sprites at fixed-seed random centres: all six drawn ids at both scales, a cluster of overlapping
    sprites, sprites cut by the frame edge, a row of colour -1, a row of shape id 5 (row ``ID5_ROW``: it must stay blank), the agent and
    zero padding rows.  Rows ``STAR_ROW`` and ``SPOKE_ROW`` hold an id-7 and an id-9 sprite inside the frame."""
    rs = np.random.RandomState(700 + e)
    rows = np.zeros((16, 5), dtype=np.float32)
    for i, h in enumerate(DRAWN_IDS):                                                   # rows 0..5: each id once, scales alternating
        rows[i] = (rs.randint(7), h, (0.15, 0.22)[(i + e) % 2], rs.uniform(0.15, 0.85), rs.uniform(0.15, 0.85))
    cx, cy = rs.uniform(0.3, 0.7, size=2)
    for i, h in enumerate((7, 9, 2, 7)):                                                # rows 6..9: overlapping, the other scale for 7 and 9
        rows[6 + i] = (i, h, (0.22, 0.15)[(i + e) % 2], cx + rs.uniform(-0.04, 0.04), cy + rs.uniform(-0.04, 0.04))
    rows[10] = (4, 7, 0.22, rs.uniform(0.0, 0.03), rs.uniform(0.2, 0.8))                # cut by the left edge
    rows[11] = (5, 9, 0.22, rs.uniform(0.3, 0.7), rs.uniform(0.97, 1.0))                # cut by the lower edge
    rows[12] = (-1, 7, 0.22, rs.uniform(0.2, 0.8), rs.uniform(0.2, 0.8))
    rows[ID5_ROW] = (6, 5, 0.22, rs.uniform(0.2, 0.8), rs.uniform(0.2, 0.8))
    rows[14] = (3, 3, 0.15, rs.uniform(0.075, 0.925), rs.uniform(0.075, 0.925))          # the agent; row 15 stays zero
    return rows


def render_case(E):
    """the rows [E, 16, 5] of the GPU render test for E environments"""
    return np.stack([hand_rows(e) for e in range(E)])
