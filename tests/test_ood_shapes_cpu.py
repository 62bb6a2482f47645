"""CPU-only checks of the two out-of-distribution shapes, star_5 (id 7) and spoke_4 (id 9): the Python surface and the library's
validation accept them and still refuse every other name and id, the shape-OOD configs compose, and the numpy restatement the GPU
tests hold the kernels to (tests/ood_shapes_ref.py) is the geometry it claims to be.

Bounds.  Areas: 2 % of 2.314 r^2 and 3.36 r^2 at H = 512, one sprite centred, at both scales (a pixel count differs from the
area by a share of the pixels on the outline; the cross at scale 0.15, whose bars are 30.72 pixels wide, comes within 1.9 %).  The polygon and utils.data._mask comparisons leave out
pixels within 1e-5 of an edge (the float64 margin of the restatement) and are exact elsewhere.  The share of such pixels in the GPU
render test's rows is capped at 1e-3, the cap that test asserts."""
import ctypes
import os

import numpy as np
import pytest

from ocrl_amd import envs
from ocrl_amd.utils.config import compose
from tests import ood_shapes_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
F = np.float32
BASE = ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "num_envs=16", "device=cuda:0"]
OTHER_NAMES = ["pentagon", "hexagon", "octagon", "star_6", "spoke_5", "spoke_6"]
ENV_FILES = {   # file -> (name, COLORS, SHAPES, num_objects_range, obj_comp)
    "odd-one-out-N4C2S2S1-ood-ocr-shape1": ("OddOneOutN4C2S2S1Env", ["blue", "green"], ["star_5", "triangle"], [4, 4], False),
    "odd-one-out-N4C2S2S1-ood-ocr-shape2": ("OddOneOutN4C2S2S1Env", ["blue", "green"], ["star_5", "spoke_4"], [4, 4], False),
    "odd-one-out-N4C2S2S1-oc-ood-ocr-shape1": ("OddOneOutN4C2S2S1Env", ["blue", "green"], ["star_5", "triangle"], [4, 4], True),
    "odd-one-out-N4C2S2S1-oc-ood-ocr-shape2": ("OddOneOutN4C2S2S1Env", ["blue", "green"], ["star_5", "spoke_4"], [4, 4], True),
    "odd-one-out-N4C2S2S1-ood-ocr-color2-shape2": ("OddOneOutN4C2S2S1UnseenEnv", ["cyan", "pink"], ["star_5", "spoke_4"], [4, 4], False),
    "odd-one-out-N6C2S2S1-ood-ocr-color2-shape2": ("OddOneOutN6C2S2S1UnseenEnv", ["cyan", "pink"], ["star_5", "spoke_4"], [6, 6], False),
    "odd-one-out-N4C3S1S1-ood-ocr-color3-shape1": ("OddOneOutN4C3S1S1UnseenEnv", ["brown", "cyan", "pink"], ["star_5"], [4, 4], False),
    "odd-one-out-N6C3S1S1-ood-ocr-color3-shape1": ("OddOneOutN6C3S1S1UnseenEnv", ["brown", "cyan", "pink"], ["star_5"], [6, 6], False),
}
DATASET_FILES = ["odd-one-out-N4C2S2S1-ood-ocr-shape2", "odd-one-out-N4C2S2S1-ood-ocr-color2-shape2"]


def cfg(env, **over):
    return compose(CFG, "train_sb3", BASE + [f"env={env}"] + [f"{k}={v}" for k, v in over.items()])


# ---------------------------------------------------------------------------------------------------------------- 1, 2. the names
def test_env_desc_accepts_star_5_and_spoke_4_everywhere_a_shape_is_named():
    assert envs.sprite.DRAWN_SHAPES == ["square", "triangle", "star_4", "circle", "star_5", "spoke_4"]
    assert envs.sprite.SHAPES.index("star_5") == 7 and envs.sprite.SHAPES.index("spoke_4") == 9
    d = envs.env_desc(cfg("target-N4C4S3S1", **{"env.SHAPES": "[star_5,spoke_4,square]", "env.AGENT": "[red,spoke_4,0.15]",
                                                "env.target": "[blue,star_5,0.15]"}).env, 4)
    assert list(d.shapes)[:d.n_shapes] == [7, 9, 0] and d.agent_shape == 9 and d.target_shape == 7
    d = envs.env_desc(cfg("target-N4C4S3S1", **{"env.AGENT": "[red,star_5,0.15]", "env.target": "[blue,spoke_4,0.15]"}).env, 4)
    assert d.agent_shape == 7 and d.target_shape == 9 and list(d.shapes)[:d.n_shapes] == [0, 1, 2]
    d = envs.env_desc(cfg("odd-one-out-N4C2S2S1", **{"env.SHAPES": "[spoke_4,star_5]"}).env, 4)
    assert list(d.shapes)[:d.n_shapes] == [9, 7] and d.agent_shape == 3


@pytest.mark.parametrize("name", OTHER_NAMES)
def test_the_six_other_names_are_still_refused_by_name(name):
    for env, over in (("target-N4C4S3S1", {"env.SHAPES": f"[square,{name}]"}), ("target-N4C4S3S1", {"env.AGENT": f"[red,{name},0.15]"}),
                      ("target-N4C4S3S1", {"env.target": f"[blue,{name},0.15]"}), ("odd-one-out-N4C2S2S1", {"env.SHAPES": f"[star_5,{name}]"})):
        with pytest.raises(ValueError, match=name):
            envs.env_desc(cfg(env, **over).env, 4)


# ---------------------------------------------------------------------------------------------------------------- 3. the library
def test_the_library_accepts_ids_7_and_9_and_rejects_every_other_id_above_3():
    from ocrl_amd import _lib
    L = _lib.lib()
    assert L.ocrl_abi_version() == 5

    def floats(**fields):
        d = envs.env_desc(cfg("target-N4C4S3S1").env, 4)
        for k, v in fields.items():
            if k == "shape1":
                d.shapes[1] = v
            else:
                setattr(d, k, v)
        return L.ocrl_sprite_env_state_floats(ctypes.byref(d))
    for good in (0, 1, 2, 3, 7, 9):
        for field in ("shape1", "target_shape", "agent_shape"):
            assert floats(**{field: good}) > 0, (field, good)
    for bad in (4, 5, 6, 8, 10, 11, 12, -1):
        for field in ("shape1", "target_shape", "agent_shape"):
            assert floats(**{field: bad}) == 0, (field, bad)
            assert f"shape id {bad} " in L.ocrl_last_error().decode(), (field, bad, L.ocrl_last_error().decode())


# ---------------------------------------------------------------------------------------------------------------- 4. the configs
@pytest.mark.parametrize("file", list(ENV_FILES))
def test_an_env_config_composes_and_is_accepted(file):
    name, colors, shapes, n_range, obj_comp = ENV_FILES[file]
    c = cfg(file).env
    plain = cfg("odd-one-out-N4C2S2S1").env
    assert (c.name, c.env, list(c.COLORS), list(c.SHAPES), list(c.SCALES), list(c.num_objects_range)) == (name, "OddOneOutEnv", colors, shapes, [0.15], n_range)
    assert bool(c.get("obj_comp", False)) == obj_comp and c.get("unseen_combi_mode", None) is None
    own = {"name", "COLORS", "SHAPES", "num_objects_range", "obj_comp"}
    rest = lambda x: {k: v for k, v in x.to_dict().items() if k not in own}
    assert rest(c) == rest(plain)                                                                          # the base file's defaults otherwise
    d = envs.env_desc(c, 8)
    ids = [envs.sprite.SHAPES.index(s) for s in shapes]
    assert (d.task, list(d.shapes)[:d.n_shapes], d.lo, d.hi, d.obj_comp, d.unseen_mode, d.agent_shape) == (1, ids, n_range[0], n_range[1], int(obj_comp), 0, 3)
    assert list(d.colors)[:d.n_colors] == [envs.sprite.COLORS.index(x) for x in colors]
    from ocrl_amd import _lib
    assert _lib.lib().ocrl_sprite_env_state_floats(ctypes.byref(d)) > 0, _lib.lib().ocrl_last_error().decode()


@pytest.mark.parametrize("file", DATASET_FILES)
def test_a_dataset_config_composes_onto_its_env_file(file):
    c = compose(CFG, "train_ocr", ["ocr=vae", f"dataset={file}"]).dataset
    like = compose(CFG, "train_ocr", ["ocr=vae", "dataset=odd-one-out-N4C2S2S1"]).dataset
    assert c.on_device is True and c.tags == file and c.only_initial is True and c.name != like.name
    rest = lambda x: {k: v for k, v in x.to_dict().items() if k not in ("name", "tags", "task")}
    assert rest(c) == rest(like)
    assert c.task.to_dict() == cfg(file).env.to_dict()
    d = envs.env_desc(c.task, 1)
    assert list(d.shapes)[:d.n_shapes] == [7, 9]


# ---------------------------------------------------------------------------------------------------------------- 5. the restatement
def centred(shape, H=512, scale=0.22, dtype=np.float32):
    T = dtype
    lin = (np.arange(H).astype(T) + T(0.5)) / T(H)
    xx, yy = np.meshgrid(lin, lin)
    r = T(T(scale) * T(0.5))
    return xx - T(0.5), yy - T(0.5), r


@pytest.mark.parametrize("scale", [0.15, 0.22])
def test_the_restated_star_is_the_ten_vertex_polygon(scale):
    dx, dy, r = centred(7, scale=scale)
    m = S.covers(7, dx, dy, r)
    area = m.sum() / 512 ** 2 / float(r) ** 2
    print(f"star_5 scale {scale}: area {area:.4f} r^2 (polygon {S.STAR5_AREA:.4f})")
    assert abs(area - 2.314) <= 0.02 * 2.314
    assert np.array_equal(m, S.covers(7, -dx, dy, r)) and np.array_equal(m, m[:, ::-1])                   # the mirror dx -> -dx
    assert not np.array_equal(m, m[::-1])                                                                 # and no mirror in y
    up, down = S.covers(7, np.array([F(0)]), np.array([F(-1.2) * r]), r), S.covers(7, np.array([F(0)]), np.array([F(1.2) * r]), r)
    assert up[0] and not down[0]                                                                          # the tip points up
    # the predicate's five triangles against the polygon's own edges, away from the edges
    x64, y64, r64 = centred(7, scale=scale, dtype=np.float64)
    sure = S.margin(7, x64, y64, float(r64)) >= 1e-5
    assert np.array_equal(m[sure], S.in_polygon(S.star5_polygon(float(r64)), x64, y64)[sure]) and sure.mean() > 0.999
    # every tip and every notch: just inside them covered, just outside not
    poly = S.star5_polygon(float(r64))
    for k, (vx, vy) in enumerate(poly):
        for f, want in ((0.98, True), (1.02, False)):
            got = S.covers(7, np.array([F(vx * f)]), np.array([F(vy * f)]), r)[0]
            assert got == want, (k, f)


@pytest.mark.parametrize("scale", [0.15, 0.22])
def test_the_restated_cross_has_its_area_and_its_symmetry(scale):
    dx, dy, r = centred(9, scale=scale)
    m = S.covers(9, dx, dy, r)
    area = m.sum() / 512 ** 2 / float(r) ** 2
    print(f"spoke_4 scale {scale}: area {area:.4f} r^2")
    assert abs(area - 3.36) <= 0.02 * 3.36
    assert np.array_equal(m, S.covers(9, dy, dx, r)) and np.array_equal(m, m.T)                           # dx and dy swapped
    rr = float(r)
    for (x, y), want in (((0.0, 1.2), True), ((1.2, 0.0), True), ((0.39, -1.24), True), ((0.41, 0.41), False), ((0.0, 1.26), False), ((0.41, 1.0), False)):
        assert S.covers(9, np.array([F(x * rr)]), np.array([F(y * rr)]), r)[0] == want, (x, y)


def test_the_restatement_keeps_the_four_old_shapes_and_the_drawn_row_rule():
    from tests import sprite_env_ref as R
    dx, dy, r = centred(0, H=64)
    for shape in range(4):
        assert np.array_equal(S.covers(shape, dx, dy, r), R.covers(shape, dx, dy, r))
    row = lambda c, h, z: np.array([c, h, z, 0.5, 0.5], dtype=np.float32)
    assert [h for h in range(-1, 14) if S.drawn(row(0, h, 0.15))] == [0, 1, 2, 3, 7, 9]
    assert not S.drawn(row(-1, 7, 0.15)) and not S.drawn(row(7, 7, 0.15)) and not S.drawn(row(0, 9, 0.0)) and S.drawn(row(6, 9, 0.22))
    rows = np.stack([row(0, 7, 0.22), row(1, 5, 0.22), row(2, 9, 0.15)])
    img, masks = S.render(rows, 64)
    assert masks[0].any() and not masks[1].any() and masks[2].any() and masks.shape == (4, 64, 64, 1)
    assert tuple(img[32, 32]) == (255, 255, 0) and tuple(img[24, 32]) == (0, 0, 255)                      # the cross over the star's centre; the star's upper tip
    assert tuple(img[40, 32]) == (0, 0, 0) and not masks[0, 40, 32]                                       # no tip points down


# ---------------------------------------------------------------------------------------------------------------- 6. utils.data._mask
@pytest.mark.parametrize("shape", [7, 9])
def test_the_host_side_mask_is_the_same_definition(shape):
    from ocrl_amd.utils.data import _mask
    rs = np.random.RandomState(5)
    for H in (36, 64, 512):
        lin = (np.arange(H) + 0.5) / H
        xx, yy = np.meshgrid(lin, lin)
        for scale in (0.15, 0.22):
            cx, cy = rs.uniform(0.2, 0.8, size=2)
            r = scale / 2
            got = _mask(shape, xx, yy, cx, cy, r)
            want = S.covers(shape, xx - cx, yy - cy, np.float64(r))
            sure = S.margin(shape, xx - cx, yy - cy, r) >= 1e-5
            assert got.dtype == bool and got.any() and np.array_equal(got[sure], want[sure]) and sure.mean() > 0.999
            want32 = S.covers(shape, (xx - cx).astype(np.float32), (yy - cy).astype(np.float32), np.float32(r))
            assert np.array_equal(got[sure], want32[sure])
    # the pre-training scenes still draw the first four shapes from the same stream
    from ocrl_amd.utils.data import random_sprite_scenes
    _, objs = random_sprite_scenes(8, 16, seed=3, with_objs=True)
    assert set(objs[..., 1].ravel().tolist()) <= {0.0, 1.0, 2.0, 3.0}


# ---------------------------------------------------------------------------------------------------------------- 7. the margin's share
@pytest.mark.parametrize("H", S.RENDER_H)
@pytest.mark.parametrize("E", S.RENDER_E)
def test_few_pixels_of_the_gpu_render_tests_rows_lie_within_1e_5_of_an_edge(E, H):
    rows = S.render_case(E)
    assert rows.shape == (E, 16, 5)
    left_out = 0
    for e in range(E):
        ids, scales = rows[e, :, 1], rows[e, :, 2]
        assert set(S.DRAWN_IDS) <= set(ids.tolist()) and {F(0.15), F(0.22)} <= set(scales.tolist())
        for h in (7, 9):
            assert {F(0.15), F(0.22)} <= set(scales[(ids == h) & (rows[e, :, 0] >= 0)].tolist())
        assert rows[e, S.ID5_ROW, 1] == 5 and (rows[e, :, 0] == -1).any() and not rows[e, 15].any()
        assert rows[e, S.STAR_ROW, 1] == 7 and rows[e, S.SPOKE_ROW, 1] == 9
        img, masks, marg = S.render(rows[e], H, np.float32, with_margin=True)
        left_out += int((marg < 1e-5).sum())
        assert not masks[S.ID5_ROW].any() and masks[S.STAR_ROW].any() and masks[S.SPOKE_ROW].any()
        assert (masks[10].any() and masks[11].any()) or H == 16                                           # the sprites cut by the frame edge
        assert ((masks[6:10].sum(0) > 1).any())                                                           # the cluster overlaps
    share = left_out / (E * H * H)
    print(f"E{E} H{H}: {left_out} of {E * H * H} pixels within 1e-5 of an edge ({share:.2e})")
    assert share <= 1e-3
