"""GPU checks of the two out-of-distribution shapes, star_5 (id 7) and spoke_4 (id 9), through every entry point that paints a row:
ocrl_sprite_render, the vectorised environment on a shape-OOD config, and the task datasets (ocrl_task_scenes_batch, the rollout form,
get_dataloaders), against the numpy restatement of tests/ood_shapes_ref.py.

Bounds.  Frames and masks: byte for byte against the fp32 restatement, except pixels whose float64 decision margin to some sprite's
edge is below 1e-5 (two correct fp32 evaluations may order the operations of a predicate differently there); those are left out and
must be at most 0.1 % of the pixels compared (tests/test_ood_shapes_cpu.py holds the render test's rows to the same cap without a GPU).
Everything else is exact: an observation against render_rows of the state's own rows, and the environment on star_5 / spoke_4 against
the environment on square / triangle, which draws the same indices into its lists: identical but for the shape column."""
import numpy as np
import pytest
import torch

from ocrl_amd.utils.config import compose
from tests import ood_shapes_ref as S
from tests.gpu_util import log
from tests.test_gpu_task_scenes import CFG, DEV, generate, raw_rows

pytestmark = pytest.mark.gpu

BASE = ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "device=cuda:0"]
OOD, PLAIN = "odd-one-out-N4C2S2S1-ood-ocr-shape2", "odd-one-out-N4C2S2S1"
BYTES = {"blue": (0, 0, 255), "green": (0, 255, 0), "red": (255, 0, 0), "cyan": (0, 255, 255), "pink": (255, 192, 203)}


def config(env, *over):
    return compose(CFG, "train_sb3", BASE + [f"env={env}"] + list(over))


def make(env, E, seed, *over):
    from ocrl_amd import envs
    return envs.make_env(config(env, *over), num_envs=E, seed=seed, device="cuda")


def compare_with_the_restatement(rows, H, hwc, masks):
    """rows [B, R, 5], frames [B, H, H, 3] and mask planes [B, R + 1, H, H] (or None) as numpy -> pixels left out; asserts the rest"""
    left_out = 0
    for e in range(rows.shape[0]):
        img, msk, marg = S.render(rows[e], H, np.float32, with_margin=True)
        sure = marg >= 1e-5
        left_out += int((~sure).sum())
        assert np.array_equal(hwc[e][sure], img[sure]), e
        if masks is not None:
            assert np.array_equal(masks[e][:, sure], msk[..., 0][:, sure]), e
    return left_out


# ---------------------------------------------------------------------------------------------------------------- 1. the renderer
@pytest.mark.parametrize("H", S.RENDER_H)
@pytest.mark.parametrize("E", S.RENDER_E)
def test_render_equals_the_restatement(E, H):
    env = make(OOD, 1, 0, f"env.obs_size={H}")
    rows = S.render_case(E)
    dev = torch.from_numpy(rows)
    chw, hwc, masks = (env.render_rows(dev, m).cpu().numpy() for m in ("image", "rgb_array", "mask"))
    assert chw.shape == (E, 3, H, H) and hwc.shape == (E, H, H, 3) and masks.shape == (E, 17, H, H, 1)
    assert np.array_equal(chw, hwc.transpose(0, 3, 1, 2))
    left_out = compare_with_the_restatement(rows, H, hwc, masks[..., 0])
    share = left_out / (E * H * H)
    log(f"ood render E{E} H{H}: {left_out} of {E * H * H} pixels within 1e-5 of an edge ({share:.2e})")
    assert share <= 1e-3
    assert masks.max() == 1 and (masks[:, :-1].sum(1) + masks[:, -1] >= 1).all()
    # the modes agree: a pixel's colour is that of the last row whose plane covers it, black where the background plane is set
    top = np.zeros((E, H, H, 3), dtype=np.uint8)
    for j in range(16):
        colour = np.array([S.R.COLOR_BYTES[int(c)] if 0 <= c < 7 else (0, 0, 0) for c in rows[:, j, 0]], dtype=np.uint8)
        top = np.where(masks[:, j] == 1, colour[:, None, None, :], top)
    assert np.array_equal(top, hwc) and np.array_equal(masks[:, -1, :, :, 0] == 1, ~hwc.any(-1))
    for e in range(E):
        assert not masks[e, S.ID5_ROW].any() and masks[e, S.STAR_ROW].any() and masks[e, S.SPOKE_ROW].any()
        assert not masks[e, 12].any() and not masks[e, 15].any()                       # the -1 colour row and the padding row


# ---------------------------------------------------------------------------------------------------------------- 2. the environment
def test_the_environment_on_unseen_shapes_is_the_plain_one_but_for_the_shape_column():
    E, seed, H, T = 8, 23, 32, 20
    over = (f"env.obs_size={H}", "env.max_steps=6")
    ood, plain, state = make(OOD, E, seed, *over), make(PLAIN, E, seed, *over), make(OOD, E, seed, *over, "env.render_mode=state")
    assert list(ood._desc.shapes)[:2] == [7, 9] and list(plain._desc.shapes)[:2] == [0, 1] and ood._desc.agent_shape == 3

    def check(obs_o, obs_s):
        st_o, st_p = ood.get_state(), plain.get_state()
        rows = st_o["rows"]
        assert torch.equal(obs_o, ood.render_rows(rows)) and obs_o.shape == (E, 3, H, H) and obs_o.dtype == torch.uint8
        shape = rows[..., 1]
        assert ((shape[:, :4] == 7) | (shape[:, :4] == 9)).all() and (shape[:, 4] == 3).all() and (st_o["n"] == 4).all()
        assert torch.equal(obs_s[..., 1], shape) and torch.equal(obs_s[..., 3:], rows[..., 3:]) and torch.equal(state.get_state()["rows"], rows)
        mapped = st_p["rows"].clone()
        mapped[:, :4, 1] = torch.where(mapped[:, :4, 1] == 0, 7.0, 9.0)
        assert set(st_p["rows"][:, :4, 1].unique().tolist()) <= {0.0, 1.0} and torch.equal(mapped, rows)
        for k in st_o:
            if k != "rows":
                assert torch.equal(st_o[k], st_p[k]), k
        return rows
    plain.reset()
    first = check(ood.reset(), state.reset()).clone()
    check(ood.render("image"), state.observe())
    seen = {7: False, 9: False}
    actions = torch.from_numpy(np.random.RandomState(9).randint(0, 4, size=(T, E))).to(DEV)
    finished = 0
    for t in range(T):
        (obs_o, rew_o, done_o, ex_o), (_, rew_p, done_p, ex_p) = ood.step_device(actions[t]), plain.step_device(actions[t])
        obs_s = state.step_device(actions[t])[0]
        assert torch.equal(rew_o, rew_p) and torch.equal(done_o, done_p) and all(torch.equal(ex_o[k], ex_p[k]) for k in ex_o)
        rows = check(obs_o, obs_s)
        finished += int(done_o.sum())
        for h in seen:
            seen[h] |= bool((rows[:, :4, 1] == h).any())
    assert finished >= E and seen[7] and seen[9] and not torch.equal(rows, first)       # auto-resets included: max_steps 6 ends every episode
    colours = {tuple(c) for c in obs_o.permute(0, 2, 3, 1).reshape(-1, 3).cpu().tolist()}
    assert colours <= {(0, 0, 0), BYTES["blue"], BYTES["green"], BYTES["red"]} and BYTES["red"] in colours and len(colours) >= 3
    # the frames are the restatement's too
    left = compare_with_the_restatement(rows.cpu().numpy(), H, obs_o.permute(0, 2, 3, 1).cpu().numpy(), ood.render("mask")[..., 0].cpu().numpy())
    assert left <= 1e-3 * E * H * H


# ---------------------------------------------------------------------------------------------------------------- 3. the task scenes
@pytest.mark.parametrize("H", [16, 64])
def test_task_scenes_and_rollouts_paint_the_unseen_shapes(H):
    from ocrl_amd import envs
    from tests.test_gpu_task_rollouts import rollout
    B, seed = 7, 41
    d = envs.env_desc(config(OOD).env, 1)
    d.H = H
    idx = [(e << 24) | 0 for e in range(B)]
    env = make(OOD, B, seed, f"env.obs_size={H}")
    frames = env.reset()
    target = env.get_state()["target"].long()
    first = generate(d, seed, idx)
    later = rollout(d, seed, idx, steps=[0, 1, 2, 3, 5, 8, 13])
    assert torch.equal(first["u8"].permute(0, 3, 1, 2), frames) and torch.equal(raw_rows(first["objs"]), env.get_state()["rows"])
    left_out = 0
    for name, got in (("first frames", first), ("rollout", later)):
        assert torch.equal(got["labels"], target), name
        rows = raw_rows(got["objs"])                                                    # the scale index back to the scale
        shape = rows[..., 1]
        assert ((shape[:, :4] == 7) | (shape[:, :4] == 9)).all() and (shape[:, 4] == 3).all()
        masks = got["masks"].cpu().numpy()
        assert set(np.unique(masks).tolist()) <= {0.0, 1.0}
        if H >= 64:                                                                     # at 16 pixels a cross's bar, 0.96 pixels wide, can miss every centre
            assert masks[:, :5].reshape(B, 5, -1).any(-1).all()
        left_out += compare_with_the_restatement(rows.cpu().numpy(), H, got["u8"].cpu().numpy(), masks.astype(np.uint8))
        assert torch.equal(got["obs"], got["u8"].permute(0, 3, 1, 2).float() / 255.0)
    assert left_out <= 1e-3 * 2 * B * H * H
    taken = later["taken"].cpu().tolist()                                               # a step that would end the episode is not taken
    assert taken[:2] == [0, 1] and all(0 <= a <= b for a, b in zip(taken, [0, 1, 2, 3, 5, 8, 13]))
    assert torch.equal(later["objs"][0], first["objs"][0]) and not torch.equal(later["objs"][1, 4, 3:], first["objs"][1, 4, 3:])
    assert torch.equal(later["objs"][:, :4], first["objs"][:, :4])                      # the walk moves the agent alone


@pytest.mark.parametrize("file,names", [(OOD, ("blue", "green")), ("odd-one-out-N4C2S2S1-ood-ocr-color2-shape2", ("cyan", "pink"))])
def test_the_dataset_configs_yield_frames_of_their_own_colours(file, names):
    from ocrl_amd.utils.datasets import get_dataloaders
    c = compose(CFG, "train_ocr", ["ocr=vae", f"dataset={file}", "dataset.obs_size=32", "dataset.synthetic_train=8", "dataset.synthetic_val=4",
                                   "dataset.with_objs=True", "dataset.with_masks=True"])
    tr, va = get_dataloaders(c.dataset, 4, 0, seed=1, device=DEV)
    for dl in (tr, va):
        b = next(iter(dl))
        assert b["obss"].shape == (4, 3, 32, 32) and b["masks"].shape == (4, 6, 32, 32, 1) and b["objs"].shape == (4, 5, 5)
        colours = {tuple(p) for p in (b["obss"] * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).reshape(-1, 3).cpu().tolist()}
        assert colours <= {(0, 0, 0), BYTES["red"]} | {BYTES[n] for n in names} and colours & {BYTES[n] for n in names} and BYTES["red"] in colours
        assert set(b["objs"][:, :4, 1].unique().tolist()) <= {7.0, 9.0} and (b["objs"][:, 4, 1] == 3).all()
        assert b["masks"][:, :5].flatten(2).any(-1).all()                               # every sprite, stars and crosses included, is seen
