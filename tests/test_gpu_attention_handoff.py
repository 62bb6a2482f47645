"""The hand-off form of the causal self-attention backward (csrc/attention.hip: attn_bwd_kv_kernel<DH, true> stores its dS tiles,
attn_bwd_dq_kernel reads them) through ocrl_attention_bwd_ws, against the fp64 reference of tests/attention_ref.py and against the
two-kernel form (OCRL_ATTN_BWD=2 through ocrl_attention_bwd) on the same inputs.

The calls are hostile in the way of tests/test_gpu_attention_edges.py, whose helpers are used here: outputs pre-filled with NaN between
guard words, NaN pad columns and NaN tail rows.  In addition the dS workspace is pre-filled with NaN and sits between guard words: a tile
element that the dQ kernel reads and the dK/dV kernel did not write reaches dq as NaN, a store outside the workspace breaks a guard.

Dropout needs a triangle that can hold both kept and dropped entries (R.non_vacuity): T = 1 (one entry) runs at p = 0 only; T = 3 (six
entries per triangle) runs p = 0.1 at B = h = 1 with a (seed, site) of R's whose one triangle has both."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

from tests import attention_ref as R
from tests import test_gpu_attention_edges as E
from tests.gpu_util import log, relerr

pytestmark = pytest.mark.gpu
P = E.P
TOL = E.TOL
NAN = float("nan")
GRADS = ("dq", "dk", "dv")


def _lib_handle():
    from ocrl_amd import _lib
    return _lib.lib()


class _env:
    """OCRL_ATTN_BWD set to `value` (None: unset) for the duration of a call"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("OCRL_ATTN_BWD")
        if self.value is None:
            os.environ.pop("OCRL_ATTN_BWD", None)
        else:
            os.environ["OCRL_ATTN_BWD"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("OCRL_ATTN_BWD", None)
        else:
            os.environ["OCRL_ATTN_BWD"] = self.old


def ds_floats(B, T, h):
    n = _lib_handle().ocrl_attention_bwd_ds_floats(B, T, h)
    nblk = (T + 63) // 64
    assert n == B * h * (nblk * (nblk + 1) // 2) * 64 * 64          # 64 x 64 tiles of the causal triangle per (image, head)
    return n


def forward(q, k, v, dO, h, layout, p=0.0, seed=0, site=0, into=None):
    """places the inputs as E.run does and runs the forward; `into`: an earlier placement whose buffers are reused for new inputs"""
    from ocrl_amd import _lib
    L = _lib_handle()
    B, T, d = q.shape
    if into is None:
        (qv, kv, vv), ld, _ = E._place(layout, B, T, d, (q, k, v), NAN)
        gall = torch.full((E.HEAD + B * T + E.TAIL + (B * T * (ld - d) + d - 1) // d, d), NAN, device="cuda")
        gbuf = gall[E.HEAD:E.HEAD + B * T]
        f = SimpleNamespace(qv=qv, kv=kv, vv=vv, ld=ld, gall=gall, gbuf=gbuf, o=E.Guarded(B * T * d, extra=B * T * (ld - d)),
                            lse=E.Guarded(B * h * T), B=B, T=T, d=d, h=h, layout=layout)
    else:
        f = into
        for vw, t in zip((f.qv, f.kv, f.vv), (q, k, v)):
            vw.copy_(t.reshape(B * T, d))
    f.p, f.seed, f.site = p, seed, site
    f.gbuf.copy_(dO.reshape(B * T, d))
    _lib.check(L.ocrl_attention_fwd(P(f.qv), P(f.kv), P(f.vv), P(f.o.data), P(f.lse.data), B, T, d, h, f.ld, p, seed, site, None))
    torch.cuda.synchronize()
    assert f.o.guards_intact() and f.lse.guards_intact(), "forward wrote outside o / lse"
    f.o_bits = E._bits(f.o.data.clone())
    return f


def backward(f, env, ws_floats=None, bufs=None):
    """one backward of the placed problem: through ocrl_attention_bwd_ws with a NaN-filled guarded workspace of ws_floats floats, or
    (ws_floats None) through ocrl_attention_bwd.  `bufs`: the buffers of an earlier call, reused as they are (nothing is re-filled).
    Returns ({"dq","dk","dv"} on the CPU, bufs).  Asserts guards, pads, tail rows and that every result is finite."""
    from ocrl_amd import _lib
    L = _lib_handle()
    B, T, d, h = f.B, f.T, f.d, f.h
    if bufs is None:
        gviews, _, gallocs = E._place(f.layout, B, T, d, (NAN, NAN, NAN), E.SENTINEL)
        bufs = SimpleNamespace(gviews=gviews, gallocs=gallocs, delta=E.Guarded(B * h * T),
                               ws=None if ws_floats is None else E.Guarded(max(ws_floats, 4)))
    before = [a.clone() for a in bufs.gallocs]
    gv = bufs.gviews
    with _env(env):
        if ws_floats is None:
            _lib.check(L.ocrl_attention_bwd(P(f.qv), P(f.kv), P(f.vv), P(f.o.data), P(f.lse.data), P(f.gbuf), P(gv[0]), P(gv[1]), P(gv[2]),
                                            P(bufs.delta.data), B, T, d, h, f.ld, f.p, f.seed, f.site, None))
        else:
            _lib.check(L.ocrl_attention_bwd_ws(P(f.qv), P(f.kv), P(f.vv), P(f.o.data), P(f.lse.data), P(f.gbuf), P(gv[0]), P(gv[1]), P(gv[2]),
                                               P(bufs.delta.data), B, T, d, h, f.ld, f.p, f.seed, f.site, P(bufs.ws.data), ws_floats, None))
    torch.cuda.synchronize()
    assert bufs.delta.guards_intact(), "wrote outside delta"
    assert bufs.ws is None or bufs.ws.guards_intact(), "wrote outside the dS workspace"
    assert E._outside_unchanged(gv, bufs.gallocs, d, before), "wrote outside dq / dk / dv (pad column, tail row)"
    assert f.o.guards_intact() and f.lse.guards_intact() and torch.equal(E._bits(f.o.data), f.o_bits), "the backward changed o"
    res = {n: t.reshape(B, T, d).cpu() for n, t in zip(GRADS, gv)}
    for n, t in res.items():
        assert torch.isfinite(t).all(), f"{n} holds a non-finite value (not overwritten, an unwritten dS element, or a pad / tail row)"
    return res, bufs


def same_bits(a, b, names=GRADS):
    return {n: torch.equal(E._bits(a[n]), E._bits(b[n])) for n in names}


def grade(tag, res, ref):
    e = {n: relerr(res[n], ref[n], floor=E.grad_floor(ref)) for n in GRADS}
    log(f"[attention handoff] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    bad = {k: v for k, v in e.items() if not v < TOL}
    assert not bad, (tag, bad)


# (B, T, h, dh, layout): every length of the tile seams (1: the diagonal tile alone; 63 / 64 / 65 and 127 / 128 / 129: one, two and three
# 64-row tiles, ragged and full; 200: four), B in {1, 3}, h in {1, 2, 4}, every head width at one-tile and at multi-tile lengths, the
# three layouts spread over them
SHAPES = [
    (1, 1, 1, 16, "packed"), (3, 1, 2, 48, "padded"), (1, 3, 1, 32, "dense"), (3, 3, 2, 64, "packed"),
    (1, 63, 4, 48, "padded"), (3, 64, 1, 64, "dense"), (1, 65, 2, 16, "padded"), (3, 65, 4, 48, "packed"),
    (3, 127, 4, 32, "packed"), (1, 128, 1, 48, "padded"), (3, 129, 2, 64, "packed"), (3, 129, 4, 48, "dense"), (1, 129, 2, 16, "dense"),
    (3, 200, 4, 48, "dense"), (1, 200, 1, 32, "packed"), (1, 200, 2, 64, "padded"), (3, 200, 2, 16, "packed"),
]
DROPOUT_SHAPES = [s for s in SHAPES if s[1] >= 63 or s[:3] == (1, 3, 1)]
P_DROP = 0.1
_ids = lambda s: "B{}-T{}-h{}-dh{}-{}".format(*s)


def _drop_key(B, T, h):
    """(seed, site, keep): the first of R's seeds (below and above 2^32) and sites, tried from a start that depends on the shape, whose
    mask passes R.non_vacuity"""
    keys = [(seed, site) for seed in (R.SEED_LO, R.SEED_HI) for site in (R.SITE_BLK, R.SITE_POOL)]
    for i in range(len(keys)):
        seed, site = keys[(i + B + T + h) % len(keys)]
        keep = R.keep_mask(seed, site, P_DROP, B, h, T)
        both, share, z = R.non_vacuity(keep, P_DROP)
        if both and z < 5.0:
            return seed, site, keep
    raise AssertionError(f"no non-vacuous dropout mask at B{B} T{T} h{h}")


def _case(shape, p):
    """runs the hand-off form with a whole-batch workspace and the two-kernel form on the same placed inputs: the hand-off form against
    fp64; dk and dv of the two forms bit for bit; dq of the hand-off form is graded against fp64 above and its bitwise agreement logged"""
    B, T, h, dh, layout = shape
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    seed, site, keep = _drop_key(B, T, h) if p > 0 else (0, 0, None)
    ref = R.attention_ref(q, k, v, h, dO, keep, p)
    if p > 0:
        assert relerr(R.attention_ref(q, k, v, h)["o"], ref["o"]) > 1e-2          # the mask moves the result far beyond the tolerance
    f = forward(q, k, v, dO, h, layout, p, seed, site)
    hand, _ = backward(f, None, ds_floats(B, T, h))
    two, _ = backward(f, "2")
    tag = f"p={p} {_ids(shape)}"
    grade(tag + " hand-off", hand, ref)
    grade(tag + " two-kernel", two, ref)
    same = same_bits(hand, two)
    log(f"[attention handoff] {tag}: bitwise against the two-kernel form dq={same['dq']} dk={same['dk']} dv={same['dv']}")
    assert same["dk"] and same["dv"], (tag, same)
    return same["dq"]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_against_fp64_and_two_kernel_form(shape):
    _case(shape, 0.0)


@pytest.mark.parametrize("shape", DROPOUT_SHAPES, ids=_ids)
def test_against_fp64_and_two_kernel_form_with_dropout(shape):
    _case(shape, P_DROP)


@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_chunks_of_two_and_one_image_equal_the_whole_batch(p):
    """B = 3 with a workspace for exactly 2 images (chunks of 2 + 1) and for exactly 1 image (three chunks): bit for bit the results of
    the whole-batch workspace -- the dropout index of a chunk's images must be that of their place in the batch"""
    B, T, h, dh = 3, 129, 2, 48
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    seed, site, keep = _drop_key(B, T, h) if p > 0 else (0, 0, None)
    f = forward(q, k, v, dO, h, "packed", p, seed, site)
    full, _ = backward(f, None, ds_floats(B, T, h))
    grade(f"chunks p={p} whole batch", full, R.attention_ref(q, k, v, h, dO, keep, p))
    per = ds_floats(1, T, h)
    for n in (2 * per, per, 2 * per + per - 1):
        part, _ = backward(f, None, n)
        same = same_bits(full, part)
        assert all(same.values()), (n // per, same)


def test_workspace_below_one_image_is_the_two_kernel_form():
    """one float short of an image: the result is bit for bit OCRL_ATTN_BWD=2 through ocrl_attention_bwd, and the workspace is untouched;
    so is it with a null workspace"""
    B, T, h, dh = 3, 129, 2, 48
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    seed, site, _ = _drop_key(B, T, h)
    f = forward(q, k, v, dO, h, "packed", P_DROP, seed, site)
    two, _ = backward(f, "2")
    for env in (None, "3"):
        small, bufs = backward(f, env, ds_floats(1, T, h) - 1)
        assert all(same_bits(small, two).values()), env
        assert bool(torch.isnan(bufs.ws.data).all()), "the two-kernel form touched the dS workspace"
    # a whole-batch workspace under OCRL_ATTN_BWD=2 stays unused as well
    forced, bufs = backward(f, "2", ds_floats(B, T, h))
    assert all(same_bits(forced, two).values()) and bool(torch.isnan(bufs.ws.data).all())


def test_unset_and_3_select_the_same_form():
    B, T, h, dh = 2, 129, 2, 32
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    seed, site, _ = _drop_key(B, T, h)
    f = forward(q, k, v, dO, h, "padded", P_DROP, seed, site)
    a, ba = backward(f, None, ds_floats(B, T, h))
    b, bb = backward(f, "3", ds_floats(B, T, h))
    assert all(same_bits(a, b).values())
    # both wrote every element of the workspace (no NaN left) and the same values
    assert not bool(torch.isnan(ba.ws.data).any()) and torch.equal(E._bits(ba.ws.data), E._bits(bb.ws.data))


def test_every_element_above_the_diagonal_and_beyond_T_is_stored_as_zero():
    """the workspace after a call: no NaN left, and in the diagonal tiles [query][key] the entries with key > query, and all entries of
    rows and columns at and beyond T, are zero"""
    B, T, h, dh = 2, 129, 2, 48
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    f = forward(q, k, v, dO, h, "packed")
    _, bufs = backward(f, None, ds_floats(B, T, h))
    nblk = (T + 63) // 64
    ws = bufs.ws.data.view(B * h, nblk * (nblk + 1) // 2, 64, 64).cpu()
    assert not bool(torch.isnan(ws).any())
    i = torch.arange(64)
    for qt in range(nblk):
        for kt in range(qt + 1):
            tile = ws[:, qt * (qt + 1) // 2 + kt]
            dead = ((kt * 64 + i)[None, :] > (qt * 64 + i)[:, None]) | ((qt * 64 + i)[:, None] >= T) | ((kt * 64 + i)[None, :] >= T)
            assert bool((tile[:, dead] == 0).all()), (qt, kt)
            assert bool((tile[:, ~dead] != 0).any(-1).all()), (qt, kt)


def test_bitwise_reproducible_with_dropout():
    B, T, h, dh = 2, 132, 3, 48
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    seed, site, _ = _drop_key(B, T, h)
    f = forward(q, k, v, dO, h, "packed", P_DROP, seed, site)
    a, _ = backward(f, None, ds_floats(B, T, h))
    b, _ = backward(f, None, ds_floats(B, T, h))
    assert all(same_bits(a, b).values())
    c, _ = backward(f, None, ds_floats(1, T, h))
    assert all(same_bits(a, c).values())


def _model_step(env):
    """one training step (dropout on, device RNG) of a small SLATE model created under `env`: (all gradients, workspace bytes)"""
    from oracle import slate_oracle as O
    from ocrl_amd.engine import SlateEngine
    from tests.gpu_util import dims_from_cfg, load_params
    keys = ("OCRL_ATTN_BWD", "OCRL_ATTN_DS_MB")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        cfg = O.default_cfg(obs_size=64, vocab_size=256, num_slots=4, num_iterations=2, num_dec_blocks=2)          # T = 256: 4 tiles a side
        eng = SlateEngine(dims_from_cfg(cfg), max_batch=3, device="cuda:0")
        load_params(eng, O.formula_params(cfg))
        obs = torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(11)).cuda()
        eng.forward(obs, 1.0, train=True, seed=5)
        eng.backward()
        torch.cuda.synchronize()
        return eng.flat_g.clone().cpu(), eng.ws_bytes
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_model_step_is_the_same_with_whole_chunked_and_no_workspace():
    """SlateModel carves min(whole batch, OCRL_ATTN_DS_MB) for its decoder and hands it to every block's backward: the gradients of a
    step are bit for bit the same with the default (whole batch: 3 images of 4 heads x 10 tiles), with 1 MB (one image per chunk), with
    OCRL_ATTN_BWD=3 and with the two-kernel form, and the workspace the Python side allocates grows by what is carved"""
    whole = ds_floats(3, 256, 4) * 4
    g_default, ws_default = _model_step({})
    g_two, ws_two = _model_step({"OCRL_ATTN_BWD": "2"})
    g_mb, ws_mb = _model_step({"OCRL_ATTN_DS_MB": "1"})
    g_three, ws_three = _model_step({"OCRL_ATTN_BWD": "3"})
    g_zero, ws_zero = _model_step({"OCRL_ATTN_DS_MB": "0"})
    assert torch.isfinite(g_default).all() and g_default.abs().max() > 0
    for g in (g_two, g_mb, g_three, g_zero):
        assert torch.equal(E._bits(g_default), E._bits(g))
    assert ws_default - ws_two == whole and ws_three == ws_default and ws_mb - ws_two == 1 << 20 and ws_zero == ws_two


def test_outputs_are_overwritten_not_added_to():
    """a second call with other inputs into the same dq / dk / dv, delta and workspace (as the first call left them) matches its own
    reference, and bit for bit the same call into fresh buffers"""
    B, T, h, dh = 2, 129, 2, 48
    seed, site, keep = _drop_key(B, T, h)
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    f = forward(q, k, v, dO, h, "padded", P_DROP, seed, site)
    first, bufs = backward(f, None, ds_floats(B, T, h))
    grade("overwrite, first call", first, R.attention_ref(q, k, v, h, dO, keep, P_DROP))
    q2, k2, v2, dO2 = R.make_inputs(B, T, h, dh, seed=3)
    assert not torch.equal(q, q2)
    f = forward(q2, k2, v2, dO2, h, "padded", P_DROP, seed, site, into=f)
    second, _ = backward(f, None, ds_floats(B, T, h), bufs=bufs)
    grade("overwrite, second call", second, R.attention_ref(q2, k2, v2, h, dO2, keep, P_DROP))
    fresh, _ = backward(f, None, ds_floats(B, T, h))
    assert all(same_bits(second, fresh).values())
