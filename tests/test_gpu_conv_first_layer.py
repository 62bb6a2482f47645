"""The first encoder layer's own kernels (csrc/conv_first.hip: 5x5, 3 -> 64 channels on the NCHW observation) and the bias gradient that
conv_wgrad_kernel now sums itself, each alone against the float64 reference of tests/conv_ref.py at the project's unit tolerance (2e-5 of
the output's max), with the conventions of tests/test_gpu_conv_edges.py: ragged images, outputs between guard bands and pre-filled with
NaN, seeded inputs.

Tolerance: every sum here is an fp32 accumulation of n products in a fixed order (n <= 75 forward; the pixels of the batch backward, at
most 70 000 here, split over workers and slabs); its error grows like sqrt(n) * 2^-24 of the sum's own scale, 2e-5 leaves a factor of ten
at the largest case.  The column-sum db and the <5, 8> kernels these replace pass at the same 2e-5 on these shapes."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R
from tests.gpu_util import log, relerr
from tests.test_gpu_kernels import TOL, nhwc

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT = 0x4B3C2D1E
RAGGED = [(2, 1, 1), (1, 3, 5), (1, 4, 32), (1, 7, 33), (1, 9, 65), (3, 13, 100), (2, 33, 31)]
CAP = 512                                                       # workers of conv_first_wgrad_kernel
AROUND_CAP = [(4, 16, 992), (4, 16, 1024), (4, 17, 1000)]       # 496, 512 and 640 tiles: below, at, above (uneven second trip)


@pytest.fixture(scope="module")
def L():
    from ocrl_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dp(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.to("cuda").contiguous()


def tiles(B, H, W):
    return -(-W // 32) * -(-H // 4) * B


class Guarded:
    """a device tensor of `shape` between two bands of GUARD sentinel floats; it starts as NaN, as `init`, or (fill_sent) as sentinels"""

    def __init__(self, shape, init=None, fill_sent=False):
        self.n = math.prod(shape)
        self.buf = torch.empty(2 * GUARD + self.n, device="cuda")
        self.buf.view(torch.int32).fill_(SENT)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)
        elif not fill_sent:
            self.t.fill_(float("nan"))

    def check_bands(self, tag):
        bits = self.buf.view(torch.int32).cpu()
        for name, band, base in (("before", bits[:GUARD], -GUARD), ("after", bits[GUARD + self.n:], self.n)):
            bad = (band != SENT).nonzero()
            assert bad.numel() == 0, f"{tag}: {bad.numel()} guard floats {name} the tensor overwritten, first at flat offset {base + int(bad[0])}"

    def check(self, tag):
        self.check_bands(tag)
        nf = (~torch.isfinite(self.t.cpu())).nonzero()
        assert nf.numel() == 0, f"{tag}: {nf.shape[0]} elements never written (or not finite), first at index {tuple(nf[0].tolist())}"


def assert_close(got, want, tag):
    e = relerr(got, want)
    print(f"{tag}: relerr {e:.3e}")
    if not e < TOL:
        d = (got.double().cpu() - want).abs() / max(want.abs().max().item(), 1e-30)
        pytest.fail(f"{tag}: relerr {e:.3e} >= {TOL:.0e}; first bad element {tuple((d >= TOL).nonzero()[0].tolist())}, {int((d >= TOL).sum())} bad of {d.numel()}")
    return e


# ----------------------------------------------------------------------------------------------------------- B: first layer, forward
@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W):
    g = torch.Generator().manual_seed(31000 + 7 * B + 31 * H + W)
    c = dict(x=torch.randn(B, 3, H, W, generator=g), w=torch.randn(64, 3, 5, 5, generator=g) / 75 ** 0.5, b=torch.randn(64, generator=g))
    c["pre"] = F.conv2d(c["x"].double(), c["w"].double(), None, padding=2)
    return c


def first_fwd(L, tag, xd, wd, bd, B, H, W, relu):
    y = Guarded((B, H, W, 64))
    n = L.lib().ocrl_conv2d_first_fwd_ws_floats()
    ws = Guarded((n,))
    L.check(L.lib().ocrl_conv2d_first_fwd(P(xd), P(wd), P(bd), P(y.t), B, H, W, relu, P(ws.t), n, None))
    torch.cuda.synchronize()
    y.check(tag)
    ws.check_bands(tag + " workspace")
    return y.t


@pytest.mark.parametrize("B,H,W", RAGGED, ids=lambda v: str(v))
def test_first_layer_forward_on_ragged_images(L, B, H, W):
    c = fwd_case(B, H, W)
    xd, wd, bd = dev(c["x"]), dev(c["w"]), dev(c["b"])
    errs = []
    for bias in (0, 1):
        for relu in (0, 1):
            tag = f"conv first fwd B{B} {H}x{W} bias{bias} relu{relu}"
            ref = R.epilogue(c["pre"] + c["b"].double().view(1, -1, 1, 1) if bias else c["pre"], relu)
            y = first_fwd(L, tag, xd, wd, bd if bias else None, B, H, W, relu)
            errs.append(assert_close(y.permute(0, 3, 1, 2), ref, tag))
    log(f"conv first fwd B{B} {H}x{W} ({tiles(B, H, W)} tiles): " + ", ".join(f"{e:.2e}" for e in errs))


def test_first_layer_forward_does_not_depend_on_the_batch(L):
    B, H, W = 3, 13, 100
    c = fwd_case(B, H, W)
    xd, wd, bd = dev(c["x"]), dev(c["w"]), dev(c["b"])
    y = first_fwd(L, "conv first fwd batch", xd, wd, bd, B, H, W, 1)
    y1 = first_fwd(L, "conv first fwd image 1 alone", xd[1:2].contiguous(), wd, bd, 1, H, W, 1)
    assert torch.equal(y1[0], y[1]), "image 1 of the B = 3 call differs from the same image at B = 1"
    log("conv first fwd: image 1 of B = 3 bit-identical to B = 1")


# ------------------------------------------------------------------------------------------------- C: first layer, weight gradient
@functools.lru_cache(maxsize=None)
def wgrad_case(cin, ks, B, H, W):
    g = torch.Generator().manual_seed(47000 + 1000 * ks + 100 * cin + 7 * B + 31 * H + W)
    x, dy = torch.randn(B, cin, H, W, generator=g), torch.randn(B, 64, H, W, generator=g)
    s = (B * H * W) ** 0.5                                      # the gradients' own scale
    pw, pb = torch.randn(64, cin, ks, ks, generator=g) * s, torch.randn(64, generator=g) * s
    _, rw, rb = R.conv_grads(x, torch.zeros(64, cin, ks, ks), dy, need_dx=False)
    return dict(x=x, dy=dy, pw=pw, pb=pb, rw=rw, rb=rb)


def first_wgrad(L, tag, xd, dyd, B, H, W, accumulate=0, init_w=None, init_b=None):
    n = L.lib().ocrl_conv2d_first_wgrad_ws_floats(B, H, W)
    ws = Guarded((n,))                                          # a slab no worker writes shows as NaN in dw
    dw, db = Guarded((64, 3, 5, 5), init_w), Guarded((64,), init_b)
    L.check(L.lib().ocrl_conv2d_first_bwd_weight(P(xd), P(dyd), P(dw.t), P(db.t), B, H, W, accumulate, P(ws.t), n, None))
    torch.cuda.synchronize()
    dw.check(tag + " dw")
    db.check(tag + " db")
    ws.check_bands(tag + " workspace")
    return dw.t.cpu(), db.t.cpu()


@pytest.mark.parametrize("B,H,W", RAGGED + AROUND_CAP, ids=lambda v: str(v))
def test_first_layer_weight_gradient(L, B, H, W):
    nt = tiles(B, H, W)
    n = L.lib().ocrl_conv2d_first_wgrad_ws_floats(B, H, W)
    nw = min(CAP, nt)
    assert n % nw == 0 and n // nw >= 64 * 75 + 64
    if (B, H, W) in AROUND_CAP:
        assert (nt < CAP, nt == CAP, nt > CAP) == tuple(i == AROUND_CAP.index((B, H, W)) for i in range(3))
    c = wgrad_case(3, 5, B, H, W)
    xd, dyd = dev(c["x"]), dev(nhwc(c["dy"]))
    tag = f"conv first wgrad B{B} {H}x{W}"
    dw, db = first_wgrad(L, tag, xd, dyd, B, H, W)
    dw2, db2 = first_wgrad(L, tag + " (second call)", xd, dyd, B, H, W)
    aw, ab = first_wgrad(L, tag + " (accumulate)", xd, dyd, B, H, W, accumulate=1, init_w=c["pw"], init_b=c["pb"])
    e = assert_close(dw, c["rw"], tag + " dW")
    eb = assert_close(db, c["rb"], tag + " db")
    ea = assert_close(aw, c["pw"].double() + c["rw"], tag + " accumulated dW")
    eab = assert_close(ab, c["pb"].double() + c["rb"], tag + " accumulated db")
    assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{tag}: two identical calls differ (the sums are ordered, there are no atomics)"
    log(f"conv first wgrad B{B} {H}x{W} ({nt} tiles on {nw} workers): dW {e:.2e} db {eb:.2e}, accumulated dW {ea:.2e} db {eab:.2e}")


def test_first_layer_weight_gradient_without_db(L):
    B, H, W = 3, 13, 100
    c = wgrad_case(3, 5, B, H, W)
    n = L.lib().ocrl_conv2d_first_wgrad_ws_floats(B, H, W)
    ws, dw = Guarded((n,)), Guarded((64, 3, 5, 5))
    xd, dyd = dev(c["x"]), dev(nhwc(c["dy"]))
    L.check(L.lib().ocrl_conv2d_first_bwd_weight(P(xd), P(dyd), P(dw.t), None, B, H, W, 0, P(ws.t), n, None))
    torch.cuda.synchronize()
    dw.check("conv first wgrad, no db")
    ws.check_bands("conv first wgrad, no db: workspace")
    assert_close(dw.t.cpu(), c["rw"], "conv first wgrad, no db: dW")


# ------------------------------------------------------------------------------- A: bias gradient inside conv_wgrad_kernel
INST = [(5, 64), (5, 3), (3, 64)]
A_SHAPES = RAGGED + [(3, 20, 44), (5, 30, 70)]                  # the last: 120 tiles, above the 102-worker cap of the 5x5 kernels


def cpad_of(cin):
    return 8 if cin < 8 else 64


def slabs_of(ks, cin, B, H, W):
    return min(512 // ks, tiles(B, H, W)) * (1 if cpad_of(cin) == 64 else 2)


def wgrad_ex(L, tag, xd, dyd, B, H, W, cin, ks, accumulate=0, init_w=None, init_b=None, with_db=True):
    cpad = cpad_of(cin)
    n = L.lib().ocrl_conv2d_wgrad_ws_floats(B, H, W, ks, cpad)
    ws = Guarded((n,), fill_sent=True)                          # exactly the queried size, sentinels all through
    dw = Guarded((64, cin, ks, ks), init_w)
    db = Guarded((64,), init_b) if with_db else None
    d = L.conv_wgrad_desc(x=dp(xd), dy=dp(dyd), dw=dp(dw.t), db=dp(db.t) if with_db else None, B=B, H=H, W=W, cin=cin, cin_pad=cpad, ks=ks,
                          accumulate=accumulate)
    L.check(L.lib().ocrl_conv2d_bwd_weight_ex(d, P(ws.t), n, None))
    torch.cuda.synchronize()
    dw.check(tag + " dw")
    ws.check_bands(tag + " workspace")
    if with_db:
        db.check(tag + " db")
    return dw.t.cpu(), (db.t.cpu() if with_db else None), ws.t.view(torch.int32).cpu()


@pytest.mark.parametrize("B,H,W", A_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("ks,cin", INST)
def test_fused_bias_gradient(L, ks, cin, B, H, W):
    c = wgrad_case(cin, ks, B, H, W)
    xd, dyd = dev(nhwc(c["x"], cpad_of(cin))), dev(nhwc(c["dy"]))
    tag = f"conv wgrad fused db {ks}x{ks} cin{cin} B{B} {H}x{W}"
    dw, db, _ = wgrad_ex(L, tag, xd, dyd, B, H, W, cin, ks)
    dw2, db2, _ = wgrad_ex(L, tag + " (second call)", xd, dyd, B, H, W, cin, ks)
    aw, ab, _ = wgrad_ex(L, tag + " (accumulate)", xd, dyd, B, H, W, cin, ks, accumulate=1, init_w=c["pw"], init_b=c["pb"])
    eb = assert_close(db, c["rb"], tag + " db")
    eab = assert_close(ab, c["pb"].double() + c["rb"], tag + " accumulated db")
    e = assert_close(dw, c["rw"], tag + " dW")
    ea = assert_close(aw, c["pw"].double() + c["rw"], tag + " accumulated dW")
    assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{tag}: two identical calls differ"
    log(f"{tag} ({slabs_of(ks, cin, B, H, W)} slabs): db {eb:.2e} dW {e:.2e}, accumulated db {eab:.2e} dW {ea:.2e}")


@pytest.mark.parametrize("ks,cin", INST)
def test_without_db_nothing_is_written_past_the_dw_slabs(L, ks, cin):
    B, H, W = 5, 30, 70
    c = wgrad_case(cin, ks, B, H, W)
    tag = f"conv wgrad no db {ks}x{ks} cin{cin}"
    xd, dyd = dev(nhwc(c["x"], cpad_of(cin))), dev(nhwc(c["dy"]))
    dw, _, ws = wgrad_ex(L, tag, xd, dyd, B, H, W, cin, ks, with_db=False)
    used = slabs_of(ks, cin, B, H, W) * ks * ks * 64 * cpad_of(cin)
    assert used < ws.numel()
    bad = (ws[used:] != SENT).nonzero()
    assert bad.numel() == 0, f"{tag}: {bad.numel()} floats written past the dW slabs, first at workspace offset {used + int(bad[0])}"
    assert_close(dw, c["rw"], tag + " dW")
