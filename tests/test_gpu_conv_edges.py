"""The fp32 convolution kernels of csrc/conv.hip, each alone, against the float64 reference of tests/conv_ref.py at the project's unit
tolerance (2e-5 of the output's max): ragged images (W % 32 != 0, H % 4 != 0, images smaller than the halo), every epilogue mode
(bias, ReLU / ELU, position map, ReLU / ELU-derivative mask), the transposed (backward-data) pack, the low-latency variant, the
weight gradient below / at / above its worker cap with and without accumulation, and grids of 1 .. 510 workgroups for the XCD re-deal.

Every output sits between two guard bands and starts as NaN: a tile the re-deal drops leaves NaN behind, a store outside the tensor
breaks a band.  Inputs come from seeded generators; mask tensors are drawn independently of the data.

ELU (relu = 2, __expf in the epilogue) is graded at the same 2e-5 as everything else."""
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

GUARD = 4096                    # floats of guard band on each side of an output
SENT = 0x4B3C2D1E               # the bands' bit pattern (a finite float no kernel here produces by accident)
INST = [(5, 64), (5, 3), (3, 64)]                               # (ks, cin): conv_fwd_kernel / conv_wgrad_kernel <5,64>, <5,8>, <3,64>
SHAPES = [(2, 1, 1), (1, 3, 5), (1, 4, 32), (1, 7, 33), (1, 9, 65), (3, 20, 44), (3, 13, 100), (5, 30, 70), (2, 33, 31)]
# workgroups of the forward kernel at SHAPES, for the XCD re-deal (q = n >> 3, r = n & 7): q == 0 with r = 2, 1, 1, 4, then (q, r) = (1, 1),
# (3, 6), (6, 0), (15, 0), (2, 2); the weight-gradient grids (workers x ks) add 3, 5, 6, 10, 54, 72, 90, 120, 360 and the capped 510
GRIDS = [2, 1, 1, 4, 9, 30, 48, 120, 18]


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


def cpad_of(cin):
    return 8 if cin < 8 else 64


def tiles(B, H, W):
    return -(-W // 32) * -(-H // 4) * B


class Guarded:
    """a device tensor of `shape` with GUARD sentinel floats before and after it; the tensor starts as NaN (or as `init`)"""

    def __init__(self, shape, init=None):
        self.n = math.prod(shape)
        self.buf = torch.empty(2 * GUARD + self.n, device="cuda")
        self.buf.view(torch.int32).fill_(SENT)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)

    def check(self, tag):
        bits = self.buf.view(torch.int32).cpu()
        for name, band, base in (("before", bits[:GUARD], -GUARD), ("after", bits[GUARD + self.n:], self.n)):
            bad = (band != SENT).nonzero()
            assert bad.numel() == 0, f"{tag}: {bad.numel()} guard floats {name} the tensor overwritten, first at flat offset {base + int(bad[0])}"
        t = self.t.cpu()
        nf = (~torch.isfinite(t)).nonzero()
        assert nf.numel() == 0, f"{tag}: {nf.shape[0]} elements never written (or not finite), first at index {tuple(nf[0].tolist())}"


def grade(out_nhwc, ref_nchw, tag, tol=TOL):
    """relerr of an NHWC result against the NCHW float64 reference; on a miss the assertion names the first bad element and its tile"""
    o = out_nhwc.detach().cpu().double().permute(0, 3, 1, 2)
    e = relerr(o, ref_nchw)
    if not e < tol:
        d = (o - ref_nchw).abs() / max(ref_nchw.abs().max().item(), 1e-30)
        b, c, y, x = (d >= tol).nonzero()[0].tolist()
        pytest.fail(f"{tag}: relerr {e:.3e} >= {tol:.0e}; first bad element image {b} row {y} col {x} channel {c} (tile row {y // 4}, tile col {x // 32}, "
                    f"wave {y % 4}): got {o[b, c, y, x].item():.9g}, want {ref_nchw[b, c, y, x].item():.9g}; {int((d >= tol).sum())} bad of {d.numel()}")
    return e


def elu_mask(shape, g):
    """outputs of an ELU layer: positive, or negative inside (-1, 0), and a few elements exactly 0"""
    m = F.elu(torch.randn(*shape, generator=g))
    m.view(-1)[::53] = 0.0
    neg = m[m < 0]
    assert neg.numel() and neg.min() > -1 and int((m == 0).sum()) > 0
    return m


@functools.lru_cache(maxsize=None)
def fwd_case(ks, cin, B, H, W):
    """inputs of one forward case and its float64 convolution (no bias), shared by every epilogue and by the low-latency tests"""
    g = torch.Generator().manual_seed(1000 * ks + 100 * cin + 7 * B + 31 * H + W)
    c = dict(x=torch.randn(B, cin, H, W, generator=g), w=torch.randn(64, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5,
             b=torch.randn(64, generator=g), pm=torch.randn(64, H, W, generator=g), act=torch.randn(B, 64, H, W, generator=g))
    c["elu"] = elu_mask((B, 64, H, W), g)
    c["pre"] = F.conv2d(c["x"].double(), c["w"].double(), None, padding=ks // 2)
    return c


@functools.lru_cache(maxsize=None)
def bwd_case(ks, B, H, W):
    g = torch.Generator().manual_seed(5000 + 1000 * ks + 7 * B + 31 * H + W)
    c = dict(dy=torch.randn(B, 64, H, W, generator=g), w=torch.randn(64, 64, ks, ks, generator=g) / (64 * ks * ks) ** 0.5,
             act=torch.randn(B, 64, H, W, generator=g))
    c["elu"] = elu_mask((B, 64, H, W), g)
    c["pre"] = F.conv2d(c["dy"].double(), R.transposed_weight(c["w"]).double(), None, padding=ks // 2)
    return c


def conv_ex(L, tag, xd, wd, B, H, W, cin, ks, bias=None, relu=0, posmap=None, mask=None, mask_elu=0, transposed=0, low_latency=0):
    """ocrl_conv2d_ex into a guarded NaN tensor; returns the [B,H,W,64] result after checking the bands and that all of it was written"""
    cpad = cpad_of(cin)
    y = Guarded((B, H, W, 64))
    n = ks * ks * cpad * 64 * (2 if transposed else 1)
    ws = torch.full((n,), float("nan"), device="cuda")
    d = L.conv_desc(x=dp(xd), w=dp(wd), y=dp(y.t), B=B, H=H, W=W, cin=cin, cin_pad=cpad, ks=ks, bias=dp(bias), relu=relu, posmap=dp(posmap),
                    mask=dp(mask), mask_elu=mask_elu, transposed=transposed, low_latency=low_latency)
    L.check(L.lib().ocrl_conv2d_ex(d, P(ws), n, None))
    torch.cuda.synchronize()
    y.check(tag)
    return y.t


# (name, bias, relu, posmap, mask: None / "act" (ReLU mask) / "elu" (mask_elu = 1))
FWD_MODES = [("bias", 1, 0, 0, None), ("bias+relu", 1, 1, 0, None), ("bias+elu", 1, 2, 0, None), ("bias+relu+posmap", 1, 1, 1, None),
             ("elu+posmap+relu-mask", 0, 2, 1, "act"), ("bias+posmap+elu-mask", 1, 0, 1, "elu")]


@pytest.mark.parametrize("B,H,W", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("ks,cin", INST)
def test_forward_every_epilogue_on_ragged_images(L, ks, cin, B, H, W):
    assert tiles(B, H, W) == GRIDS[SHAPES.index((B, H, W))]
    c = fwd_case(ks, cin, B, H, W)
    xd, wd, bd = dev(nhwc(c["x"], cpad_of(cin))), dev(c["w"]), dev(c["b"])
    pmd = dev(c["pm"].permute(1, 2, 0))
    md = {"act": dev(nhwc(c["act"])), "elu": dev(nhwc(c["elu"]))}
    errs = []
    for name, bias, relu, posmap, mask in FWD_MODES:
        tag = f"conv fwd {ks}x{ks} cin{cin} B{B} {H}x{W} [{name}]"
        pre = c["pre"] + c["b"].double().view(1, -1, 1, 1) if bias else c["pre"]
        ref = R.epilogue(pre, relu, c["pm"] if posmap else None, c[mask] if mask else None, mask == "elu")
        y = conv_ex(L, tag, xd, wd, B, H, W, cin, ks, bias=bd if bias else None, relu=relu, posmap=pmd if posmap else None,
                    mask=md[mask] if mask else None, mask_elu=int(mask == "elu"))
        errs.append(f"{name} {grade(y, ref, tag):.2e}")
    log(f"conv edges fwd {ks}x{ks} cin{cin} B{B} {H}x{W} ({tiles(B, H, W)} workgroups): " + ", ".join(errs))


@pytest.mark.parametrize("B,H,W", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("ks", [5, 3])
def test_backward_data_transposed_pack_and_masks(L, ks, B, H, W):
    c = bwd_case(ks, B, H, W)
    dyd, wd = dev(nhwc(c["dy"])), dev(c["w"])
    errs = []
    for name, mask in (("no mask", None), ("relu mask", "act"), ("elu mask", "elu")):
        tag = f"conv bwd-data {ks}x{ks} B{B} {H}x{W} [{name}]"
        ref = R.epilogue(c["pre"], 0, None, c[mask] if mask else None, mask == "elu")
        dx = conv_ex(L, tag, dyd, wd, B, H, W, 64, ks, mask=dev(nhwc(c[mask])) if mask else None, mask_elu=int(mask == "elu"), transposed=1)
        errs.append(f"{name} {grade(dx, ref, tag):.2e}")
    log(f"conv edges bwd-data {ks}x{ks} B{B} {H}x{W} ({tiles(B, H, W)} workgroups): " + ", ".join(errs))


@pytest.mark.parametrize("B,H,W", [s for s in SHAPES if tiles(*s) <= 160], ids=lambda v: str(v))
def test_low_latency_kernel_on_ragged_images(L, B, H, W):
    """conv_lat_kernel (its own copy of bias / ReLU / posmap) against float64 and against the throughput kernel; and the contract of
    conv_lat_applies: with ELU or a mask the request must run the throughput kernel, bit for bit"""
    c = fwd_case(5, 64, B, H, W)
    xd, wd, bd, pmd, actd = dev(nhwc(c["x"])), dev(c["w"]), dev(c["b"]), dev(c["pm"].permute(1, 2, 0)), dev(nhwc(c["act"]))
    pre = c["pre"] + c["b"].double().view(1, -1, 1, 1)
    errs = []
    for posmap in (0, 1):
        for relu in (0, 1):
            tag = f"conv low-latency B{B} {H}x{W} relu{relu} posmap{posmap}"
            kw = dict(bias=bd, relu=relu, posmap=pmd if posmap else None)
            y1 = conv_ex(L, tag, xd, wd, B, H, W, 64, 5, low_latency=1, **kw)
            y0 = conv_ex(L, tag + " (throughput)", xd, wd, B, H, W, 64, 5, low_latency=0, **kw)
            e = grade(y1, R.epilogue(pre, relu, c["pm"] if posmap else None), tag)
            e0 = relerr(y1.cpu(), y0.cpu())
            errs.append(f"relu{relu} posmap{posmap} {e:.2e} (vs throughput {e0:.2e})")
            assert e0 < TOL, tag
    for name, kw in (("elu", dict(bias=bd, relu=2, posmap=pmd)), ("mask", dict(bias=bd, relu=1, mask=actd)),
                     ("elu mask", dict(bias=bd, relu=0, posmap=pmd, mask=dev(nhwc(c["elu"])), mask_elu=1))):
        tag = f"conv low-latency refused mode B{B} {H}x{W} [{name}]"
        y1 = conv_ex(L, tag, xd, wd, B, H, W, 64, 5, low_latency=1, **kw)
        y0 = conv_ex(L, tag, xd, wd, B, H, W, 64, 5, low_latency=0, **kw)
        assert torch.equal(y1, y0), f"{tag}: low_latency = 1 did not give the throughput kernel's result"
    log(f"conv edges low-latency B{B} {H}x{W}: " + ", ".join(errs) + "; elu / mask requests bit-identical to the throughput kernel")


def wgrad_ex(L, tag, xd, dyd, B, H, W, cin, ks, accumulate=0, init_w=None, init_b=None):
    cpad = cpad_of(cin)
    n = L.lib().ocrl_conv2d_wgrad_ws_floats(B, H, W, ks, cpad)
    ws = torch.full((n,), float("nan"), device="cuda")         # a slab no workgroup writes shows as NaN in dw
    dw, db = Guarded((64, cin, ks, ks), init_w), Guarded((64,), init_b)
    d = L.conv_wgrad_desc(x=dp(xd), dy=dp(dyd), dw=dp(dw.t), db=dp(db.t), B=B, H=H, W=W, cin=cin, cin_pad=cpad, ks=ks, accumulate=accumulate)
    L.check(L.lib().ocrl_conv2d_bwd_weight_ex(d, P(ws), n, None))
    torch.cuda.synchronize()
    dw.check(tag + " dw")
    db.check(tag + " db")
    return dw.t.cpu(), db.t.cpu()


def workers(L, B, H, W, ks, cin):
    """chunk workers of the weight-gradient grid, from the workspace the library asks for (slabs of ks*ks*64*cin_pad floats, two per
    worker for the 8-channel kernel, plus 65536 floats for the bias column sum)"""
    cpad = cpad_of(cin)
    n = L.lib().ocrl_conv2d_wgrad_ws_floats(B, H, W, ks, cpad) - (1 << 16)
    slab = (1 if cpad == 64 else 2) * ks * ks * 64 * cpad
    assert n % slab == 0
    return n // slab


WGRAD_CASES = [(ks, cin, B, H, W) for ks, cin in INST
               for B, H, W in [(b, 30, 70) for b in ((1, 5, 10) if ks == 5 else (1, 5, 8, 10, 15))] + [(2, 1, 1), (1, 3, 5), (2, 33, 31)]]
# tiles per worker at B x 30 x 70 (24 tiles per image): the single trip, and the uneven second and third trips of the main loop
TRIPS = {(5, 1): (1, 1), (5, 5): (1, 2), (5, 10): (2, 3), (3, 1): (1, 1), (3, 5): (1, 1), (3, 8): (1, 2), (3, 10): (1, 2), (3, 15): (2, 3)}


@pytest.mark.parametrize("ks,cin,B,H,W", WGRAD_CASES, ids=lambda v: str(v))
def test_weight_gradient_around_the_worker_cap_and_accumulate(L, ks, cin, B, H, W):
    nt, nw = tiles(B, H, W), workers(L, B, H, W, ks, cin)
    assert nw == min(512 // ks, nt)
    if (H, W) == (30, 70):
        assert (nt // nw, -(-nt // nw)) == TRIPS[(ks, B)]
    g = torch.Generator().manual_seed(9000 + 1000 * ks + 100 * cin + 7 * B + 31 * H + W)
    x, dy = torch.randn(B, cin, H, W, generator=g), torch.randn(B, 64, H, W, generator=g)
    s = (B * H * W) ** 0.5                                      # the gradients' own scale: sums of B*H*W unit-variance products
    pw, pb = torch.randn(64, cin, ks, ks, generator=g) * s, torch.randn(64, generator=g) * s
    _, rw, rb = R.conv_grads(x, torch.zeros(64, cin, ks, ks), dy, need_dx=False)
    xd, dyd = dev(nhwc(x, cpad_of(cin))), dev(nhwc(dy))
    tag = f"conv wgrad {ks}x{ks} cin{cin} B{B} {H}x{W}"
    dw, db = wgrad_ex(L, tag, xd, dyd, B, H, W, cin, ks)
    dw2, db2 = wgrad_ex(L, tag + " (second call)", xd, dyd, B, H, W, cin, ks)
    aw, ab = wgrad_ex(L, tag + " (accumulate)", xd, dyd, B, H, W, cin, ks, accumulate=1, init_w=pw, init_b=pb)
    e, eb = relerr(dw, rw), relerr(db, rb)
    ea, eab = relerr(aw, pw.double() + rw), relerr(ab, pb.double() + rb)
    log(f"conv edges wgrad {ks}x{ks} cin{cin} B{B} {H}x{W} ({nt} tiles on {nw} workers, {nw * ks} workgroups): dW {e:.2e} db {eb:.2e}, "
        f"accumulated dW {ea:.2e} db {eab:.2e}")
    if not e < TOL:
        d = (dw.double() - rw).abs() / rw.abs().max().item()
        co, ci, ky, kx = (d >= TOL).nonzero()[0].tolist()
        pytest.fail(f"{tag}: dW relerr {e:.3e}; first bad element co {co} ci {ci} ky {ky} kx {kx}: got {dw[co, ci, ky, kx].item():.9g}, "
                    f"want {rw[co, ci, ky, kx].item():.9g}; {int((d >= TOL).sum())} bad of {d.numel()}")
    assert eb < TOL and ea < TOL and eab < TOL
    assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{tag}: two identical calls differ (the reduce is ordered, there are no atomics)"


@pytest.mark.parametrize("ks,cin", INST)
def test_images_are_independent_forward(L, ks, cin):
    """a batch equals its images run one at a time, bit for bit: a tile's arithmetic does not depend on the grid it is dealt from"""
    B, H, W = 3, 20, 44
    c = fwd_case(ks, cin, B, H, W)
    cpad = cpad_of(cin)
    xd, wd, bd, pmd = dev(nhwc(c["x"], cpad)), dev(c["w"]), dev(c["b"]), dev(c["pm"].permute(1, 2, 0))
    for lat in ((0, 1) if (ks, cin) == (5, 64) else (0,)):
        tag = f"conv fwd {ks}x{ks} cin{cin} batch vs images low_latency{lat}"
        kw = dict(bias=bd, relu=1, posmap=pmd, low_latency=lat)
        y = conv_ex(L, tag, xd, wd, B, H, W, cin, ks, **kw)
        for b in range(B):
            yb = conv_ex(L, tag, xd[b:b + 1], wd, 1, H, W, cin, ks, **kw)
            assert torch.equal(yb[0], y[b]), f"{tag}: image {b} differs"
        log(f"conv edges {tag}: bit-identical")


@pytest.mark.parametrize("ks,cin", INST)
def test_images_are_independent_weight_gradient(L, ks, cin):
    """the batch's weight gradient is the sum of its images' (5 x 24 tiles: the batch runs the two-trip main loop where 5x5, the images
    the single trip)"""
    B, H, W = 5, 30, 70
    g = torch.Generator().manual_seed(77 + ks + cin)
    x, dy = torch.randn(B, cin, H, W, generator=g), torch.randn(B, 64, H, W, generator=g)
    xd, dyd = dev(nhwc(x, cpad_of(cin))), dev(nhwc(dy))
    tag = f"conv wgrad {ks}x{ks} cin{cin} batch vs images"
    dw, db = wgrad_ex(L, tag, xd, dyd, B, H, W, cin, ks)
    sw, sb = torch.zeros_like(dw, dtype=torch.double), torch.zeros_like(db, dtype=torch.double)
    for b in range(B):
        w1, b1 = wgrad_ex(L, tag, xd[b:b + 1], dyd[b:b + 1], 1, H, W, cin, ks)
        sw += w1.double()
        sb += b1.double()
    e, eb = relerr(dw, sw), relerr(db, sb)
    log(f"conv edges {tag}: dW {e:.2e} db {eb:.2e}")
    assert e < TOL and eb < TOL
