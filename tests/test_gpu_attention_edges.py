"""Kernel-level tests of the causal self-attention (csrc/attention.hip) through ocrl_attention_fwd / ocrl_attention_bwd against the fp64
reference of tests/attention_ref.py: dropout on, lengths around every tile seam, three stride layouts, overwrite semantics, a wide
soft-max range and bitwise reproducibility.  Every backward runs in both forms (OCRL_ATTN_BWD=1: one pass; 2: dK/dV kernel + dQ kernel).

Every call here goes through `run`, which is hostile on purpose: outputs are pre-filled with NaN (the contract is "writes", not "adds
to"), every output sits between sentinel guard words that must come back bit-unchanged, pad columns of q/k/v hold NaN and those of
dq/dk/dv a sentinel, and q/k/v/dO are followed by NaN rows, so a read past B*T rows that reaches a result shows up as NaN."""
import ctypes
import os

import pytest
import torch

from tests import attention_ref as R
from tests.gpu_util import log, relerr

pytestmark = pytest.mark.gpu
P = lambda t: ctypes.c_void_p(t.data_ptr())
TOL = 2e-5
FORMS = (("one-pass", "1"), ("two-kernel", "2"))
GUARD = 64                # guard words (floats) before and after every output; a multiple of 4 keeps the 16-byte alignment
HEAD, TAIL = 8, 72        # rows before the first and after the last image of every row-strided tensor (TAIL: more than one 64-row tile)
SENTINEL = -7.0625e10     # exactly representable; guards and pad columns are compared as bit patterns
_ids = lambda c: "B{}-T{}-h{}-dh{}".format(*c[:4]) + ("-p{}-seed{}-site{}".format(*c[4:]) if len(c) > 4 else "")


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """n floats of NaN between GUARD sentinel words before and GUARD + extra after"""

    def __init__(self, n, extra=0):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD + extra,), SENTINEL, device="cuda")
        self.data = self.buf[GUARD:GUARD + n]
        self.data.fill_(float("nan"))

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return bool((_bits(g) == _bits(torch.full_like(g, SENTINEL))).all())


def _place(layout, B, T, d, tensors, fill):
    """the three [B,T,d] tensors in the row-strided layout: returns (views [B*T, d] with row stride ld, ld, the whole allocations);
    everything outside the views' B*T x d elements (pad columns, HEAD rows before, TAIL rows after) is `fill`"""
    rows, r0 = HEAD + B * T + TAIL, HEAD
    if layout == "dense":
        ld, allocs = d, [torch.full((rows, d), fill, device="cuda") for _ in range(3)]
        views = [a[r0:r0 + B * T] for a in allocs]
    else:
        ld = 3 * d + (8 if layout == "padded" else 0)
        a = torch.full((rows, ld), fill, device="cuda")
        allocs, views = [a], [a[r0:r0 + B * T, i * d:(i + 1) * d] for i in range(3)]
    for vw, t in zip(views, tensors):
        if torch.is_tensor(t):
            vw.copy_(t.reshape(B * T, d))
        else:
            vw.fill_(t)
    return views, ld, allocs


def _outside_unchanged(views, allocs, d, before):
    """every element of the allocations outside the views is bit-identical to `before` (clones taken before the call)"""
    for a, b0 in zip(allocs, before):
        inside = torch.zeros_like(a, dtype=torch.bool)
        for vw in views:
            if vw.untyped_storage().data_ptr() == a.untyped_storage().data_ptr():
                off = vw.storage_offset() - a.storage_offset()
                r0, c0 = off // a.stride(0), off % a.stride(0)
                inside[r0:r0 + vw.shape[0], c0:c0 + d] = True
        if not bool((_bits(a)[~inside] == _bits(b0)[~inside]).all()):
            return False
    return True


def run(L, q, k, v, dO, h, layout="packed", p=0.0, seed=0, site=0, forms=FORMS, backward=True):
    """forward once, backward once per form; returns {"o", "lse", form: {"dq","dk","dv","delta"}} as CPU tensors.  Asserts the
    memory-safety side of the contract (guards, pads, no NaN in any result) on the way."""
    from ocrl_amd import _lib
    B, T, d = q.shape
    nan = float("nan")
    (qv, kv, vv), ld, _ = _place(layout, B, T, d, (q, k, v), nan)
    # dO and o have row stride d.  Both allocations reach as far as row stride ld would: a kernel that swaps the two strides then reads
    # NaN or writes into the guard -- inside this test's own memory, where it is seen -- and not past the end of an allocation
    gall = torch.full((HEAD + B * T + TAIL + (B * T * (ld - d) + d - 1) // d, d), nan, device="cuda")
    gbuf = gall[HEAD:HEAD + B * T]
    gbuf.copy_(dO.reshape(B * T, d))
    o, lse = Guarded(B * T * d, extra=B * T * (ld - d)), Guarded(B * h * T)
    _lib.check(L.ocrl_attention_fwd(P(qv), P(kv), P(vv), P(o.data), P(lse.data), B, T, d, h, ld, p, seed, site, None))
    torch.cuda.synchronize()
    assert o.guards_intact() and lse.guards_intact(), "forward wrote outside o / lse"
    out = dict(o=o.data.view(B, T, d).cpu(), lse=lse.data.view(B, h, T).cpu())
    assert torch.isfinite(out["o"]).all() and torch.isfinite(out["lse"]).all(), "forward left or produced a non-finite value"
    if not backward:
        return out
    old = os.environ.get("OCRL_ATTN_BWD")
    try:
        for name, flag in forms:
            os.environ["OCRL_ATTN_BWD"] = flag
            gviews, _, gallocs = _place(layout, B, T, d, (nan, nan, nan), SENTINEL)
            before = [a.clone() for a in gallocs]
            delta = Guarded(B * h * T)
            _lib.check(L.ocrl_attention_bwd(P(qv), P(kv), P(vv), P(o.data), P(lse.data), P(gbuf), P(gviews[0]), P(gviews[1]), P(gviews[2]),
                                            P(delta.data), B, T, d, h, ld, p, seed, site, None))
            torch.cuda.synchronize()
            assert delta.guards_intact(), f"{name}: wrote outside delta"
            assert _outside_unchanged(gviews, gallocs, d, before), f"{name}: wrote outside dq / dk / dv (pad column, tail row)"
            res = {n: t.reshape(B, T, d).cpu() for n, t in zip(("dq", "dk", "dv"), gviews)}
            res["delta"] = delta.data.view(B, h, T).cpu()
            for n, t in res.items():
                assert torch.isfinite(t).all(), f"{name}: {n} holds a non-finite value (not overwritten, or read from a pad / tail row)"
            out[name] = res
    finally:
        if old is None:
            os.environ.pop("OCRL_ATTN_BWD", None)
        else:
            os.environ["OCRL_ATTN_BWD"] = old
    assert o.guards_intact() and lse.guards_intact()
    assert torch.equal(_bits(out["o"]), _bits(o.data.view(B, T, d).cpu())), "the backward changed o"
    return out


def grad_floor(ref):
    """Each gradient is graded on its own max-norm, floored at a tenth of the largest of the three.  The floor matters where a gradient
    is exactly zero or nearly so -- at T = 1, P = 1 and dq = dk = 0: both sides then hold the rounding residue of dP - delta -- and
    never exceeds the norm of the joint dq|dk|dv tensor that tests/test_gpu_attention.py grades on."""
    return 0.1 * max(ref[n].abs().max().item() for n in ("dq", "dk", "dv"))


def errors(out, ref):
    """{quantity: relerr} of a run against the reference, backward forms included (delta is scratch: checked for guards and NaN only)"""
    e = dict(o=relerr(out["o"], ref["o"]), lse=relerr(out["lse"], ref["lse"]))
    for name, _ in FORMS:
        if name in out:
            for n in ("dq", "dk", "dv"):
                e[f"{name}.{n}"] = relerr(out[name][n], ref[n], floor=grad_floor(ref))
    return e


def check(tag, out, ref, tol=TOL):
    e = errors(out, ref)
    log(f"[attention edges] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()) + f" worst={max(e.values()):.2e}")
    bad = {k: v for k, v in e.items() if not v < tol}
    assert not bad, (tag, bad)
    return e


def _lib_handle():
    from ocrl_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("case", R.LENGTH_CASES, ids=_ids)
def test_lengths_without_dropout(case):
    """every length around the 64-query / 128-key tile seams, T % 4 != 0 included, each head width at T = 1, 65, 129"""
    B, T, h, dh = case
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    layout = R.LAYOUTS[R.LENGTH_CASES.index(case) % 3]
    out = run(_lib_handle(), q, k, v, dO, h, layout)
    check(f"p=0 {_ids(case)} {layout}", out, R.attention_ref(q, k, v, h, dO))


def _dropout_case(case, layout, group):
    B, T, h, dh, p, seed, site = case
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    keep = R.keep_mask(seed, site, p, B, h, T)
    both, share, z = R.non_vacuity(keep, p)
    assert both and z < 5.0, (both, share, z)
    out = run(_lib_handle(), q, k, v, dO, h, layout, p, seed, site)
    ref = R.attention_ref(q, k, v, h, dO, keep, p)
    plain = R.attention_ref(q, k, v, h)["o"]
    assert relerr(plain, ref["o"]) > 1e-2                      # the mask moves the result far beyond the tolerance
    return check(f"{group} {_ids(case)} {layout} dropped {share:.4f} ({z:.1f} sigma)", out, ref)


@pytest.mark.parametrize("case", R.DROPOUT_CASES, ids=_ids)
def test_dropout_matches_host_mask(case):
    """keep decisions of all four kernels against the host restatement of the counter RNG, through the fp64 reference"""
    _dropout_case(case, R.LAYOUTS[R.DROPOUT_CASES.index(case) % 3], "dropout")


@pytest.mark.parametrize("case", R.ODD_DROPOUT_CASES, ids=_ids)
def test_dropout_at_lengths_off_the_group_size(case):
    """T % 4 != 0: mask rows are indexed with the key stride T4 (csrc/common.h attn_drop_ld), so the forward / dQ kernels (group of four
    keys from the row start) and the dK/dV kernels (group of the key) take the same decisions as the mask dump"""
    _dropout_case(case, R.LAYOUTS[R.ODD_DROPOUT_CASES.index(case) % 3], "dropout T%4")


@pytest.mark.parametrize("case", [c for c in R.DROPOUT_CASES + R.ODD_DROPOUT_CASES if c[6] == R.SITE_POOL and c[1] in (9, 64)], ids=_ids)
def test_device_mask_dump_equals_host_mask(case):
    """the device's dump of the site (ocrl_pool_transformer_dropout_mask: site 300 + 8*layer + which, any seed and p), read as
    [B,h,T,T4][..., :T], is the mask the host restatement builds"""
    from ocrl_amd import _lib
    B, T, h, dh, p, seed, site = case
    T4 = (T + 3) & ~3
    layer, which = (site - 300) // 8, (site - 300) % 8
    m = torch.full((B, h, T, T4), float("nan"), device="cuda")
    _lib.check(_lib_handle().ocrl_pool_transformer_dropout_mask(layer, which, m.numel(), p, seed, P(m), None))
    torch.cuda.synchronize()
    dev = m[..., :T].cpu()
    assert set(dev.unique().tolist()) == {0.0, 1.0}
    assert torch.equal(dev.bool(), R.keep_mask(seed, site, p, B, h, T))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("case", R.STRIDE_CASES, ids=_ids)
def test_stride_layouts(case, layout):
    """q/k/v and dq/dk/dv have row stride ld, o and dO row stride d: one qkv tensor (ld = 3d), three dense tensors (ld = d), and
    ld = 3d + 8 with NaN / sentinel pad columns; the three layouts also agree bit for bit"""
    B, T, h, dh, p, seed, site = case
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    keep = R.keep_mask(seed, site, p, B, h, T) if p > 0 else None
    out = run(_lib_handle(), q, k, v, dO, h, layout, p, seed, site)
    check(f"strides {_ids(case)} {layout}", out, R.attention_ref(q, k, v, h, dO, keep, p))
    if layout != "packed":
        base = run(_lib_handle(), q, k, v, dO, h, "packed", p, seed, site)
        assert torch.equal(_bits(out["o"]), _bits(base["o"])) and torch.equal(_bits(out["lse"]), _bits(base["lse"]))
        for name, _ in FORMS:
            for n in ("dq", "dk", "dv"):
                assert torch.equal(_bits(out[name][n]), _bits(base[name][n])), (name, n)


@pytest.mark.parametrize("B,T,h,dh", [(1, 200, 2, 48), (2, 129, 2, 64)])
def test_softmax_range(B, T, h, dh):
    """scores spanning about +-60 and one logit of -1e6 per row: the online max / rescale must stay finite and accurate.  The bar is
    computed here: the same math in fp32 PyTorch on the CPU is measured against fp64, and the kernel may be max(2e-5, 4 x that) off
    (4: MFMA summation order and the fast exponential)."""
    q, k, v, dO = R.make_wide_range_inputs(B, T, h, dh)
    ref = R.attention_ref(q, k, v, h, dO)
    f32 = R.attention_ref(q, k, v, h, dO, dtype=torch.float32)
    out = run(_lib_handle(), q, k, v, dO, h, "packed")           # run() asserts that no result is inf or NaN
    e = errors(out, ref)
    bad = {}
    for key, err in e.items():
        n = key.split(".")[-1]
        e32 = relerr(f32[n], ref[n], floor=grad_floor(ref) if n in ("dq", "dk", "dv") else 0.0)
        bar = max(TOL, 4 * e32)
        log(f"[attention edges] softmax range B{B} T{T} h{h} dh{dh} {key}: kernel {err:.2e} fp32-cpu {e32:.2e} bar {bar:.2e}")
        if not err <= bar:
            bad[key] = (err, e32, bar)
    assert not bad, bad


@pytest.mark.parametrize("case", R.REPRO_CASES, ids=_ids)
def test_bitwise_reproducible(case):
    """two calls on the same inputs give the same bits in both backward forms; at p = 0, image 0 of a B = 3 call equals the B = 1
    call (the block-to-work mapping changes with B, the arithmetic must not)"""
    B, T, h, dh, p, seed, site = case
    q, k, v, dO = R.make_inputs(B, T, h, dh)
    L = _lib_handle()
    a, b = (run(L, q, k, v, dO, h, "packed", p, seed, site) for _ in range(2))
    same = lambda x, y, sl=slice(None): torch.equal(_bits(x[sl]), _bits(y))
    assert same(a["o"], b["o"]) and same(a["lse"], b["lse"])
    for name, _ in FORMS:
        for n in ("dq", "dk", "dv"):
            assert same(a[name][n], b[name][n]), (name, n)
    if p == 0:
        one = run(L, q[:1], k[:1], v[:1], dO[:1], h, "packed")
        assert same(a["o"], one["o"], slice(0, 1)) and same(a["lse"], one["lse"], slice(0, 1))
        for name, _ in FORMS:
            for n in ("dq", "dk", "dv"):
                assert same(a[name][n], one[name][n], slice(0, 1)), (name, n)
