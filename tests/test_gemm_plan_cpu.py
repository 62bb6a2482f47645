"""CPU-only: the GEMM's C-ABI descriptor matches the header, ocrl_gemm_plan reports the documented dispatch rule (what gemm_launch runs,
gemm_plan in csrc/gemm.hip), forced combinations that are not built are refused, and the case list of tests/test_gpu_gemm_dispatch.py
reaches every kernel instantiation the launchers can produce.  No device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000        # a 16-byte aligned address: the plan never dereferences a pointer


@pytest.fixture(scope="module")
def L():
    from ocrl_amd import _lib
    return _lib


def plan(L, **kw):
    out = (ctypes.c_int * 6)()
    kw.setdefault("A", FAKE)
    kw.setdefault("B", FAKE)
    kw.setdefault("C", FAKE)
    rc = L.lib().ocrl_gemm_plan(L.gemm_desc(**kw), out)
    return None if rc else tuple(out)


def mm(akc, bkc, M, N, K, **kw):
    """descriptor fields of a compact product"""
    return dict(akc=akc, bkc=bkc, M=M, N=N, K=K, lda=K if akc else M, ldb=K if bkc else N, ldc=N, **kw)


def header_fields(struct):
    """field names and C types of a descriptor struct of include/ocrl_hip.h, in declaration order"""
    hdr = open(os.path.join(ROOT, "include", "ocrl_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
    names, types = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            parts = [f.strip() for f in decl.split(",")]
            ctype = re.match(r"(.*?)(\w+)$", parts[0]).group(1).strip()
            for f in parts:
                names.append(re.search(r"(\w+)$", f).group(1))
                types.append(ctype)
    return names, types


def test_desc_struct_matches_the_header(L):
    fields, _ = header_fields("ocrl_gemm_desc")
    assert [n for n, _ in L.GemmDesc._fields_] == fields
    assert L.lib().ocrl_gemm_desc_size() == ctypes.sizeof(L.GemmDesc)


@pytest.mark.parametrize("struct,cls,size_fn", [("ocrl_conv_desc", "ConvDesc", "ocrl_conv_desc_size"),
                                                ("ocrl_conv_wgrad_desc", "ConvWgradDesc", "ocrl_conv_wgrad_desc_size")])
def test_conv_desc_structs_match_the_header(L, struct, cls, size_fn):
    fields, types = header_fields(struct)
    mirror = getattr(L, cls)
    assert [n for n, _ in mirror._fields_] == fields
    # pointers mirror pointers, ints mirror ints: equal sizes alone would not show an int where a 4-byte float is declared
    for (n, t), c in zip(mirror._fields_, types):
        assert t is (ctypes.c_void_p if c.endswith("*") else {"int": ctypes.c_int}[c]), (n, c)
    assert getattr(L.lib(), size_fn)() == ctypes.sizeof(mirror)


def test_conv_desc_makers_default_to_absent():
    from ocrl_amd import _lib
    d = _lib.conv_desc(B=2, ks=5, relu=2, x=FAKE)
    assert (d.B, d.ks, d.relu, d.x) == (2, 5, 2, FAKE)
    assert (d.bias, d.posmap, d.mask, d.mask_elu, d.transposed, d.low_latency) == (None, None, None, 0, 0, 0)
    g = _lib.conv_wgrad_desc(cin=3, cin_pad=8, accumulate=1)
    assert (g.cin, g.cin_pad, g.accumulate, g.db) == (3, 8, 1, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(ks=4, cin=64, cin_pad=64), "no kernel"),
    (dict(ks=3, cin=3, cin_pad=8), "no kernel"),
    (dict(ks=5, cin=9, cin_pad=8), "cin"),
    (dict(ks=5, cin=64, cin_pad=64, relu=3), "relu"),
    (dict(ks=5, cin=64, cin_pad=64, mask_elu=1), "mask_elu"),
    (dict(ks=5, cin=3, cin_pad=8, transposed=1), "transposed"),
    (dict(ks=5, cin=64, cin_pad=64, bias=FAKE + 4), "aligned"),
    (dict(ks=5, cin=64, cin_pad=64, B=0), "non-empty"),
    (dict(ks=5, cin=64, cin_pad=64, transposed=1, ws_floats=25 * 64 * 64), "workspace"),
])
def test_unsupported_convolutions_are_refused_before_any_launch(L, kw, msg):
    """ocrl_conv2d_ex returns 1 with a message for what no kernel serves; the checks come before the first launch, so the fake
    addresses are never touched"""
    kw = dict(kw)
    ws_floats = kw.pop("ws_floats", 1 << 20)
    base = dict(x=FAKE, w=FAKE, y=FAKE, B=1, H=4, W=4)
    base.update(kw)
    assert L.lib().ocrl_conv2d_ex(L.conv_desc(**base), FAKE, ws_floats, None) == 1
    assert msg in L.lib().ocrl_last_error().decode()
    if not {"relu", "mask_elu", "transposed", "bias"} & set(kw):
        g = dict(x=FAKE, dy=FAKE, dw=FAKE, B=base["B"], H=4, W=4, ks=base["ks"], cin=base["cin"], cin_pad=base["cin_pad"])
        assert L.lib().ocrl_conv2d_bwd_weight_ex(L.conv_wgrad_desc(**g), FAKE, 16, None) == 1


def rule(akc, bkc, M, N, K):
    """the documented selection (csrc/gemm.hip gemm_plan): (BM, BN, single buffer)"""
    if akc and N == 192 and K >= 1024 and M >= 4096:
        return 128, 192, 1
    if not akc and not bkc and N == 192 and K >= 4096:
        return 128, 192, 1
    sb = 1 if akc else 0
    if N % 128 == 0:
        return (128 if M > 64 else 64), 128, sb
    return (128 if M > 64 else 64), 64, sb


# (akc, bkc, M, N, K) of the model's products: batch-128 SLATE at 64x64 / 128x128 (4096 / 16384 tokens per image set), d_model 192,
# vocabulary 4096, MLP 768, slot widths 64 / 128, and their dX / dW forms
MODEL_SHAPES = [(1, 1, 128 * 256, 192, 192), (1, 1, 128 * 256, 4096, 192), (1, 0, 128 * 256, 192, 4096), (0, 0, 4096, 192, 128 * 256),
                (0, 0, 192, 192, 128 * 256), (1, 1, 128 * 256, 768, 192), (1, 0, 128 * 256, 192, 768), (0, 0, 768, 192, 128 * 256),
                (0, 0, 192, 768, 128 * 256), (1, 1, 128 * 7, 192, 64), (1, 0, 128 * 7, 64, 192), (0, 0, 192, 64, 128 * 7),
                (1, 1, 2 * 16, 4096, 192), (1, 1, 60, 64, 64), (1, 0, 62, 192, 128), (0, 0, 64, 128, 4096), (1, 1, 4096, 192, 1024),
                (1, 0, 4095, 192, 1024), (1, 1, 4096, 192, 1020), (0, 0, 128, 192, 4096), (0, 0, 128, 192, 4092), (0, 1, 64, 192, 8192),
                (1, 1, 128 * 1024, 192, 192), (0, 0, 192, 192, 128 * 1024)]


def _env_overrides():
    return [k for k in ("OCRL_GEMM_TILE", "OCRL_GEMM_SB") if os.environ.get(k)]


@pytest.mark.parametrize("akc,bkc,M,N,K", MODEL_SHAPES)
def test_plan_reports_the_documented_rule(L, akc, bkc, M, N, K):
    if _env_overrides():
        pytest.skip(f"{_env_overrides()} set: the dispatch is overridden")
    p = plan(L, **mm(akc, bkc, M, N, K))
    assert p is not None, L.lib().ocrl_last_error()
    assert p[:3] == rule(akc, bkc, M, N, K)
    assert p[3:] == (0, 0, 2 * akc + bkc)
    assert plan(L, **mm(akc, bkc, M, N, K, adrop_p=0.1, adrop_ld=(K if akc else M)))[:4] == rule(akc, bkc, M, N, K) + (1,)


@pytest.mark.parametrize("N_out,K_in,rows", [(192, 192, 128 * 256), (4096, 192, 128 * 256), (768, 192, 128 * 256), (192, 768, 128 * 256),
                                             (192, 4096, 128 * 256), (576, 192, 4096), (192, 192, 4095), (64, 192, 896), (192, 64, 896),
                                             (4, 64, 4100), (64, 48, 777), (128, 192, 4096), (192, 100, 5000)])
def test_weight_gradient_split_count_matches_the_plan(L, N_out, K_in, rows):
    """The split-count rule of the Linear weight gradients (lin_splitk_count in csrc/gemm.hip) divides its ~1024 workgroups by the output
    tiles gemm_plan cuts for the dW form.  Pins that tiling: one 128x192 column tile for 192 input features over >= 4096 rows, else
    128- or 64-wide column tiles, 128-row tiles above 64 outputs"""
    if _env_overrides():
        pytest.skip(f"{_env_overrides()} set: the dispatch is overridden")
    col_tiles = 1 if (K_in == 192 and rows >= 4096) else -(-K_in // (128 if K_in % 128 == 0 else 64))
    p = plan(L, **mm(0, 0, N_out, K_in, rows))
    assert p is not None, L.lib().ocrl_last_error()
    assert -(-K_in // p[1]) == col_tiles
    assert p[0] == 128 or N_out <= 64


def instantiations():
    """every gemm_kernel<BM, BN, AKC, BKC, SB, XF, EPI> the launchers build, as (BM, BN, SB, XF, EPI, 2*akc + bkc)"""
    out = set()
    for akc, bkc in ((1, 1), (1, 0), (0, 0), (0, 1)):
        for bm, bn in ((128, 128), (128, 64), (64, 128), (64, 64), (128, 192)):
            if (bm, bn) == (128, 192) and not akc and bkc:
                continue
            for sb in (0, 1):
                for xf in ((0, 1, 2) if akc or not bkc else (0, 1)):
                    out.add((bm, bn, sb, xf, 0, 2 * akc + bkc))
    out |= {(128, 128, 1, 0, 1, 3), (128, 128, 1, 0, 2, 3), (128, 128, 1, 0, 3, 2)}
    return out


def test_gpu_sweep_reaches_every_instantiation(L):
    from tests import test_gpu_gemm_dispatch as S
    seen = set()
    for c in S.CASES:
        present = S.buffers_present(c)
        p = plan(L, **S.desc_fields(c, lambda n: FAKE if n in present else 0))
        assert p is not None, (S._cid(c), L.lib().ocrl_last_error())
        if c["tile"]:
            assert (p[0] * 1000 + p[1], p[2]) == (c["tile"], c["sb"]), S._cid(c)
        seen.add(p)
    want = instantiations()
    assert len(want) == 109
    assert not (want - seen), sorted(want - seen)
    assert not (seen - want), sorted(seen - want)


@pytest.mark.parametrize("kw,msg", [
    (dict(mm(0, 1, 128, 192, 256), force_tile=128192), "not built"),
    (dict(mm(1, 1, 128, 128, 256), force_tile=32032), "not built"),
    (dict(mm(1, 1, 128, 128, 256), force_sb=2), "force_sb"),
    (dict(mm(0, 1, 128, 128, 256), a_mode=2, x_lse=FAKE), "operand transforms"),
    (dict(mm(1, 1, 128, 256, 64), epi_mode=1, stat=FAKE, force_tile=64064), "128x128"),
    (dict(mm(1, 1, 128, 256, 64), epi_mode=1, stat=FAKE, force_sb=0), "128x128"),
])
def test_forced_combinations_that_are_not_built_are_refused(L, kw, msg):
    assert plan(L, **kw) is None
    assert msg in L.lib().ocrl_last_error().decode()


def test_forced_choice_is_honoured(L):
    for tile in (128128, 128064, 64128, 64064, 128192):
        for sb in (0, 1):
            p = plan(L, **mm(1, 0, 4096, 192, 1024, force_tile=tile, force_sb=sb))
            assert p == (tile // 1000, tile % 1000, sb, 0, 0, 2)
    assert plan(L, **mm(1, 1, 128, 256, 64, epi_mode=1, stat=FAKE, force_tile=128128, force_sb=1)) == (128, 128, 1, 0, 1, 3)
