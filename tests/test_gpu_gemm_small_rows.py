"""The dX form of the fp32 GEMM (k-contiguous A, n-contiguous B) with at most 64 rows and N not a multiple of 128 runs on single-buffered
64x64 tiles.  Its epilogue stages each wave's 32x32 accumulator tile in a 32x36 LDS patch over the operand tiles; the launch must
reserve all four patches or tile rows 60..63 come back wrong.  Checked through the C ABI and through the short pooling path, whose
dslots product has that shape at B = 2, K = 31, rep_dim = 192."""
import pytest
import torch

from oracle import pooling_oracle as PO
from tests.gpu_util import log, relerr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M", [33, 60, 61, 62, 64])
@pytest.mark.parametrize("N", [64, 68, 192])
def test_dx_form_with_up_to_64_rows(M, N):
    from ocrl_amd import _lib
    L = _lib.lib()
    K = 128
    g = torch.Generator().manual_seed(M * 1000 + N)
    A, Bm = torch.randn(M, K, generator=g).cuda(), torch.randn(K, N, generator=g).cuda()
    C = torch.full((M, N), float("nan"), device="cuda")
    _lib.check(L.ocrl_gemm(_lib.ptr(A), _lib.ptr(Bm), _lib.ptr(C), M, N, K, K, N, N, 1, 0, 1.0, None, 0, None, 0, None, 0, 1, None, None))
    torch.cuda.synchronize()
    ref = A.double() @ Bm.double()
    assert relerr(C, ref) < 1e-5


def test_short_pooling_path_dslots_at_62_rows():
    from tests.test_gpu_pooling import run_hip
    cfg = PO.default_cfg(num_slots=31, rep_dim=192, dim_feedforward=512)
    P = PO.formula_params(cfg)
    g = torch.Generator().manual_seed(4)
    slots, cot = torch.randn(2, 31, 192, generator=g), torch.randn(2, cfg.d_model, generator=g)
    out, grads, ds = run_hip(cfg, P, slots, cot)
    r_out, r_g, r_ds = PO.loss_and_grads(P, slots, cfg, cot, dtype=torch.float64)
    e = dict(out=relerr(out, r_out), dslots=relerr(ds, r_ds))
    log(f"[gemm 62 rows] short pooling path: out {e['out']:.2e} dslots {e['dslots']:.2e}")
    assert e["out"] < 2e-5 and e["dslots"] < 3e-4, e
