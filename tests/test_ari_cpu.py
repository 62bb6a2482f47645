"""CPU-only checks of the segmentation-ARI path: the closing arithmetic shared by the numpy and the device path (ari_from_pair_sums), the
argument checks of ocrl_ari_counts (no GPU is needed to reject a call), the get_ari_mse configuration, and the unchanged CPU-tensor
branch of calculate_ari."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ocrl_amd.utils.config import compose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")


def _pair_sums(a, b):
    """the three pair sums from a dense contingency table built in numpy"""
    cont = np.zeros((int(a.max()) + 1, int(b.max()) + 1), dtype=np.int64)
    np.add.at(cont, (a, b), 1)
    comb = lambda x: x * (x - 1) // 2
    return comb(cont).sum(), comb(cont.sum(1)).sum(), comb(cont.sum(0)).sum()


def _label_pairs():
    rs = np.random.RandomState(7)
    cases = []
    for ca, cb, n in [(2, 2, 2), (2, 3, 17), (3, 7, 225), (5, 4, 500), (6, 7, 4096), (7, 7, 16384), (17, 17, 65536), (2, 17, 65536), (16, 2, 1000)]:
        cases.append((f"random_{ca}x{cb}_n{n}", rs.randint(0, ca, n), rs.randint(0, cb, n)))
    z = np.zeros(300, dtype=np.int64)
    r = rs.randint(0, 6, 300)
    cases.append(("one_cluster_each", z, z.copy()))
    cases.append(("one_cluster_vs_many", z, r))
    cases.append(("n1", np.array([3]), np.array([0])))
    cases.append(("identical", r, r.copy()))
    cases.append(("identical_renamed", r, (r + 2) % 6))
    return cases


@pytest.mark.parametrize("tag,a,b", _label_pairs(), ids=[c[0] for c in _label_pairs()])
def test_ari_from_pair_sums_matches_numpy_path_and_sklearn(tag, a, b):
    from sklearn.metrics import adjusted_rand_score
    from ocrl_amd.utils.tools import _adjusted_rand_score, ari_from_pair_sums
    got = ari_from_pair_sums(*_pair_sums(a, b), a.size)
    assert isinstance(got, float)
    assert got == _adjusted_rand_score(a, b)
    assert got == pytest.approx(adjusted_rand_score(a, b), abs=1e-12)


def test_ari_from_pair_sums_accepts_plain_ints():
    """the device path hands numpy int64 scalars, a C host plain integers: the same float either way"""
    from ocrl_amd.utils.tools import ari_from_pair_sums
    a, b = np.array([0, 0, 1, 1, 2, 2, 2]), np.array([0, 1, 1, 1, 2, 2, 0])
    s = _pair_sums(a, b)
    assert ari_from_pair_sums(*[int(x) for x in s], 7) == ari_from_pair_sums(*s, np.int64(7))
    assert ari_from_pair_sums(0, 0, 0, 1) == 1.0


def test_ari_counts_is_exported_and_rejects_bad_arguments_without_a_gpu():
    from ocrl_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "ocrl_ari_counts")
    for Ct, Cp, B, N in [(0, 7, 1, 16), (6, 33, 1, 16), (33, 1, 1, 16), (6, 0, 1, 16), (6, 7, 0, 16), (6, 7, 1, 0), (6, 7, 1, 2 ** 31)]:
        rc = L.ocrl_ari_counts(None, 0, 0, 0, Ct, None, 0, 0, 0, Cp, 0, B, N, None, None, None)
        assert rc != 0 and b"invalid" in L.ocrl_last_error(), (Ct, Cp, B, N, L.ocrl_last_error())
    # valid sizes, null pointers: rejected as well, before anything is launched
    assert L.ocrl_ari_counts(None, 0, 0, 0, 6, None, 0, 0, 0, 7, 1, 1, 16, None, None, None) != 0 and b"invalid" in L.ocrl_last_error()
    assert L.ocrl_abi_version() == 5
    with pytest.raises(RuntimeError, match="invalid"):
        _lib.check(L.ocrl_ari_counts(None, 0, 0, 0, 0, None, 0, 0, 0, 1, 0, 1, 1, None, None, None))


def test_get_ari_mse_config_composes_with_reference_keys():
    c = compose(CFG, "get_ari_mse", ["ocr=slate", "dataset=random-N5C4S4S2"])
    assert c.batch_size == 32 and c.bg_mask_idx == -1
    assert c.ocr_checkpoint.to_dict() == {"entity": "", "project": "", "run_id": "", "file": "", "local_file": ""}
    assert c.ocr.name == "SLATE" and c.dataset.name == "RandomN5C4S4S2" and c.wandb.project == "ocrl-ari-mse"
    assert c.run_dir == "./outputs/get_ari/SLATE-RandomN5C4S4S2"
    c2 = compose(CFG, "get_ari_mse", ["ocr=iodine", "dataset=random-N5C4S4S2", "dataset.with_masks=True", "bg_mask_idx=0",
                                      "ocr_checkpoint.local_file=a/b.pth"])
    assert c2.bg_mask_idx == 0 and c2.dataset.with_masks is True and c2.ocr_checkpoint.local_file == "a/b.pth"
    with pytest.raises(ValueError, match="ocr"):
        compose(CFG, "get_ari_mse", ["dataset=random-N5C4S4S2"])
    with pytest.raises(ValueError, match="dataset"):
        compose(CFG, "get_ari_mse", ["ocr=slate"])


def test_background_last_moves_one_channel():
    from get_ari_mse import background_last
    m = torch.arange(2 * 4 * 3).reshape(2, 4, 1, 1, 3).float()
    assert background_last(m, -1) is m and background_last(m, 3) is m
    assert torch.equal(background_last(m, 0), m[:, [1, 2, 3, 0]])
    assert torch.equal(background_last(m, -3), m[:, [0, 2, 3, 1]])
    with pytest.raises(RuntimeError):
        background_last(m, 4)


def test_calculate_ari_on_cpu_tensors_is_pinned_to_sklearn():
    """the CPU-tensor branch is the path every earlier release took: argmax labels, then the pair-counting ARI per image"""
    from sklearn.metrics import adjusted_rand_score
    from ocrl_amd.utils.tools import calculate_ari, segmentation_ari
    g = torch.Generator().manual_seed(3)
    B, Ct, K, S = 4, 6, 5, 16
    true = torch.rand(B, Ct, 1, S, S, generator=g)
    pred = torch.rand(B, K + 1, 1, S, S, generator=g)
    got = calculate_ari(true, pred)
    assert isinstance(got, list) and len(got) == B and all(isinstance(x, float) for x in got)
    t, p = true.flatten(2).argmax(1).numpy(), pred.flatten(2).argmax(1).numpy()
    for b in range(B):
        assert got[b] == pytest.approx(adjusted_rand_score(t[b], p[b]), abs=1e-12)
    # segmentation_ari on CPU tensors is the three torch lines of the encoders' get_loss followed by calculate_ari
    lab = torch.randint(0, Ct, (B, S, S), generator=g)
    masks = torch.nn.functional.one_hot(lab, Ct).permute(0, 3, 1, 2).unsqueeze(2).float()
    attns = torch.softmax(torch.randn(B, K, 1, S, S, generator=g), dim=1)
    fg = 1 - masks[:, -1].unsqueeze(1)
    assert segmentation_ari(masks, attns) == calculate_ari(masks, torch.cat([attns * fg, fg], dim=1))
    # more than 32 channels never reach the kernel, on any device
    wide = torch.rand(1, 40, 1, 4, 4, generator=g)
    assert calculate_ari(wide, wide) == [1.0]
