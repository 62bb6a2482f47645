"""Training services the SLATE path touches (reference: utils/tools.py). wandb / h5py / omegaconf are optional."""
import numpy as np
import torch

from .. import _lib


def to_device(batch, device):
    """utils/tools.py:182-191"""
    if isinstance(batch, list):
        return [b.to(device) for b in batch]
    if isinstance(batch, dict):
        return {k: v.to(device) for k, v in batch.items()}
    return batch.to(device)


def obs_from_uint8(u8):
    """uint8 [B,H,W,C] on the GPU -> fp32 [B,C,H,W] in [0,1] (utils/datasets.py:17 + the H2D copy of train_ocr.py:52-53), converted by
    the library's kernel: the host ships a quarter of the bytes and never touches the pixels"""
    if not (u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 4):
        raise RuntimeError("obs_from_uint8: expected a uint8 [B,H,W,C] tensor on the GPU")
    u8 = u8.contiguous()
    B, H, W, C = u8.shape
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=u8.device)
    _lib.check(_lib.lib().ocrl_obs_u8_to_f32(_lib.ptr(u8), _lib.ptr(out), B, H, W, C, _lib.stream(u8.device)))
    return out


def get_item(x):
    """utils/tools.py:195-199"""
    if not torch.is_tensor(x):
        return x
    if len(x.shape) == 0:
        return x.item()
    return x.detach().cpu().numpy()


def for_viz(x):
    """utils/tools.py:203-205"""
    return np.array(x.clamp(0, 1).permute(0, 2, 3, 1).detach().cpu().numpy() * 255.0, dtype=np.uint8)


def visualize(images):
    """utils/tools.py:209-219: width-concatenate [B,3,H,W] images and [B,K,3,H,W] stacks"""
    viz = []
    for img in images:
        if img.dim() == 4:
            viz.append(img)
        else:
            viz += list(torch.unbind(img, dim=1))
    return torch.cat(viz, dim=-1)


def ari_from_pair_sums(sum_ij, sum_a, sum_b, n):
    """the adjusted Rand index from its pair sums: sum_ij C(n_ij) over the contingency table, sum_i C(a_i) over its row sums, sum_j C(b_j)
    over its column sums and the number of samples n, C(x) = x (x - 1) / 2.  Shared by the numpy path and the device path."""
    sum_ij, sa, sb = np.int64(sum_ij), np.int64(sum_a), np.int64(sum_b)
    n = np.int64(n)
    tot = n * (n - 1) // 2
    if tot == 0:
        return 1.0
    exp = sa * sb / tot
    mx = 0.5 * (sa + sb)
    if mx == exp:
        return 1.0
    return float((sum_ij - exp) / (mx - exp))


def _adjusted_rand_score(a, b):
    """sklearn.metrics.adjusted_rand_score (pair-counting form) for two integer label vectors"""
    a = np.asarray(a).ravel()
    b = np.asarray(b).ravel()
    n = a.size
    _, ai = np.unique(a, return_inverse=True)
    _, bi = np.unique(b, return_inverse=True)
    cont = np.zeros((ai.max() + 1, bi.max() + 1), dtype=np.int64)
    np.add.at(cont, (ai, bi), 1)
    comb = lambda x: x * (x - 1) // 2
    return ari_from_pair_sums(comb(cont).sum(), comb(cont.sum(1)).sum(), comb(cont.sum(0)).sum(), n)


ARI_MAX_CHANNELS = _lib.CONSTANTS["OCRL_ARI_MAX_CHANNELS"]


def _on_device(*ts):
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() >= 3 and t.shape[1] <= ARI_MAX_CHANNELS for t in ts)


def ari_counts(truth, pred, fuse_fg=False):
    """ocrl_ari_counts on the current stream: truth [B, Ct, ...] and pred [B, Cp or K, ...] CUDA fp32 score stacks over the same pixels
    (any strides that flatten(2) can express are read in place).  Returns (table [B, Ct, Cp] int32, sums [B, 3] int64) on the device;
    fuse_fg: pred holds K = Cp - 1 maps and the foreground channel 1 - truth[:, -1] is formed in the kernel."""
    from .. import _bridge
    t, p = truth.flatten(2), pred.flatten(2)
    B, Ct, N = t.shape
    Cp = p.shape[1] + (1 if fuse_fg else 0)
    if p.shape[0] != B or p.shape[2] != N:
        raise RuntimeError(f"ari_counts: truth {tuple(truth.shape)} and pred {tuple(pred.shape)} do not cover the same pixels")
    table = torch.empty(B, Ct, Cp, dtype=torch.int32, device=t.device)
    sums = torch.empty(B, 3, dtype=torch.int64, device=t.device)
    _bridge.launch(t.device, _lib.lib().ocrl_ari_counts, _lib.ptr(t), *t.stride(), Ct, _lib.ptr(p), *p.stride(), Cp, int(fuse_fg), B, N,
                   _lib.ptr(table), _lib.ptr(sums))
    return table, sums


def _ari_on_device(truth, pred, fuse_fg):
    n = truth[0, 0].numel()
    sums = ari_counts(truth, pred, fuse_fg)[1].cpu().numpy()        # 3 B int64: the only device-to-host copy
    return [ari_from_pair_sums(s[0], s[1], s[2], n) for s in sums]


def calculate_ari(true_masks, pred_masks):
    """utils/tools.py:309-320.  CUDA fp32 stacks of at most 32 channels are counted on the GPU (ocrl_ari_counts); the integers are exact
    and the closing arithmetic is shared, so both paths return equal floats."""
    if _on_device(true_masks, pred_masks) and true_masks.device == pred_masks.device:
        return _ari_on_device(true_masks, pred_masks, False)
    t = torch.argmax(true_masks.flatten(2), dim=1).cpu().numpy()
    p = torch.argmax(pred_masks.flatten(2), dim=1).cpu().numpy()
    return [_adjusted_rand_score(t[b], p[b]) for b in range(t.shape[0])]


def segmentation_ari(masks, attns):
    """per-image ARI of the foreground-masked slot maps against the ground truth (slate_module.py:211-216, iodine_module.py:263-267):
    masks [B, Ct, 1, H, W] with the background channel last, attns [B, K, 1, H, W] (a strided view is read in place).  Equal to
    calculate_ari(masks, cat([attns * fg, fg], 1)) with fg = 1 - masks[:, -1:]; on the GPU the masking, both argmax passes and the
    counting are one kernel."""
    if _on_device(masks, attns) and masks.device == attns.device and attns.shape[1] < ARI_MAX_CHANNELS:
        return _ari_on_device(masks, attns, True)
    fg_mask = 1 - masks[:, -1].unsqueeze(1)
    return calculate_ari(masks, torch.cat([attns * fg_mask, fg_mask], dim=1))
