"""fp64 reference of one clip + Adam step on flat buffers (ocrs/base.py:60-74: clip_grad_norm_ then torch.optim.Adam), built on the
oracle's own adam_update / grad_clip_inf and on the L2 clip of oracle/iodine_oracle.py restated without its cast of the norm to fp32.
tests/test_optimizer_ref_cpu.py pins it to torch.optim.Adam + torch.nn.utils.clip_grad_norm_; tests/test_gpu_optimizer.py holds the
HIP step against it."""
from types import SimpleNamespace

import torch

from oracle import slate_oracle as O


def grad_norm(grads, norm_type):
    """total norm of a list of fp64 tensors: "inf" -> max |g| (oracle.slate_oracle.grad_clip_inf), 2 -> sqrt(sum g^2) (the sum of
    oracle.iodine_oracle.grad_clip_l2, kept in fp64).  NaN and inf propagate as in torch."""
    if not grads:
        return torch.zeros((), dtype=torch.float64)
    if norm_type == "inf":
        return O.grad_clip_inf(grads, 1.0)[0]
    assert float(norm_type) == 2.0, norm_type
    return torch.sqrt(sum((g ** 2).sum() for g in grads))


def ref_step(p, g, m, v, tensors, lrs, clip, norm_type, t, gscale=1.0, has_grad=None):
    """p, g, m, v: flat tensors (any float dtype, any device); tensors: [(offset, numel, group)]; lrs: per group; clip: 0 / None = no
    clipping; norm_type: "inf" or 2; t: Adam's step count after the increment; has_grad: per-tensor flag (default: all).
    Returns fp64 CPU copies p, m, v after the step, the norm of the scaled gradient and the clip coefficient."""
    p, m, v = (x.detach().double().cpu().clone() for x in (p, m, v))
    g = g.detach().double().cpu() * gscale
    has_grad = [True] * len(tensors) if has_grad is None else list(has_grad)
    live = [tn for tn, h in zip(tensors, has_grad) if h]
    norm = grad_norm([g[o:o + n] for o, n, _ in live], norm_type)
    coef = torch.clamp(clip / (norm + 1e-6), max=1.0) if clip else torch.ones((), dtype=torch.float64)
    for o, n, grp in live:          # a tensor without a gradient is skipped entirely, as torch's Adam skips .grad is None
        O.adam_update(p[o:o + n], g[o:o + n] * coef, m[o:o + n], v[o:o + n], t, float(lrs[grp]))
    return SimpleNamespace(p=p, m=m, v=v, norm=norm, coef=coef)
