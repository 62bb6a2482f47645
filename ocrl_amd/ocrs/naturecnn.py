"""NatureCNN encoder (ocrs/naturecnn/naturecnn.py:10-17, naturecnn_module.py:11-63, configs/ocr/naturecnn.yaml) on the HIP backend.

``NatureCNN_Module`` holds real ``nn.Conv2d`` / ``nn.Linear`` layers at the reference's ``Sequential`` indices (the ReLU slots are
``nn.Identity``, as in poolings/mlp.py), so ``state_dict()`` keys, shapes and default initialisation are the reference's, reference
checkpoints load unchanged, and SB3's ``ortho_init`` finds the layers.  The containers' ``forward`` is never called: the arithmetic is
``ocrl_naturecnn_fwd/_bwd`` (strided implicit-GEMM convolutions on the fp32 MFMA, the Linear on the library's GEMM) wrapped in a
``torch.autograd.Function``, so PPO trains the encoder end to end through torch autograd.  No CPU fallback: a CPU tensor raises.

Differences from the reference: ``get_loss(obs, with_rep=True)`` without ``use_cnn_feat`` returns the representation
(the reference reads a non-existent ``self._nets``), and the observation gets no gradient (``obs.requires_grad`` raises)."""
from types import SimpleNamespace

import torch
from torch import nn

from .. import _lib
from .base import Base

_CONVS = ((32, 8, 4), (64, 4, 2), (64, 3, 1), (128, 3, 1))       # (out channels, kernel, stride) of _cnn.0 / .2 / .4 / .6


def _map_size(obs_size, n_convs):
    s = obs_size
    for _, k, st in _CONVS[:n_convs]:
        s = (s - k) // st + 1 if s >= k else 0
    return s


def _check_inputs(obs, params, dims, cin):
    """everything the C entry points cannot check themselves: they get no parameter sizes, and derive the Linear's input width from the
    observation's H and W.  So the observation must flatten to the width the Linear was built for (the reference's Linear raises
    torch's shape-mismatch error otherwise), and every parameter must have the shape, dtype and device the kernels read it with."""
    groups, feat, use_feat, rep = dims
    n_conv = 4 if feat == 2 else 3
    if obs.dim() != 4 or obs.shape[1] != cin:
        raise ValueError(f"ocrl_amd.ocrs.NatureCNN: expected observations [B, {cin}, H, W], got {list(obs.shape)}")
    shapes, c = [], cin
    for cout, k, _ in _CONVS[:n_conv]:
        shapes += [(cout, c, k, k), (cout,)]
        c = cout
    if not use_feat:
        lin = params[2 * n_conv]                              # module 0's Linear weight; every module must match it
        oh, ow = _map_size(obs.shape[2], n_conv), _map_size(obs.shape[3], n_conv)
        if lin.dim() != 2 or c * oh * ow != lin.shape[1]:
            raise ValueError(f"ocrl_amd.ocrs.NatureCNN: {obs.shape[2]} x {obs.shape[3]} observations flatten to {c} x {oh} x {ow} = "
                             f"{c * oh * ow} features, but the Linear takes {list(lin.shape)[1:]} (built for another obs_size)")
        shapes += [(rep, c * oh * ow), (rep,)]
    shapes = shapes * groups
    if len(params) != len(shapes) or any(tuple(p.shape) != sh for p, sh in zip(params, shapes)):
        raise ValueError(f"ocrl_amd.ocrs.NatureCNN: parameter shapes {[list(p.shape) for p in params]} are not the encoder's "
                         f"{[list(sh) for sh in shapes]}")
    if not obs.is_cuda:
        raise RuntimeError("ocrl_amd.ocrs: tensors must live on the GPU (there is no CPU fallback)")
    if obs.requires_grad:
        raise RuntimeError("ocrl_amd.ocrs.NatureCNN: the observation gets no gradient (the first convolution's input gradient is not built)")
    for p in params:
        if p.dtype != torch.float32 or p.device != obs.device:
            raise RuntimeError(f"ocrl_amd.ocrs.NatureCNN: parameters must be float32 on the observations' device {obs.device} "
                               f"(got {p.dtype} on {p.device})")


def _encode(obs, dims, params, save):
    """one ocrl_naturecnn_fwd call; returns (out, ws)"""
    groups, feat, use_feat, rep = dims
    L = _lib.lib()
    B, C, H, W = obs.shape
    n = L.ocrl_naturecnn_ws_floats(B, H, W, C, groups, feat, use_feat, rep)
    if n == 0:
        raise ValueError(f"ocrl_amd.ocrs.NatureCNN: shape not supported: batch {B} of {C} x {H} x {W} images, {groups} module(s), "
                         f"cnn_feat_size {feat}, use_cnn_feat {bool(use_feat)}, rep_dim {rep}: "
                         + L.ocrl_last_error().decode())
    ws = torch.empty(n, device=obs.device, dtype=torch.float32)
    if use_feat:
        n_conv = 4 if feat == 2 else 3
        oh, ow = _map_size(H, n_conv), _map_size(W, n_conv)
        out = torch.empty(B, oh * ow, _CONVS[n_conv - 1][0], device=obs.device, dtype=torch.float32)
    elif groups == 1:
        out = torch.empty(B, rep, device=obs.device, dtype=torch.float32)
    else:
        out = torch.empty(B, groups, rep, device=obs.device, dtype=torch.float32)
    arr = _lib.ptrs(params)
    st = _lib.stream()
    _lib.check(L.ocrl_naturecnn_fwd(_lib.ptr(obs), arr, _lib.ptr(out), B, H, W, C, groups, feat, use_feat, rep, int(save), _lib.ptr(ws), n, st))
    return out, ws


class _NatureCNNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obs, dims, *params):
        ps = [p.contiguous() for p in params]
        out, ws = _encode(obs, dims, ps, save=True)
        # through save_for_backward, so that torch's version check raises if the observation or a weight changes in place before
        # the backward (the backward reads both again)
        ctx.save_for_backward(obs, *ps)
        ctx.dims, ctx.ws = dims, ws
        return out

    @staticmethod
    def backward(ctx, dout):
        groups, feat, use_feat, rep = ctx.dims
        obs, *ps = ctx.saved_tensors
        L = _lib.lib()
        B, C, H, W = obs.shape
        dout = dout.contiguous().float()
        gs = [torch.empty_like(p) for p in ps]
        arr = _lib.ptrs(ps)
        garr = _lib.ptrs(gs)
        st = _lib.stream()
        _lib.check(L.ocrl_naturecnn_bwd(_lib.ptr(obs), _lib.ptr(dout), arr, garr, B, H, W, C, groups, feat, use_feat, rep,
                                        _lib.ptr(ctx.ws), ctx.ws.numel(), st))
        return (None, None, *gs)


def run_naturecnn(obs, dims, params, cin):
    """the encoders' forward: an autograd node that keeps the activations when a parameter needs a gradient, a bare call otherwise
    (a no_grad rollout keeps nothing)"""
    _check_inputs(obs, params, dims, cin)
    obs = obs.contiguous().float()
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _NatureCNNFn.apply(obs, dims, *params)
    return _encode(obs, dims, [p.contiguous() for p in params], save=False)[0]


class NatureCNN_Module(nn.Module):
    # the encoder trains through torch autograd (its parameters get .grad from the RL loss); the extractor and the pooling wrapper admit
    # such modules for the trainable path beside SLATE's finetune_through_slots
    trains_through_autograd = True

    def __init__(self, ocr_config, env_config) -> None:
        super().__init__()
        obs_size = env_config.obs_size
        obs_channels = env_config.obs_channels
        self._use_cnn_feat = bool(ocr_config.use_cnn_feat)
        self._cnn_feat_size = int(ocr_config.cnn_feat_size)
        if self._use_cnn_feat:
            if self._cnn_feat_size == 4:
                self.rep_dim, self.num_slots = 64, 4 ** 2
            elif self._cnn_feat_size == 2:
                self.rep_dim, self.num_slots = 128, 2 ** 2
            else:                                             # the reference leaves rep_dim / num_slots unset and fails later
                raise ValueError(f"NatureCNN: use_cnn_feat needs cnn_feat_size 2 or 4 (got {self._cnn_feat_size})")
        else:
            self.rep_dim = int(ocr_config.rep_dim)
            self.num_slots = 1
        n_conv = 4 if self._cnn_feat_size == 2 else 3        # the 4th conv comes with cnn_feat_size 2, with or without use_cnn_feat
        cnn = []
        cin = obs_channels
        for cout, k, s in _CONVS[:n_conv]:
            cnn += [nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=0), nn.Identity()]
            cin = cout
        if not self._use_cnn_feat:
            cnn.append(nn.Flatten())
        self._cnn = nn.Sequential(*cnn)
        side = _map_size(obs_size, n_conv)
        if side < 1:
            raise ValueError(f"NatureCNN: obs_size {obs_size} leaves an empty feature map (at least {36 if n_conv == 3 else 52} needed)")
        self._obs_channels = obs_channels
        if not self._use_cnn_feat:
            n_flatten = cin * side * side                     # the reference's dry forward pass at obs_size
            self._linear = nn.Sequential(nn.Linear(n_flatten, self.rep_dim), nn.Identity())

    def _param_list(self):
        convs = [m for m in self._cnn if isinstance(m, nn.Conv2d)]
        lin = [self._linear[0]] if not self._use_cnn_feat else []
        return [p for m in convs + lin for p in (m.weight, m.bias)]

    def _dims(self):
        return (1, self._cnn_feat_size, int(self._use_cnn_feat), 0 if self._use_cnn_feat else self.rep_dim)

    def forward(self, obs):
        return run_naturecnn(obs, self._dims(), self._param_list(), self._obs_channels)

    def get_loss(self, obs, with_rep=False):
        if with_rep:
            return {}, self(obs)
        return {}

    def get_samples(self, obs) -> dict:
        return {}


class NatureCNN(Base):
    def __init__(self, ocr_config, env_config) -> None:
        self._module = NatureCNN_Module(ocr_config, env_config)
        super().__init__(ocr_config, env_config)
        learning = getattr(ocr_config, "learning", None)
        if learning is not None and hasattr(learning, "lr"):      # ocrs/base.py:20-25
            self._opt = torch.optim.Adam(self._module.parameters(), lr=learning.lr)

    def get_samples(self, obs) -> dict:
        return {}


def forced_config(ocr_config):
    """the NatureCNN config MultipleCNN gives each of its modules (cnn_feat_size 4, use_cnn_feat False), as a copy: the reference
    writes these two values into the caller's config (multiple_cnn_module.py:20-22)"""
    return SimpleNamespace(rep_dim=ocr_config.rep_dim, cnn_feat_size=4, use_cnn_feat=False)
