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

from .. import _bridge, _lib
from .._bridge import NATURE_CONVS, conv_map_size, conv_shapes
from .base import Base

_WHO = "ocrl_amd.ocrs.NatureCNN"


def _check_inputs(obs, params, dims, cin):
    """everything the C entry points cannot check themselves: they get no parameter sizes, and derive the Linear's input width from the
    observation's H and W.  So the observation must flatten to the width the Linear was built for (the reference's Linear raises
    torch's shape-mismatch error otherwise), and every parameter must have the shape, dtype and device the kernels read it with.
    Returns (observation, parameters) as the kernels read them"""
    groups, feat, use_feat, rep = dims
    n_conv = 4 if feat == 2 else 3
    if obs.dim() != 4 or obs.shape[1] != cin:
        raise ValueError(f"{_WHO}: expected observations [B, {cin}, H, W], got {list(obs.shape)}")
    shapes = conv_shapes(cin, n_conv)
    if not use_feat:
        lin = params[2 * n_conv]                              # module 0's Linear weight; every module must match it
        c, oh, ow = NATURE_CONVS[n_conv - 1][0], conv_map_size(obs.shape[2], n_conv), conv_map_size(obs.shape[3], n_conv)
        if lin.dim() != 2 or c * oh * ow != lin.shape[1]:
            raise ValueError(f"{_WHO}: {obs.shape[2]} x {obs.shape[3]} observations flatten to {c} x {oh} x {ow} = "
                             f"{c * oh * ow} features, but the Linear takes {list(lin.shape)[1:]} (built for another obs_size)")
        shapes += [(rep, c * oh * ow), (rep,)]
    x, ps = _bridge.inputs(_WHO, obs, params, shapes * groups)
    if obs.requires_grad:
        raise RuntimeError(f"{_WHO}: the observation gets no gradient (the first convolution's input gradient is not built)")
    return x, ps


def _encode(obs, dims, params, save):
    """one ocrl_naturecnn_fwd call; returns (out, ws)"""
    groups, feat, use_feat, rep = dims
    L, dev = _lib.lib(), obs.device
    B, C, H, W = obs.shape
    ws = _bridge.workspace(_WHO, L.ocrl_naturecnn_ws_floats(B, H, W, C, *dims), dev,
                           f"batch {B} of {C} x {H} x {W} images, {groups} module(s), cnn_feat_size {feat}, use_cnn_feat {bool(use_feat)}, rep_dim {rep}")
    if use_feat:
        n_conv = 4 if feat == 2 else 3
        shape = (B, conv_map_size(H, n_conv) * conv_map_size(W, n_conv), NATURE_CONVS[n_conv - 1][0])
    else:
        shape = (B, rep) if groups == 1 else (B, groups, rep)
    out = torch.empty(shape, device=dev, dtype=torch.float32)
    _bridge.launch(dev, L.ocrl_naturecnn_fwd, _lib.ptr(obs), _lib.ptrs(params), _lib.ptr(out), B, H, W, C, *dims, int(save), _lib.ptr(ws), ws.numel())
    return out, ws


class _NatureCNNFn(torch.autograd.Function):
    """over the observation and the parameters `ps` as _check_inputs returned them; `params` are their attached originals, which get
    the gradients"""

    @staticmethod
    def forward(ctx, obs, dims, ps, *params):
        out, ws = _encode(obs, dims, ps, save=True)
        ctx.save_for_backward(obs, *ps)
        ctx.dims, ctx.ws = dims, ws
        return out

    @staticmethod
    def backward(ctx, dout):
        obs, *ps = ctx.saved_tensors
        B, C, H, W = obs.shape
        dout = _bridge.cotangent(dout)
        gs = [torch.empty_like(p) for p in ps]
        _bridge.launch(obs.device, _lib.lib().ocrl_naturecnn_bwd, _lib.ptr(obs), _lib.ptr(dout), _lib.ptrs(ps), _lib.ptrs(gs), B, H, W, C, *ctx.dims,
                       _lib.ptr(ctx.ws), ctx.ws.numel())
        return (None, None, None, *gs)


def run_naturecnn(obs, dims, params, cin):
    """the encoders' forward: an autograd node that keeps the activations when a parameter needs a gradient, a bare call otherwise
    (a no_grad rollout keeps nothing)"""
    x, ps = _check_inputs(obs, params, dims, cin)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _NatureCNNFn.apply(x, dims, ps, *params)
    return _encode(x, dims, ps, save=False)[0]


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
        for cout, k, s in NATURE_CONVS[:n_conv]:      # _cnn.0 / .2 / .4 / .6
            cnn += [nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=0), nn.Identity()]
            cin = cout
        if not self._use_cnn_feat:
            cnn.append(nn.Flatten())
        self._cnn = nn.Sequential(*cnn)
        side = conv_map_size(obs_size, n_conv)
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
