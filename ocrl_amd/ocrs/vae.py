"""VAE representation module (ocrs/vaes/vae.py, vae_module.py, ocrs/common/models.py:49-93, configs/ocr/vae.yaml) on the HIP backend.

``VAE_Module`` holds real ``nn.Conv2d`` / ``nn.Linear`` layers at the reference's ``Sequential`` indices (the ReLU of each Conv2dBlock
lives in the block, the PixelShuffle slots are parameter-free ``nn.PixelShuffle``), with the reference's initialisation, so
``state_dict()`` keys and shapes are the reference's and a reference ``vae.pth`` loads unchanged.  The containers' ``forward`` is never
called: the arithmetic is ``ocrl_vae_fwd/_bwd`` wrapped in two ``torch.autograd.Function``s, the encoder alone (the rollout; backward
from d rep) and the whole loss (backward from d loss and d rep, summed), so the module trains through torch autograd and torch Adam.
No CPU fallback: a CPU tensor raises.

Differences from the reference: the observation gets no gradient (``obs.requires_grad`` raises), and
``get_loss(obs, masks)`` as ``train_ocr.py`` calls it (a mask tensor in the ``with_rep`` slot) returns the metrics alone."""
import math

import numpy as np
import torch
from torch import nn

from .. import _bridge, _lib
from .._lib import ptrs as _ptrs
from .base import AutogradUpdate, Base

_WHO = "ocrl_amd.ocrs.VAE"


def stages(obs_size, cnn_feat_size):
    """n = log2(obs_size / cnn_feat_size); ValueError unless that is a positive integer (models.py:55 asserts the same)"""
    r = obs_size / cnn_feat_size
    n = int(round(math.log2(r))) if r >= 1 else -1
    if r != int(r) or n < 1 or 2 ** n != r:
        raise ValueError(f"VAE: obs_size / cnn_feat_size must be a power of two >= 2 (got {obs_size} / {cnn_feat_size})")
    return n


def _conv(cin, cout, k, stride=1, padding=0, kaiming=True):
    """ocrs/common/networks.py conv2d: kaiming-uniform(relu) for Conv2dBlock, xavier-uniform for the plain conv2d; zero bias"""
    m = nn.Conv2d(cin, cout, k, stride, padding)
    if kaiming:
        nn.init.kaiming_uniform_(m.weight, nonlinearity="relu")
    else:
        nn.init.xavier_uniform_(m.weight)
    nn.init.zeros_(m.bias)
    return m


class _Block(nn.Module):
    """Conv2dBlock: the parameters live in ``.m`` (state_dict key ``<i>.m.weight``)"""

    def __init__(self, cin, cout, k, stride=1, padding=0):
        super().__init__()
        self.m = _conv(cin, cout, k, stride, padding)


class _Encoder(nn.Module):
    def __init__(self, obs_channels, n):
        super().__init__()
        layers, cin = [], obs_channels
        for _ in range(n):
            layers += [_Block(cin, 64, 2, 2), _Block(64, 64, 1), _Block(64, 64, 1), _Block(64, 64, 1)]
            cin = 64
        layers.append(_conv(64, 64, 1, kaiming=False))
        self._encoder = nn.Sequential(*layers)


class _Decoder(nn.Module):
    def __init__(self, obs_channels, n):
        super().__init__()
        layers = [_Block(64, 64, 1)]
        for _ in range(n):
            layers += [_Block(64, 64, 3, 1, 1), _Block(64, 64, 1), _Block(64, 64, 1), _Block(64, 256, 1), nn.PixelShuffle(2)]
        layers.append(_conv(64, obs_channels, 1, kaiming=False))
        self._decoder = nn.Sequential(*layers)


def param_shapes(C, n, f, L):
    """the shapes the C entry points read every parameter at, in state_dict order, from the configuration alone"""
    shapes, cin = [], C
    for _ in range(n):
        shapes += [(64, cin, 2, 2), (64,)] + [(64, 64, 1, 1), (64,)] * 3
        cin = 64
    F_ = 64 * f * f
    shapes += [(64, 64, 1, 1), (64,), (L, F_), (L,), (L, F_), (L,), (F_, L), (F_,), (64, 64, 1, 1), (64,)]
    for _ in range(n):
        shapes += [(64, 64, 3, 3), (64,), (64, 64, 1, 1), (64,), (64, 64, 1, 1), (64,), (256, 64, 1, 1), (256,)]
    shapes += [(C, 64, 1, 1), (C,)]
    return shapes


def _check_inputs(obs, params, shapes, C, S):
    """(observation, parameters) as the kernels read them"""
    if obs.dim() != 4 or obs.shape[1] != C or obs.shape[2] != S or obs.shape[3] != S:
        raise ValueError(f"{_WHO}: expected observations [B, {C}, {S}, {S}], got {list(obs.shape)}")
    x, ps = _bridge.inputs(_WHO, obs, params, shapes)
    if obs.requires_grad:
        raise RuntimeError(f"{_WHO}: the observation gets no gradient (the first convolution's input gradient is not built)")
    return x, ps


def _ws(obs, dims, full):
    S, C, f, L, cnn, _ = dims
    return _bridge.workspace(_WHO, _lib.lib().ocrl_vae_ws_floats(obs.shape[0], S, C, f, L, cnn, int(full)), obs.device,
                             f"batch {obs.shape[0]} of {C} x {S} x {S} images, cnn_feat_size {f}, latent_dim {L}")


def _rep_like(obs, dims):
    S, C, f, L, cnn, _ = dims
    shape = (obs.shape[0], f * f, 64) if cnn else (obs.shape[0], L)
    return torch.empty(shape, device=obs.device, dtype=torch.float32)


def _fwd(obs, dims, params, full, eps=None, recon=None):
    """one ocrl_vae_fwd call; returns (rep, metrics or None, ws)"""
    S, C, f, L, cnn, kw = dims
    ws = _ws(obs, dims, full)
    rep = _rep_like(obs, dims)
    metrics = torch.empty(3, device=obs.device, dtype=torch.float32) if full else None
    _bridge.launch(obs.device, _lib.lib().ocrl_vae_fwd, _lib.ptr(obs), _ptrs(params), _lib.ptr(eps), _lib.ptr(rep),
                   _lib.ptr(metrics), _lib.ptr(recon), obs.shape[0], S, C, f, L, cnn, float(kw), int(full), _lib.ptr(ws), ws.numel())
    return rep, metrics, ws


def _bwd(obs, eps, dims, params, dloss, drep, ws, full):
    S, C, f, L, cnn, kw = dims
    n = len(params) if full else 4 * stages(S, f) * 2 + 4            # the encoder's and _mu's entries
    gs = [torch.empty_like(p) for p in params[:n]]
    gptr = _ptrs(gs + [None] * (len(params) - n))
    _bridge.launch(obs.device, _lib.lib().ocrl_vae_bwd, _lib.ptr(obs), _lib.ptr(eps), _ptrs(params), _lib.ptr(dloss),
                   _lib.ptr(drep), gptr, obs.shape[0], S, C, f, L, cnn, float(kw), int(full), _lib.ptr(ws), ws.numel())
    if cnn and not full:
        gs[-2:] = [None, None]                  # the token output does not pass through _mu
    return gs + [None] * (len(params) - n)


class _EncodeFn(torch.autograd.Function):
    """the encoder (and _mu): obs -> rep; backward from d rep.  Over the observation and the parameters `ps` as _check_inputs returned
    them; `params` are their attached originals, which get the gradients"""

    @staticmethod
    def forward(ctx, obs, dims, ps, *params):
        rep, _, ws = _fwd(obs, dims, ps, False)
        ctx.save_for_backward(obs, *ps)
        ctx.dims, ctx.ws = dims, ws
        return rep

    @staticmethod
    def backward(ctx, drep):
        obs, *ps = ctx.saved_tensors
        gs = _bwd(obs, None, ctx.dims, ps, None, _bridge.cotangent(drep), ctx.ws, False)
        return (None, None, None, *gs)


class _LossFn(torch.autograd.Function):
    """get_loss: (obs, eps) -> (loss, mse, kld, rep); backward from d loss and d rep, summed (mse and kld are detached metrics)"""

    @staticmethod
    def forward(ctx, obs, eps, dims, ps, *params):
        rep, m, ws = _fwd(obs, dims, ps, True, eps=eps)
        ctx.save_for_backward(obs, eps, *ps)
        ctx.dims, ctx.ws = dims, ws
        ctx.set_materialize_grads(False)
        mse, kld = m[1].clone(), m[2].clone()
        ctx.mark_non_differentiable(mse, kld)
        return m[0].clone(), mse, kld, rep

    @staticmethod
    def backward(ctx, dloss, _dmse, _dkld, drep):
        obs, eps, *ps = ctx.saved_tensors
        if dloss is None and drep is None:
            return (None, None, None, None) + (None,) * len(ps)
        # a missing cotangent counts as zero: without d loss the C backward skips the decoder and KL terms (zero gradients there)
        if dloss is not None:
            dloss = dloss.reshape(1)
        gs = _bwd(obs, eps, ctx.dims, ps, _bridge.cotangent(dloss), _bridge.cotangent(drep), ctx.ws, True)
        return (None, None, None, None, *gs)


class VAE_Module(nn.Module):
    # the module trains through torch autograd (its parameters get .grad); the extractor and the pooling wrapper admit such modules
    trains_through_autograd = True

    def __init__(self, ocr_config, env_config) -> None:
        super().__init__()
        obs_size = int(env_config.obs_size)
        obs_channels = int(env_config.obs_channels)
        latent_dim = int(ocr_config.latent_dim)
        self._kld_weight = float(ocr_config.learning.kld_weight)
        self._use_cnn_feat = bool(ocr_config.use_cnn_feat)
        self._cnn_feat_size = f = int(ocr_config.cnn_feat_size)
        if self._use_cnn_feat:
            self.rep_dim, self.num_slots = 64, f ** 2
        else:
            self.rep_dim, self.num_slots = latent_dim, 1
        n = stages(obs_size, f)
        self._obs_size, self._obs_channels, self._latent_dim, self._n = obs_size, obs_channels, latent_dim, n
        self._enc = _Encoder(obs_channels, n)
        self._mu = nn.Linear(64 * f * f, latent_dim)
        self._var = nn.Linear(64 * f * f, latent_dim)
        self._in_dec = nn.Linear(latent_dim, 64 * f * f)
        self._dec = _Decoder(obs_channels, n)
        self._max_batch = 0
        self._gen = None

    def set_seed(self, seed: int) -> None:
        """seeds the generator of the reparameterisation noise (train_ocr.py calls it once per rank)"""
        self._gen = torch.Generator(device=next(self.parameters()).device)
        self._gen.manual_seed(int(seed))

    def _dims(self):
        return (self._obs_size, self._obs_channels, self._cnn_feat_size, self._latent_dim, int(self._use_cnn_feat), self._kld_weight)

    def _params(self):
        return list(self.parameters())

    def _shapes(self):
        return param_shapes(self._obs_channels, self._n, self._cnn_feat_size, self._latent_dim)

    def _check(self, obs, params):
        return _check_inputs(obs, params, self._shapes()[:len(params)], self._obs_channels, self._obs_size)

    def _enc_params(self):
        n = 4 * self._n * 2 + 4
        return self._params()[:n]

    def forward(self, obs):
        """mu [B, latent], or with use_cnn_feat img_to_slot(enc(obs)) [B, f^2, 64]; the decoder does not run"""
        params = self._enc_params()
        obs, ps = self._check(obs, params)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _EncodeFn.apply(obs, self._dims(), ps, *params)
        return _fwd(obs, self._dims(), ps, False)[0]

    def draw_eps(self, obs):
        """eps = randn_like(std) [B, latent] on the observations' device (vae_module.py:52)"""
        return torch.randn(obs.shape[0], self._latent_dim, device=obs.device, dtype=torch.float32, generator=self._gen
                           if self._gen is not None and self._gen.device == obs.device else None)

    def loss_terms(self, obs, eps=None):
        """(loss, mse, kld, rep) through the HIP kernels; eps drawn here when not given (tests pass recorded noise)"""
        params = self._params()
        obs, ps = self._check(obs, params)
        if eps is None:
            eps = self.draw_eps(obs)
        eps = eps.contiguous().float()
        if eps.shape != (obs.shape[0], self._latent_dim) or eps.device != obs.device:
            raise ValueError(f"{_WHO}: eps must be [{obs.shape[0]}, {self._latent_dim}] on {obs.device} (got {list(eps.shape)} on {eps.device})")
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _LossFn.apply(obs, eps, self._dims(), ps, *params)
        rep, m, _ = _fwd(obs, self._dims(), ps, True, eps=eps)
        return m[0], m[1], m[2], rep

    def get_loss(self, obs, with_rep=False, eps=None):
        loss, mse, kld, rep = self.loss_terms(obs, eps)
        metrics = {"loss": loss, "mse": mse.detach(), "kld": -kld.detach()}
        if with_rep is True:
            return metrics, rep
        return metrics

    @torch.no_grad()
    def reconstruct(self, obs, eps=None):
        """the decoder's output [B, C, S, S] for obs (vae_module.py:80-87)"""
        obs, ps = self._check(obs, self._params())
        if eps is None:
            eps = self.draw_eps(obs)
        recon = torch.empty_like(obs)
        _fwd(obs, self._dims(), ps, True, eps=eps.contiguous().float(), recon=recon)
        return recon

    def get_samples(self, obs) -> dict:
        from ..utils.tools import for_viz
        return {"samples": np.concatenate([for_viz(obs), for_viz(self.reconstruct(obs))], axis=-2)}


class VAE(AutogradUpdate, Base):
    def __init__(self, ocr_config, env_config) -> None:
        self._module = VAE_Module(ocr_config, env_config)
        super().__init__(ocr_config, env_config)
        learning = getattr(ocr_config, "learning", None)
        if learning is not None and hasattr(learning, "lr"):      # ocrs/base.py:20-25
            self._opt = torch.optim.Adam(self._module.parameters(), lr=learning.lr)

    def get_loss(self, obs, with_rep=False):
        return self._module.get_loss(obs, with_rep)
