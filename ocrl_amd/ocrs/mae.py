"""Masked autoencoder (ocrs/mae/mae.py, mae_module.py, models_mae.py, util/pos_embed.py, configs/ocr/mae.yaml) on the HIP backend.

``MAE_Module`` holds real ``nn.Parameter`` / ``nn.Conv2d`` / ``nn.Linear`` / ``nn.LayerNorm`` containers under ``_mae.`` with the
reference's names, shapes and initialisation (timm 0.3.2's ``PatchEmbed`` and ``Block`` restated from their definition), so
``state_dict()`` is the reference's and a reference ``mae.pth`` loads unchanged; timm is not needed.  The containers' ``forward`` is
never called: the arithmetic is ``ocrl_mae_fwd/_bwd`` wrapped in two ``torch.autograd.Function``s, the full-patch encoder (the rollout;
backward from d rep) and the masked pre-training loss (backward from d loss and d latent, summed), so the module trains through torch
autograd and a torch optimiser.  No CPU fallback: a CPU tensor raises.

Differences from the reference: the observation gets no gradient (``obs.requires_grad`` raises); the masking noise is
drawn here (``torch.rand`` from the generator ``set_seed`` seeds) and ranked on the device, with ties broken by index."""
import numpy as np
import torch
from torch import nn

from .. import _bridge, _lib
from .._lib import ptrs as _ptrs
from .base import AutogradUpdate, Base

_WHO = "ocrl_amd.ocrs.MAE"
VIT = {"base": (768, 12, 12), "large": (1024, 24, 16)}      # width, depth, heads
DECODER = (512, 8, 16)
MLP_RATIO = 4
LN_EPS = 1e-6


def sincos_1d(dim, pos):
    """[M, dim] table of positions pos [M]: sin then cos of pos / 10000^(2 i / dim), in float64"""
    omega = 1.0 / 10000 ** (np.arange(dim // 2, dtype=np.float64) / (dim / 2.0))
    out = np.einsum("m,d->md", pos.reshape(-1).astype(np.float64), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_2d(dim, grid, cls_token=True):
    """the fixed 2-D sin-cos table [(1 +) grid^2, dim] (float64): the first half of the columns encodes the column index of a patch,
    the second half its row index (the reference meshgrids with w first), a zero row in front for the CLS token"""
    if dim % 4:
        raise ValueError(f"{_WHO}: the sin-cos table needs a width that is a multiple of 4 (got {dim})")
    ax = np.arange(grid, dtype=np.float32)
    col, row = np.meshgrid(ax, ax)                     # col[i, j] = j, row[i, j] = i
    t = np.concatenate([sincos_1d(dim // 2, col), sincos_1d(dim // 2, row)], axis=1)
    return np.concatenate([np.zeros([1, dim]), t], axis=0) if cls_token else t


class _Attention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, MLP_RATIO * dim)
        self.fc2 = nn.Linear(MLP_RATIO * dim, dim)


class _Block(nn.Module):
    """timm's Block: x += proj(attn(norm1(x))); x += fc2(GELU(fc1(norm2(x))))"""

    def __init__(self, dim):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = _Attention(dim)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = _Mlp(dim)


class _PatchEmbed(nn.Module):
    def __init__(self, patch, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)


class _MAE(nn.Module):
    """the parameter containers of MaskedAutoencoderViT, registered in its order"""

    def __init__(self, grid, patch, enc, dec):
        super().__init__()
        (D, depth, _), (Dd, ddepth, _) = enc, dec
        L = grid * grid
        self.patch_embed = _PatchEmbed(patch, D)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.pos_embed = nn.Parameter(torch.zeros(1, L + 1, D), requires_grad=False)
        self.blocks = nn.ModuleList([_Block(D) for _ in range(depth)])
        self.norm = nn.LayerNorm(D, eps=LN_EPS)
        self.decoder_embed = nn.Linear(D, Dd)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, Dd))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, L + 1, Dd), requires_grad=False)
        self.decoder_blocks = nn.ModuleList([_Block(Dd) for _ in range(ddepth)])
        self.decoder_norm = nn.LayerNorm(Dd, eps=LN_EPS)
        self.decoder_pred = nn.Linear(Dd, patch * patch * 3)
        # initialize_weights: fixed sin-cos tables, the patch projection like a Linear, normal tokens, xavier Linears, LayerNorm (1, 0)
        self.pos_embed.data.copy_(torch.from_numpy(sincos_2d(D, grid)).float().unsqueeze(0))
        self.decoder_pos_embed.data.copy_(torch.from_numpy(sincos_2d(Dd, grid)).float().unsqueeze(0))
        w = self.patch_embed.proj.weight.data
        nn.init.xavier_uniform_(w.view(w.shape[0], -1))
        nn.init.normal_(self.cls_token, std=0.02)
        nn.init.normal_(self.mask_token, std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)


def param_shapes(L, patch, enc, dec):
    """the shapes the C entry points read every parameter at, in state_dict order"""
    (D, depth, _), (Dd, ddepth, _) = enc, dec

    def block(d):
        return [(d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (MLP_RATIO * d, d), (MLP_RATIO * d,), (d, MLP_RATIO * d), (d,)]
    P = 3 * patch * patch
    return ([(1, 1, D), (1, L + 1, D), (1, 1, Dd), (1, L + 1, Dd), (D, 3, patch, patch), (D,)] + block(D) * depth + [(D,), (D,), (Dd, D), (Dd,)]
            + block(Dd) * ddepth + [(Dd,), (Dd,), (P, Dd), (P,)])


def n_encoder_params(depth):
    """entries of `w` up to and including the encoder's final norm"""
    return 6 + 12 * depth + 2


def _dims_args(dims, len_keep, full):
    S, p, (D, depth, h), (Dd, ddepth, dh) = dims
    return (S, p, D, depth, h, Dd, ddepth, dh, int(len_keep), int(full))


def _ws(obs, dims, len_keep, full):
    S, p = dims[0], dims[1]
    return _bridge.workspace(_WHO, _lib.lib().ocrl_mae_ws_floats(obs.shape[0], *_dims_args(dims, len_keep, full)), obs.device,
                             f"batch {obs.shape[0]} of 3 x {S} x {S} images, patch {p}, encoder {dims[2]}, decoder {dims[3]}, len_keep {len_keep}")


def _fwd(obs, dims, params, len_keep, full, noise=None, want_pred=False):
    """one ocrl_mae_fwd call; returns (rep, metrics, pred, mask, ws)"""
    S, p, (D, _, _), _ = dims
    B, L = obs.shape[0], (S // p) ** 2
    ws = _ws(obs, dims, len_keep, full)
    new = lambda *sh: torch.empty(sh, device=obs.device, dtype=torch.float32)
    rep = new(B, (len_keep if full else L) + 1, D)
    metrics = new(2) if full else None
    pred = new(B, L, 3 * p * p) if full and want_pred else None
    mask = new(B, L) if full and want_pred else None
    _bridge.launch(obs.device, _lib.lib().ocrl_mae_fwd, _lib.ptr(obs), _ptrs(params), _lib.ptr(noise), _lib.ptr(rep), _lib.ptr(metrics),
                   _lib.ptr(pred), _lib.ptr(mask), None, B, *_dims_args(dims, len_keep, full), _lib.ptr(ws), ws.numel())
    return rep, metrics, pred, mask, ws


def _bwd(obs, dims, params, len_keep, dloss, drep, ws, full):
    n = len(params) if full else n_encoder_params(dims[2][1])
    frozen = (1, 3)                                    # the sin-cos tables get no gradient
    gs = [None if i in frozen or (not full and i == 2) else torch.empty_like(p) for i, p in enumerate(params[:n])]
    gs += [None] * (len(params) - n)
    _bridge.launch(obs.device, _lib.lib().ocrl_mae_bwd, _lib.ptr(obs), _ptrs(params), _lib.ptr(dloss), _lib.ptr(drep), _ptrs(gs), obs.shape[0],
                   *_dims_args(dims, len_keep, full), _lib.ptr(ws), ws.numel())
    return gs


class _EncodeFn(torch.autograd.Function):
    """encode_full_patches: obs -> rep [B, L + 1, D]; backward from d rep.  `ps` are the parameters as the kernels read them, `params`
    their attached originals, which get the gradients"""

    @staticmethod
    def forward(ctx, obs, dims, ps, *params):
        rep, _, _, _, ws = _fwd(obs, dims, ps, 0, False)
        ctx.save_for_backward(obs, *ps)
        ctx.dims, ctx.ws = dims, ws
        return rep

    @staticmethod
    def backward(ctx, drep):
        obs, *ps = ctx.saved_tensors
        gs = _bwd(obs, ctx.dims, ps, 0, None, _bridge.cotangent(drep), ctx.ws, False)
        return (None, None, None, *gs)


class _LossFn(torch.autograd.Function):
    """the masked loss: (obs, noise) -> (loss, latent [B, len_keep + 1, D]); backward from d loss and d latent, summed"""

    @staticmethod
    def forward(ctx, obs, noise, dims, len_keep, ps, *params):
        rep, m, _, _, ws = _fwd(obs, dims, ps, len_keep, True, noise=noise)
        ctx.save_for_backward(obs, noise, *ps)
        ctx.dims, ctx.len_keep, ctx.ws = dims, len_keep, ws
        ctx.set_materialize_grads(False)
        return m[1].clone(), rep

    @staticmethod
    def backward(ctx, dloss, drep):
        obs, _noise, *ps = ctx.saved_tensors
        if dloss is None and drep is None:
            return (None,) * (5 + len(ps))
        if dloss is not None:                          # a missing cotangent counts as zero
            dloss = dloss.reshape(1)
        gs = _bwd(obs, ctx.dims, ps, ctx.len_keep, _bridge.cotangent(dloss), _bridge.cotangent(drep), ctx.ws, True)
        return (None, None, None, None, None, *gs)


class MAE_Module(nn.Module):
    # the module trains through torch autograd (its parameters get .grad); the extractor and the pooling wrapper admit such modules
    trains_through_autograd = True

    def __init__(self, ocr_config, env_config) -> None:
        super().__init__()
        self._masking_ratio = float(ocr_config.masking_ratio)
        self._return_cls = bool(ocr_config.return_cls)
        S, p = int(env_config.obs_size), int(ocr_config.patch_size)
        if S % p:
            raise ValueError(f"{_WHO}: obs_size must be a multiple of patch_size (got {S} / {p})")
        if ocr_config.vit_size not in VIT:
            raise ValueError(f"{_WHO}: vit_size must be one of {sorted(VIT)} (got {ocr_config.vit_size!r})")
        # `_test_dims` = ((D, depth, heads), (Dd, ddepth, dheads)): small stacks for the tests; the reference has base and large only
        enc, dec = getattr(ocr_config, "_test_dims", None) or (VIT[ocr_config.vit_size], DECODER)
        self._obs_size, self._patch_size, self._enc, self._dec = S, p, tuple(enc), tuple(dec)
        self._num_patches = (S // p) ** 2
        self.rep_dim = self._enc[0]
        self.num_slots = 1 if self._return_cls else self._num_patches
        self._mae = _MAE(S // p, p, self._enc, self._dec)
        self._max_batch = 0
        self._gen = None

    def set_seed(self, seed: int) -> None:
        """seeds the generator of the masking noise (train_ocr.py calls it once per rank)"""
        self._gen = torch.Generator(device=next(self.parameters()).device)
        self._gen.manual_seed(int(seed))

    @property
    def len_keep(self):
        return int(self._num_patches * (1 - self._masking_ratio))

    def _dims(self):
        return (self._obs_size, self._patch_size, self._enc, self._dec)

    def _params(self):
        return list(self.parameters())

    def _check(self, obs, params):
        S = self._obs_size
        if obs.dim() != 4 or tuple(obs.shape[1:]) != (3, S, S):
            raise ValueError(f"{_WHO}: expected observations [B, 3, {S}, {S}], got {list(obs.shape)}")
        shapes = param_shapes(self._num_patches, self._patch_size, self._enc, self._dec)
        x, ps = _bridge.inputs(_WHO, obs, params, shapes[:len(params)])
        if obs.requires_grad:
            raise RuntimeError(f"{_WHO}: the observation gets no gradient (the patch projection's input gradient is not built)")
        return x, ps

    def encode_full_patches(self, obs):
        """[B, L + 1, D]: every patch through the encoder and its final norm, the CLS row first"""
        params = self._params()[:n_encoder_params(self._enc[1])]
        obs, ps = self._check(obs, params)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _EncodeFn.apply(obs, self._dims(), ps, *params)
        return _fwd(obs, self._dims(), ps, 0, False)[0]

    def forward(self, obs):
        rep = self.encode_full_patches(obs)
        return rep[:, 0] if self._return_cls else rep[:, 1:]

    def draw_noise(self, obs):
        """noise = rand(B, L) on the observations' device (models_mae.py random_masking)"""
        return torch.rand(obs.shape[0], self._num_patches, device=obs.device, dtype=torch.float32, generator=self._gen
                          if self._gen is not None and self._gen.device == obs.device else None)

    def _noise(self, obs, noise):
        if noise is None:
            noise = self.draw_noise(obs)
        noise = noise.contiguous().float()
        if noise.shape != (obs.shape[0], self._num_patches) or noise.device != obs.device:
            raise ValueError(f"{_WHO}: noise must be [{obs.shape[0]}, {self._num_patches}] on {obs.device} (got {list(noise.shape)} on {noise.device})")
        return noise

    def loss_terms(self, obs, noise=None):
        """(loss, latent [B, len_keep + 1, D]) through the HIP kernels; the noise is drawn here when not given (tests pass recorded noise)"""
        params = self._params()
        obs, ps = self._check(obs, params)
        noise = self._noise(obs, noise)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _LossFn.apply(obs, noise, self._dims(), self.len_keep, ps, *params)
        rep, m, _, _, _ = _fwd(obs, self._dims(), ps, self.len_keep, True, noise=noise)
        return m[1], rep

    def get_loss(self, obs, with_rep=False, noise=None):
        loss, _ = self.loss_terms(obs, noise)
        metrics = {"loss": loss, "mse": loss.detach()}
        if with_rep is True:
            return metrics, self(obs)
        return metrics

    @torch.no_grad()
    def predict(self, obs, noise=None, masking_ratio=None):
        """(pred [B, L, 3 p p] in patchify's order, mask [B, L]) of one masked pass"""
        obs, ps = self._check(obs, self._params())
        keep = self.len_keep if masking_ratio is None else int(self._num_patches * (1 - masking_ratio))
        _, _, pred, mask, _ = _fwd(obs, self._dims(), ps, keep, True, noise=self._noise(obs, noise), want_pred=True)
        return pred, mask

    def unpatchify(self, x):
        """[B, L, p p 3] -> [B, 3, S, S]"""
        p, g = self._patch_size, self._obs_size // self._patch_size
        return x.reshape(x.shape[0], g, g, p, p, 3).permute(0, 5, 1, 3, 2, 4).reshape(x.shape[0], 3, g * p, g * p)

    def get_samples(self, obs) -> dict:
        from ..utils.tools import for_viz
        pred, mask = self.predict(obs)
        pred = self.unpatchify(pred)
        if self._masking_ratio == 0.0:
            return {"samples": np.concatenate([for_viz(obs), for_viz(pred)], axis=-2)}
        mask = self.unpatchify(mask.unsqueeze(-1).repeat(1, 1, self._patch_size ** 2 * 3))
        obs = obs.float()
        return {"samples": np.concatenate([for_viz(obs), for_viz(obs * (1 - mask)), for_viz(obs * (1 - mask) + pred * mask)], axis=-2)}


class MAE(AutogradUpdate, Base):
    def __init__(self, ocr_config, env_config) -> None:
        self._module = MAE_Module(ocr_config, env_config)
        super().__init__(ocr_config, env_config)
        # the reference builds weight-decay parameter groups from learning.weight_decay and then hands AdamW the plain parameter list, so
        # torch's default weight decay applies to every parameter; kept as it runs
        self._opt = torch.optim.AdamW(self._module.parameters(), lr=ocr_config.learning.lr, betas=(0.9, 0.95))
