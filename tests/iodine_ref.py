"""fp64 torch references of the IODINE kernels and the broadcast decoder's own kernels (include/ocrl_hip_iodine.h), one per entry point,
for tests/test_gpu_iodine_kernels.py and tests/test_iodine_ref_cpu.py.  Where oracle/iodine_oracle.py has the operation (elbo_terms,
encoding, layernorm3, coords) it is called in the given dtype and not restated; the rest is a torch forward with autograd for the backward.
Tensors are in torch's layouts (NCHW, [B, K, ...]); to_out4 / enc_nhwc and friends convert to the kernels'.  `dtype` is float64 for a
reference and float32 where the CPU suite measures what the same formulas lose in the kernels' precision."""
import math

import torch
import torch.nn.functional as F

from oracle import iodine_oracle as IO

F64 = torch.float64
ENC_GROUPS = (("0-8", slice(0, 9)), ("9-11", slice(9, 12)), ("12", slice(12, 13)), ("13", slice(13, 14)), ("14", slice(14, 15)),
              ("15-16", slice(15, 17)))


# ---------------------------------------------------------------------------------------------------------------- ELBO inputs
# name -> std of the mask logits.  "well": the project's kernel bar applies to every output; "spread" and "saturated": see the table of
# floors in tests/test_gpu_iodine_kernels.py
INPUT_SETS = {"well": 1.0, "spread": 4.0, "saturated": 8.0}


def elbo_inputs(kind, K, S, B, seed=0):
    """fp32 (obs [B,3,S,S] in [0,1], recons [B,K,3,S,S] in [-0.3,1.3], mask_logits [B,K,1,S,S] ~ N(0, std^2), denc [B,K,17,S,S] ~ N(0,1))"""
    g = torch.Generator().manual_seed(1000 * seed + 100 * K + S + B)
    obs = torch.rand(B, 3, S, S, generator=g)
    recons = torch.rand(B, K, 3, S, S, generator=g) * 1.6 - 0.3
    logits = torch.randn(B, K, 1, S, S, generator=g) * INPUT_SETS[kind]
    denc = torch.randn(B, K, 17, S, S, generator=g)
    return obs, recons, logits, denc


def to_out4(recons, logits):
    """[B,K,3,S,S], [B,K,1,S,S] -> the kernels' out4 [B,K,S,S,4]"""
    return torch.cat((recons, logits), dim=2).permute(0, 1, 3, 4, 2).contiguous()


def nhwc(x):
    """[B,K,C,S,S] -> [B,K,S,S,C]"""
    return x.permute(0, 1, 3, 4, 2).contiguous()


def _cfg(S, sigma, layer_norm):
    return IO.default_cfg(obs_size=S, sigma=sigma, beta=1.0, layer_norm=layer_norm)


def _terms(obs, recons, logits, cfg):
    B, K = recons.shape[:2]
    z = recons.new_zeros(B, K, 1)                     # a posterior at the prior: kl = 0, elbo = ll
    return IO.elbo_terms(obs, z, z, z, recons, logits, cfg)


def elbo_fwd(obs, recons, logits, sigma, layer_norm, dtype=F64):
    """one iteration's ELBO as io_elbo + io_enc_norm produce it: dict of ll, mse (sums over the batch, as `part` holds them), masks, recon
    and recons_masked (clamped), dout4 [B,K,S,S,4] = d(B elbo)/d(recons, mask logits), enc [B,K,S,S,17], st1 / st2 [B,K,4]"""
    obs = obs.to(dtype)
    recons = recons.to(dtype).clone().requires_grad_(True)
    logits = logits.to(dtype).clone().requires_grad_(True)
    B, K, S = recons.shape[0], recons.shape[1], recons.shape[-1]
    cfg = _cfg(S, sigma, layer_norm)
    t = _terms(obs, recons, logits, cfg)
    g_r, g_k, g_a = torch.autograd.grad(B * t["elbo"], [recons, t["masks"], logits])          # exactly as iodine_forward takes them
    with torch.no_grad():
        enc = IO.encoding(obs, recons, logits, t, g_r, g_k, cfg)
        raw = IO.encoding(obs, recons, logits, t, g_r, g_k, _cfg(S, sigma, False))
        groups = [raw[:, :, 9:12], raw[:, :, 12:13], raw[:, :, 13:14], raw[:, :, 14:15]]
        st1 = torch.stack([v.sum(dim=(2, 3, 4)) for v in groups], dim=-1)
        st2 = torch.stack([((v - v.mean(dim=(2, 3, 4), keepdim=True)) ** 2).sum(dim=(2, 3, 4)) for v in groups], dim=-1)
        return dict(ll=t["pll"].sum(), mse=t["mse"] * B, masks=t["masks"][:, :, 0], recon=t["recon"].clamp(0, 1),
                    recons_masked=t["recons_masked"].clamp(0, 1), dout4=to_out4(g_r, g_a), enc=nhwc(enc), st1=st1, st2=st2)


def elbo_bwd(obs, recons, logits, denc, sigma, cw, dtype=F64):
    """d(cw * sum of pixel log-likelihoods + <enc, denc>) / d(recons, mask logits) as [B,K,S,S,4]; enc is built as in the model, its gradient
    and likelihood inputs detached, so only channels 3-8 carry gradient whatever denc holds (denc None: the likelihood term alone)"""
    obs = obs.to(dtype)
    recons = recons.to(dtype).clone().requires_grad_(True)
    logits = logits.to(dtype).clone().requires_grad_(True)
    B, S = recons.shape[0], recons.shape[-1]
    cfg = _cfg(S, sigma, True)
    t = _terms(obs, recons, logits, cfg)
    total = cw * t["pll"].sum()
    if denc is not None:
        g_r, g_k = torch.autograd.grad(B * t["elbo"], [recons, t["masks"]], retain_graph=True)
        enc = IO.encoding(obs, recons, logits, t, g_r.detach(), g_k.detach(), cfg)
        total = total + (enc * denc.to(dtype)).sum()
    d_r, d_a = torch.autograd.grad(total, [recons, logits])
    return to_out4(d_r, d_a)


def elbo_bwd_analytic(obs, recons, logits, denc, sigma, cw, dtype=F64):
    """the same gradient written out (the formulas of io_elbo_bwd_kernel's header comment), for the self-consistency check"""
    obs, recons, logits = obs.to(dtype), recons.to(dtype), logits.to(dtype)
    m = F.softmax(logits, dim=1)
    d = obs[:, None] - recons
    clp = -d * d / (2 * sigma ** 2) - math.log(sigma) - 0.5 * math.log(2 * math.pi)
    post = F.softmax((m + 1e-12).log() + clp, dim=1)
    dr = cw * post * d / sigma ** 2
    dm = (cw * post / (m + 1e-12)).sum(dim=2, keepdim=True)
    da = torch.zeros_like(logits)
    if denc is not None:
        e = denc.to(dtype)
        dA = e[:, :, 8:9] - F.softmax(clp.sum(dim=2, keepdim=True), dim=1) * e[:, :, 8:9].sum(dim=1, keepdim=True)
        dr = dr + e[:, :, 3:6] + dA * d / sigma ** 2
        dm = dm + e[:, :, 6:7]
        da = e[:, :, 7:8]
    return to_out4(dr, da + m * (dm - (m * dm).sum(dim=1, keepdim=True)))


def _rel(a, b):
    den = b.abs().max().item()
    return (a.double() - b).abs().max().item() / den if den else float((a.double() - b).abs().max().item() != 0)


def elbo_pairs(kind, sigma, case):
    """{layer_norm: (elbo_fwd in fp64, elbo_fwd in fp32)} at an input set: one evaluation of each"""
    K, S, B = case
    obs, rec, lg, _ = elbo_inputs(kind, K, S, B)
    return {ln: (elbo_fwd(obs, rec, lg, sigma, ln), elbo_fwd(obs, rec, lg, sigma, ln, dtype=torch.float32)) for ln in (True, False)}


def elbo_floors(pairs):
    """what the reference's own formulas lose in fp32, from elbo_pairs: {layer_norm: {group: error of the encoding's channels 9-14}} and
    under the key None the same for the columns of st1 / st2 ("st1:9-11", ...; they do not depend on the layer norm), each relative to
    the fp64 tensor's maximum"""
    out = {ln: {g: _rel(lo["enc"][..., sl], hi["enc"][..., sl]) for g, sl in ENC_GROUPS[1:5]} for ln, (hi, lo) in pairs.items()}
    hi, lo = pairs[True]
    out[None] = {f"{s}:{g}": _rel(lo[s][..., j], hi[s][..., j]) for s in ("st1", "st2") for j, (g, _) in enumerate(ENC_GROUPS[1:5])}
    return out


# ---------------------------------------------------------------------------------------------------------------- posterior
def sample(mu, ls, eps, dtype=F64):
    """(slots, sum of the elementwise KL terms)"""
    mu, ls, eps = mu.to(dtype), ls.to(dtype), eps.to(dtype)
    s = ls.exp()
    return mu + s * eps, (-ls + 0.5 * (s * s + mu * mu) - 0.5).sum()


def latent(mu, ls, eps, ds, beta, layer_norm, dtype=F64):
    """[BK, 4L] = (mu, ls, LN(ds - beta mu), LN(ds sigma eps - beta (sigma^2 - 1))) with the oracle's 3-D layer norm"""
    mu, ls, eps, ds = (v.to(dtype) for v in (mu, ls, eps, ds))
    s = ls.exp()
    ln = (lambda v: IO.layernorm3(v[None])[0]) if layer_norm else (lambda v: v)
    return torch.cat((mu, ls, ln(ds - beta * mu), ln(ds * s * eps - beta * (s * s - 1))), dim=1)


def post_grad(mu, ls, eps, ds, dlat, kw, dtype=F64):
    """(d/dmu, d/dls) of <ds, mu + exp(ls) eps> + kw * KL + <dlat[:, :L], mu> + <dlat[:, L:2L], ls> by autograd (dlat None: without)"""
    mu = mu.to(dtype).clone().requires_grad_(True)
    ls = ls.to(dtype).clone().requires_grad_(True)
    slots, kl = sample(mu, ls, eps, dtype)
    total = (ds.to(dtype) * slots).sum() + kw * kl
    if dlat is not None:
        L = mu.shape[1]
        total = total + (dlat[:, :L].to(dtype) * mu).sum() + (dlat[:, L:2 * L].to(dtype) * ls).sum()
    return torch.autograd.grad(total, [mu, ls])


def post_grad_analytic(mu, ls, eps, ds, dlat, kw, dtype=F64):
    mu, ls, eps, ds = (v.to(dtype) for v in (mu, ls, eps, ds))
    s, L = ls.exp(), mu.shape[1]
    a, b = ds + kw * mu, ds * s * eps + kw * (s * s - 1)
    return (a, b) if dlat is None else (a + dlat[:, :L].to(dtype), b + dlat[:, L:2 * L].to(dtype))


# ---------------------------------------------------------------------------------------------------------------- refinement network
def out_size(h):
    return (h - 1) // 2 + 1


def im2col(x, ldc):
    """x [Bn,Hi,Wi,C] -> col [Bn*Ho*Wo, ldc], column tap*C + c of the stride-2, pad-1 3x3 window, zero padded to ldc; keeps x's dtype
    (a copy: the GPU result must equal it bit for bit)"""
    Bn, Hi, Wi, C = x.shape
    u = F.unfold(x.permute(0, 3, 1, 2), 3, stride=2, padding=1)                                # [Bn, C*9, Ho*Wo], row c*9 + tap
    u = u.reshape(Bn, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)
    return F.pad(u, (0, ldc - 9 * C))


def col2im(dcol, act, shape, dtype=F64):
    """the transpose of im2col by autograd, times elu'(act) taken from the ELU output (act > 0 ? 1 : act + 1); act None: no gate"""
    x = torch.zeros(shape, dtype=dtype, requires_grad=True)
    (dx,) = torch.autograd.grad((im2col(x, dcol.shape[1]) * dcol.to(dtype)).sum(), x)
    if act is not None:
        a = act.to(dtype)
        dx = dx * torch.where(a > 0, torch.ones_like(a), a + 1)
    return dx


def refw_pack(W, ldc):
    """W [64,C,3,3] -> Wp [64, ldc], column tap*C + c"""
    return F.pad(W.permute(0, 2, 3, 1).reshape(W.shape[0], -1), (0, ldc - 9 * W.shape[1]))


def pool(pre, dpool, dtype=F64):
    """pre [BK,n,64] (pre-activation of the last refinement conv) -> (r = elu(pre), mean over n, d pre for the cotangent dpool)"""
    pre = pre.to(dtype).clone().requires_grad_(True)
    r = F.elu(pre)
    p = r.mean(dim=1)
    (dpre,) = torch.autograd.grad((p * dpool.to(dtype)).sum(), pre)
    return r.detach(), p.detach(), dpre


def elu2(a, dy, dtype=F64):
    a = a.to(dtype).clone().requires_grad_(True)
    y = F.elu(F.elu(a))
    (da,) = torch.autograd.grad((y * dy.to(dtype)).sum(), a)
    return y.detach(), da


def lstm(gates, c0, dh1, dc1, dtype=F64):
    """torch's LSTMCell arithmetic (gate order i, f, g, o) -> (acts [rows,4H], c1, h1, dgates, dc0); dh1 / dc1 None = zero"""
    gates = gates.to(dtype).clone().requires_grad_(True)
    c0 = c0.to(dtype).clone().requires_grad_(True)
    gi, gf, gg, go = gates.chunk(4, dim=1)
    acts = torch.cat((torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)), dim=1)
    c1 = torch.sigmoid(gf) * c0 + torch.sigmoid(gi) * torch.tanh(gg)
    h1 = torch.sigmoid(go) * torch.tanh(c1)
    total = gates.sum() * 0
    if dh1 is not None:
        total = total + (h1 * dh1.to(dtype)).sum()
    if dc1 is not None:
        total = total + (c1 * dc1.to(dtype)).sum()
    dgates, dc0 = torch.autograd.grad(total, [gates, c0], allow_unused=True)
    dc0 = torch.zeros_like(c0) if dc0 is None else dc0
    return acts.detach(), c1.detach(), h1.detach(), dgates, dc0


# ---------------------------------------------------------------------------------------------------------------- 64 -> 4 convolution
def act_gate(act, elu):
    """derivative of the saved activation: ReLU' (act > 0) or ELU' (act > 0 ? 1 : act + 1)"""
    one = torch.ones_like(act)
    return torch.where(act > 0, one, act + 1 if elu else torch.zeros_like(act))


def c4(X, W, bias, dY, act, elu, dtype=F64):
    """X [Bn,S,S,64], W [co_n,64,3,3] (zero rows up to 4 outputs), bias [4], dY [Bn,S,S,4], act [Bn,S,S,64] -> (Y [Bn,S,S,4], dX gated by
    the activation's derivative [Bn,S,S,64], dW [4,64,3,3])"""
    X = X.to(dtype).clone().requires_grad_(True)
    W4 = torch.zeros(4, 64, 3, 3, dtype=dtype)
    W4[:W.shape[0]] = W.to(dtype)
    W4.requires_grad_(True)
    Y = F.conv2d(X.permute(0, 3, 1, 2), W4, bias.to(dtype), padding=1).permute(0, 2, 3, 1)
    dX, dW = torch.autograd.grad((Y * dY.to(dtype)).sum(), [X, W4])
    return Y.detach(), dX * act_gate(act.to(dtype), elu), dW


# ---------------------------------------------------------------------------------------------------------------- Slot-Attention mixture
def mix(out4, obs, dtype=F64):
    """out4 [B,K,S,S,4], obs [B,C,S,S] -> (recon [B,S,S,3], loss = sum (obs - recon)^2 / B over obs's C channels, d loss / d out4)"""
    out4 = out4.to(dtype).clone().requires_grad_(True)
    B, C = obs.shape[:2]
    m = F.softmax(out4[..., 3:], dim=1)
    recon = (m * out4[..., :3]).sum(dim=1)
    loss = ((obs.to(dtype).permute(0, 2, 3, 1) - recon[..., :C]) ** 2).sum() / B
    (d,) = torch.autograd.grad(loss, out4)
    return recon.detach(), loss.detach(), d


def compose(W1, Wpos, bpos, dtype=F64):
    """W1 [64,D,5,5], Wpos [D,4], bpos [D] -> (Wc [25,64,5], W1r [25,64,D]) by direct contraction"""
    W1r = W1.to(dtype).reshape(64, -1, 25).permute(2, 0, 1)
    Wc = torch.cat((torch.einsum("tod,dj->toj", W1r, Wpos.to(dtype)), torch.einsum("tod,d->to", W1r, bpos.to(dtype))[..., None]), dim=-1)
    return Wc, W1r.contiguous()


def compose_bwd(W1, Wpos, bpos, dWc, dW1r, dtype=F64):
    """(dW1, dWpos, dbpos) by autograd through compose"""
    leaves = [v.to(dtype).clone().requires_grad_(True) for v in (W1, Wpos, bpos)]
    Wc, W1r = compose(*leaves, dtype=dtype)
    return torch.autograd.grad((Wc * dWc.to(dtype)).sum() + (W1r * dW1r.to(dtype)).sum(), leaves)
