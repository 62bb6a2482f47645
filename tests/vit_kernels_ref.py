"""fp64 torch references of the pooling-Transformer and masked-autoencoder kernels (csrc/pool.hip, pool_long.hip, mae.hip through
include/ocrl_hip_vit_kernels.h), one function per entry point, with the named inputs and the case tables tests/test_gpu_vit_kernels.py
iterates.  Every reference takes a `dtype` where its formula holds a soft-max, an exp or an erf, so that the same code gives the fp32
floor tests/test_vit_kernels_ref_cpu.py measures.  The keep masks are arguments: the GPU test reads them from ocrl_tp_dropout_mask at the
entry's (seed, site), the CPU test from the host restatement of the counter RNG (tests/gpu_util.py)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.gpu_util import dropout_keep

F64 = torch.float64
SEED_LO, SEED_HI = 0x1234567, (0x9ABCDEF << 32) + 0x1357          # below and above 2^32
SITE = 300


def gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def rel(a, b):
    """max |a - b| / max |b| in fp64 (an exactly zero b: the absolute error)"""
    a, b = a.detach().double(), b.detach().double()
    den = b.abs().max().item() if b.numel() else 0.0
    d = (a - b).abs().max().item() if b.numel() else 0.0
    return d / den if den else d


def host_keep(seed, site, p, n):
    """the keep decisions (1 / 0, fp64) of the first n elements of a dropout site"""
    return torch.from_numpy(dropout_keep(seed, site, p, np.arange(n)).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------- attention (short and flash)
# (B, S, d, h, p, seed): every head size 8 / 16 / 32 / 64 at S in {1, 2, 7, 31, 32} (h S <= 256: one trip of the pair loop), dropout at
# three of them; h S = 272 (a second trip); the shape exactly at the 160 KiB backward limit
POOL_ATTN_CASES = [(3, S, 64, h, p, seed) for h in (8, 4, 2, 1) for S, p, seed in
                   ((1, 0.0, 0), (2, 0.0, 0), (7, 0.0, 0), (7, 0.1, SEED_LO), (31, 0.0, 0), (31, 0.5, SEED_HI), (32, 0.0, 0), (32, 0.1, SEED_HI))]
POOL_ATTN_CASES += [(3, 17, 128, 16, 0.0, 0), (3, 17, 128, 16, 0.1, SEED_LO), (3, 32, 256, 4, 0.0, 0), (3, 32, 256, 4, 0.5, SEED_LO),
                    (1, 32, 256, 4, 0.1, SEED_HI)]
FLASH_S = (1, 7, 8, 9, 31, 32, 33, 40, 127, 128, 129, 257)
# (B, S, d, h, p, seed, kind)
FLASH_CASES = [(2, S, 3 * hd, 3, 0.0, 0, "randn") for hd in (16, 32, 48, 64) for S in FLASH_S]
FLASH_CASES += [(2, S, hd, 1, 0.0, 0, "randn") for hd in (16, 32, 48, 64) for S in (1, 9, 129)]
FLASH_CASES += [(2, S, 3 * hd, 3, p, seed, "randn") for hd in (16, 32, 48, 64) for S in (9, 33, 129) for p, seed in ((0.1, SEED_LO), (0.5, SEED_HI))]
FLASH_CASES += [(2, 40, 3 * hd, 3, 0.0, 0, "wide") for hd in (16, 32, 48, 64)]
WIDE_KEY = 5                                                      # the key whose logit is -1e6 for every query


def attn_inputs(B, S, d, h, kind="randn"):
    """qkv [B S, 3 d], dO [B S, d] (fp32).  "wide": the scaled scores span +-50 and key WIDE_KEY (mod S) has a logit of about -1e6 in every row"""
    g = gen(11, B, S, d, h, len(kind))
    qkv, dO = randn(g, B * S, 3 * d), randn(g, B * S, d)
    if kind == "wide":
        hd = d // h
        x = qkv.reshape(B, S, 3, h, hd)
        s = torch.einsum("bihe,bjhe->bhij", x[:, :, 0].double(), x[:, :, 1].double()) / math.sqrt(hd)
        x[:, :, 0] *= 50.0 / s.abs().max().item()
        x[:, :, 0, :, 0] = 8.0                                    # q_0 k_0 / sqrt(hd) = -1e6 at the planted key, 0 elsewhere: q_0 is of
        x[:, :, 1, :, 0] = 0.0                                    # the size of q's other channels, so that dk = dS^T q stays sharp in all
        x[:, WIDE_KEY % S, 1, :, 0] = -125000.0 * math.sqrt(hd)
        qkv = x.reshape(B * S, 3 * d).contiguous()
    return qkv, dO


def attention(qkv, B, S, d, h, keep=None, p=0.0, dO=None, dtype=F64, scale=None, head_perm=None):
    """soft-max attention of h heads over all S keys, dropout on the weights; with dO its gradient.  `scale` and `head_perm` exist for the
    wrong restatements of the CPU file"""
    hd = d // h
    sc = hd ** -0.5 if scale is None else scale
    x = qkv.to(dtype).reshape(B, S, 3, h, hd)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))     # [B, h, S, hd]
    if head_perm is not None:
        k = k[:, head_perm]
    s = (q * sc) @ k.transpose(-1, -2)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    kp = torch.ones_like(P) if keep is None else keep.to(dtype).reshape(B, h, S, S) / (1.0 - p)
    Pd = P * kp
    O = Pd @ v
    out = dict(P=P, lse=lse.reshape(B * h, S), O=O.transpose(1, 2).reshape(B * S, d), s=s)
    if dO is not None:
        g = dO.to(dtype).reshape(B, S, h, hd).transpose(1, 2)
        dP = (g @ v.transpose(-1, -2)) * kp
        Dd = (g * O).sum(-1)
        dS = P * (dP - Dd[..., None])
        if S == 1:                                                # the soft-max of one score is the constant 1: dS is exactly zero
            dS = torch.zeros_like(dS)
        f = lambda t: t.transpose(1, 2).reshape(B * S, d)
        out["zero_scale"] = (dP.abs().max() * torch.maximum(q.abs().max(), k.abs().max()) * sc).item()     # what a zero dq / dk cancels from
        out.update(Dd=Dd.reshape(B * h, S), dq=f(dS @ k * sc), dk=f(dS.transpose(-1, -2) @ (q * sc)), dv=f(Pd.transpose(-1, -2) @ g))
    return out


# ---------------------------------------------------------------------------------------------------------------- CLS-row attention
CLS_DH = ((64, 1), (64, 2), (128, 8), (192, 3), (192, 6), (256, 4), (256, 16))
CLS_S = (1, 2, 63, 64, 65, 129, 300)
# (B, S, d, h, p, seed, kind, chunks)
CLS_CHUNKS = {1: 1, 2: 1, 63: 1, 64: 1, 65: 2, 129: 3, 300: 5}
# dropout (p = 0.1) where every head has enough keys to keep and drop: S = 63, 65, 300 (tests/test_vit_kernels_ref_cpu.py asserts it per case)
CLS_CASES = [(2, S, d, h, (0.1 if S in (63, 65, 300) else 0.0), (SEED_HI if S == 65 else SEED_LO), "randn", CLS_CHUNKS[S]) for d, h in CLS_DH for S in CLS_S]
CLS_CASES += [(1, S, d, h, (0.1 if S == 129 else 0.0), SEED_LO, "randn", CLS_CHUNKS[S]) for d, h in ((64, 1), (256, 16)) for S in CLS_S]
CLS_CASES += [(1024, 130, 64, 2, 0.0, 0, "randn", 1), (2, 129, 128, 8, 0.0, 0, "wide", 3)]


def cls_inputs(B, S, d, h, kind="randn"):
    """X [B, S, d], Win [3 d, d], bin [3 d], q [B, d] = row 0 through the in-projection (fp32 rounded), dO [B, d]"""
    g = gen(13, B, S, d, h, len(kind))
    X, Win, bin_, dO = randn(g, B, S, d), randn(g, 3 * d, d) / math.sqrt(d), randn(g, 3 * d) * 0.5, randn(g, B, d)
    if kind == "wide":
        hd = d // h
        q = X[:, 0].double() @ Win[:d].double().t() + bin_[:d].double()
        U = torch.einsum("bhe,hec->bhc", q.reshape(B, h, hd), Win[d:2 * d].double().reshape(h, hd, d)) / math.sqrt(hd)
        s = torch.einsum("bsc,bhc->bhs", X.double(), U)
        Win[:d] *= 50.0 / s.abs().max().item()
        bin_[:d] *= 50.0 / s.abs().max().item()
    q = (X[:, 0].double() @ Win[:d].double().t() + bin_[:d].double()).float()
    return X, Win, bin_, q, dO


def cls_keep_index(B, S, h):
    """flat element of the attention site that key j of image-head bh uses: bh S S + j (the row of query 0)"""
    return (torch.arange(B * h).reshape(B, h, 1) * S * S + torch.arange(S).reshape(1, 1, S)).reshape(-1)


def cls_attn(X, Win, bin_, q, B, S, d, h, keep=None, p=0.0, dO=None, dtype=F64, bv_term=True):
    """keep [B, h, S] (or None).  bv_term = False drops b_v sum p' (a wrong restatement for the CPU file)"""
    hd, sc = d // h, (d // h) ** -0.5
    X, Win, bin_, q = (t.to(dtype) for t in (X, Win, bin_, q))
    Wk, Wv, bv = Win[d:2 * d].reshape(h, hd, d), Win[2 * d:].reshape(h, hd, d), bin_[2 * d:].reshape(h, hd)
    U = torch.einsum("bhe,hec->bhc", q.reshape(B, h, hd), Wk) * sc
    s = torch.einsum("bsc,bhc->bhs", X, U)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    kp = torch.ones_like(P) if keep is None else keep.to(dtype).reshape(B, h, S) / (1.0 - p)
    Pd = P * kp
    z, a = torch.einsum("bhs,bsc->bhc", Pd, X), Pd.sum(-1)
    o = torch.einsum("hec,bhc->bhe", Wv, z) + (bv * a[..., None] if bv_term else 0.0)
    out = dict(U=U, z=z, stat=torch.stack([a, lse], -1), o=o.reshape(B, d), s=s)
    if dO is not None:
        g = dO.to(dtype).reshape(B, h, hd)
        G, gb = torch.einsum("hec,bhe->bhc", Wv, g), (bv * g).sum(-1)
        D = (z * G).sum(-1) + a * gb
        t = torch.einsum("bsc,bhc->bhs", X, G)
        ds = P * ((t + gb[..., None]) * kp - D[..., None])
        if S == 1:                                                # one key: D = (t + gb) kp exactly, so ds, w and dq are exactly zero
            ds = torch.zeros_like(ds)
        out["zero_scale_w"] = ((t + gb[..., None]).abs().max() * X.abs().max()).item()      # what a zero w / dq cancels from
        out["zero_scale_dq"] = out["zero_scale_w"] * Wk.abs().sum(-1).max().item() * sc
        dX = torch.einsum("bhs,bhc->bsc", ds, U) + torch.einsum("bhs,bhc->bsc", Pd, G)
        w = torch.einsum("bhs,bsc->bhc", ds, X)
        dq = (torch.einsum("hec,bhc->bhe", Wk, w) * sc).reshape(B, d)
        dW = torch.cat([dq.t() @ X[:, 0], (torch.einsum("bhe,bhc->hec", q.reshape(B, h, hd), w) * sc).reshape(d, d),
                        torch.einsum("bhe,bhc->hec", g, z).reshape(d, d)])
        db = torch.cat([dq.sum(0), torch.zeros(d, dtype=dtype), (g * a[..., None]).sum(0).reshape(d)])
        out.update(G=G, gD=torch.stack([gb, D], -1), dX=dX, w=w, dq=dq, dW=dW, db=db)
    return out


def cls_nchunk(B, S):
    """pool_cls_nchunk: (chunks per image, rows per chunk)"""
    cd = lambda a, b: -(-a // b)
    want = max(1, min(cd(1024, B), cd(S, 64)))
    c = cd(cd(S, want), 64) * 64
    return cd(S, c), c


def ln_chunks(R):
    """mae_ln_chunks: (chunks, rows per chunk)"""
    n = min(256, (R + 7) // 8)
    rpc = -(-R // n)
    return -(-R // rpc), rpc


def pool_attn_lds(S, d, h):
    """(forward, backward) LDS bytes of pool_attn"""
    return 12 * S * d, 4 * (4 * S * d + 2 * h * S * S)


def pool_short_ok(K, Din, d, h):
    S = K + 1
    return (1 <= K <= 31 and Din >= 4 and Din % 4 == 0 and d in (64, 128, 192, 256) and h >= 1 and d % h == 0 and d // h in (8, 16, 32, 64)
            and max(pool_attn_lds(S, d, h)) <= 160 * 1024)


# ---------------------------------------------------------------------------------------------------------------- data movement
def pool_embed(lin, cls, pos):
    B, K, d = lin.shape
    x0 = torch.cat([cls.reshape(1, 1, d).expand(B, 1, d), lin], 1)
    return x0 if pos is None else x0 + pos


def pool_rows(x, K, mode):
    if mode == 0:
        return x[:, 1:].reshape(-1, x.shape[-1])
    if mode == 1:
        out = torch.zeros(x.shape[0], K + 1, x.shape[1], dtype=x.dtype)
        out[:, 0] = x
        return out
    return x[:, 0]


def pool_cols(src, ncols, ncopy):
    out = torch.zeros(src.shape[0], ncols, dtype=src.dtype)
    out[:, :ncopy] = src[:, :ncopy]
    return out


def cls_drop_index(B, N, S):
    return (torch.arange(B).reshape(B, 1) * S * N + torch.arange(N).reshape(1, N)).reshape(-1)


# (S, p): the vector kernel (p % 4 == 0) and the scalar one
GATHER_CASES = ((16, 4), (24, 8), (12, 2), (12, 6))


def patchify(imgs, p):
    """models_mae.py patchify: [B, 3, S, S] -> [B, L, p p 3] in (ph, pw, c) order"""
    B, _, S, _ = imgs.shape
    G = S // p
    return torch.einsum("nchpwq->nhwpqc", imgs.reshape(B, 3, G, p, G, p)).reshape(B, G * G, p * p * 3)


def patch_gather(obs, ids, n, p, order="cpq"):
    """rows of the patch-embedding product in the Conv2d weight's (c, ph, pw) order; order = "pqc" is the wrong restatement"""
    B, _, S, _ = obs.shape
    G = S // p
    x = torch.einsum("nchpwq->nhw" + order, obs.reshape(B, 3, G, p, G, p)).reshape(B, G * G, 3 * p * p)
    idx = torch.arange(n).expand(B, n) if ids is None else ids.long()
    return x.gather(1, idx[..., None].expand(B, n, 3 * p * p)).reshape(B * n, 3 * p * p)


def tokens_fwd(embed, cls, pos, ids):
    B, n, D = embed.shape
    idx = torch.arange(n).expand(B, n) if ids is None else ids.long()
    return torch.cat([(cls + pos[0]).reshape(1, 1, D).expand(B, 1, D), embed + pos[1 + idx]], 1)


def unshuffle_fwd(e, mtok, dpos, restore):
    """models_mae.py forward_decoder: mask tokens appended, gathered back through ids_restore, the CLS row in front, plus the position table"""
    B, n1, D = e.shape
    L = restore.shape[1]
    x_ = torch.cat([e[:, 1:], mtok.reshape(1, 1, D).expand(B, L + 1 - n1, D)], 1)
    x_ = x_.gather(1, restore.long()[..., None].expand(B, L, D))
    return torch.cat([e[:, :1], x_], 1) + dpos


def mae_ids(B, L, len_keep, seed=0):
    """(restore [B, L], keep [B, len_keep], mask [B, L]) of a noise draw, as argsort(argsort(noise)) gives them"""
    noise = torch.rand(B, L, generator=gen(17, B, L, len_keep, seed))
    shuffle = noise.argsort(dim=1, stable=True)
    restore = shuffle.argsort(dim=1, stable=True)
    mask = (restore >= len_keep).float()
    return restore.int(), shuffle[:, :len_keep].int(), mask


# ---------------------------------------------------------------------------------------------------------------- GELU, LayerNorm, loss
def gelu_inputs(n4):
    """arguments over [-12, 12] with +-0, the tails and the neighbourhood of 0"""
    n = 4 * n4
    x = torch.linspace(-12.0, 12.0, n)
    special = torch.tensor([0.0, -0.0, 12.0, -12.0, 1e-8, -1e-8, 5.5, -5.5, 8.0, -8.0, 0.5, -0.5])[:n]
    x[torch.randperm(n, generator=gen(19, n4))[:special.numel()]] = special
    return x, randn(gen(23, n4), n)


def gelu(x, dtype=F64):
    x = x.to(dtype)
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_grad(x, dy, dtype=F64):
    x = x.to(dtype)
    return dy.to(dtype) * (0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


LN_F = (4, 32, 252, 256, 260, 768, 1024)
LN_R = (1, 3, 4, 5, 7, 8, 9, 17)
# (kind, F): the hard rows, each at both eps and 5 rows: a row of mean 100, a constant row, rows of spread 1e-3 (where eps decides)
LN_HARD = [(kind, F_) for kind in ("offset", "const", "small") for F_ in (32, 252, 260, 1024)]
LN_EPS = (1e-6, 1e-5)


def ln_inputs(R, F_, kind="randn"):
    """x, gamma, beta, dy, resid.  "offset": row 0 has mean 100 and spread 1; "const": row 0 is constant; "small": every row has spread
    1e-3, so that eps (1e-6 or 1e-5 against a variance of 1e-6) decides the output"""
    g = gen(29, R, F_, len(kind))
    x = randn(g, R, F_)
    if kind == "offset":
        x[0] = 100.0 + randn(g, F_)
    if kind == "const":
        x[0] = 3.25
    if kind == "small":
        x = x * 1e-3
    return x, 1.0 + 0.5 * randn(g, F_), randn(g, F_), randn(g, R, F_), randn(g, R, F_)


def layernorm(x, gam, beta, eps, dtype=F64):
    x, gam, beta = x.to(dtype), gam.to(dtype), beta.to(dtype)
    mean = x.mean(-1)
    rstd = (x.var(-1, unbiased=False) + eps).rsqrt()
    return dict(y=(x - mean[:, None]) * rstd[:, None] * gam + beta, mean=mean, rstd=rstd)


def layernorm_bwd(dy, x, gam, eps, resid=None, dtype=F64):
    dy, x, gam = dy.to(dtype), x.to(dtype), gam.to(dtype)
    f = layernorm(x, gam, torch.zeros_like(gam), eps, dtype)
    xh = (x - f["mean"][:, None]) * f["rstd"][:, None]
    a = dy * gam
    dx = f["rstd"][:, None] * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    return dict(dx=dx if resid is None else dx + resid.to(dtype), dg=(dy * xh).sum(0), db=dy.sum(0))


LOSS_CASES = ((12, 2), (16, 4), (24, 8), (64, 16))              # 3 p p = 12, 48, 192 (< 256) and 768 (> 512)


def mae_loss(pred, obs, mask, p, dloss=None):
    """models_mae.py forward_loss (norm_pix_loss off) and its gradient [B, L + 1, P] with zero CLS rows"""
    pred, mask = pred.double(), mask.double()
    tgt = patchify(obs.double(), p)
    diff = pred - tgt
    loss = (diff.pow(2).mean(-1) * mask).sum() / mask.sum()
    out = dict(loss=loss)
    if dloss is not None:
        g = float(dloss) * 2.0 * diff * mask[..., None] / (diff.shape[-1] * mask.sum())
        out["dpred"] = torch.cat([torch.zeros_like(g[:, :1]), g], 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- fp32 floors
def floor_cases():
    """(key, {output: (fp64, fp32)}) of every reference that holds a soft-max, an exp or an erf, at the inputs the GPU file uses; p = 0
    (dropout multiplies by a constant and moves no floor)"""
    for B, S, d, h, p, seed in POOL_ATTN_CASES:
        if p == 0.0:
            qkv, dO = attn_inputs(B, S, d, h)
            hi, lo = (attention(qkv, B, S, d, h, dO=dO, dtype=t) for t in (F64, torch.float32))
            yield ("pool_attn", S, d, h, "randn"), {n: (hi[n], lo[n]) for n in ("P", "O", "dq", "dk", "dv") if S > 1 or n not in ("dq", "dk")}
    for B, S, d, h, p, seed, kind in FLASH_CASES:
        if p == 0.0:
            qkv, dO = attn_inputs(B, S, d, h, kind)
            hi, lo = (attention(qkv, B, S, d, h, dO=dO, dtype=t) for t in (F64, torch.float32))
            yield ("flash", S, d, h, kind), {n: (hi[n], lo[n]) for n in ("O", "lse", "Dd", "dq", "dk", "dv") if S > 1 or n not in ("dq", "dk")}
    for B, S, d, h, p, seed, kind, _ in CLS_CASES:
        i = cls_inputs(B, S, d, h, kind)
        hi, lo = (cls_attn(*i[:4], B, S, d, h, dO=i[4], dtype=t) for t in (F64, torch.float32))
        yield ("cls", B, S, d, h, kind), {n: (hi[n], lo[n]) for n in ("U", "z", "stat", "o", "G", "gD", "dX", "w", "dq", "dW", "db") if S > 1 or n not in ("w", "dq")}
    for kind, F_ in LN_HARD:
        x, gam, beta, dy, resid = ln_inputs(5, F_, kind)
        for eps in LN_EPS:
            hi, lo = ({**layernorm(x, gam, beta, eps, t), **layernorm_bwd(dy, x, gam, eps, resid, t)} for t in (F64, torch.float32))
            yield ("ln", kind, F_, eps), {n: (hi[n], lo[n]) for n in ("y", "mean", "rstd", "dx", "dg", "db")}
    x, dy = gelu_inputs(257)
    yield ("gelu",), {"y": (gelu(x), gelu(x, torch.float32)), "dpre": (gelu_grad(x, dy), gelu_grad(x, dy, torch.float32))}
