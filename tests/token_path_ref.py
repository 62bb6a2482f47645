"""fp64 torch references of the SLATE token-path and helper kernels (csrc/elementwise.hip through include/ocrl_hip_slate_kernels.h), one
plain function per entry, written from each operation's definition (the header's comment, oracle/slate_oracle.py for the Gumbel soft-max
and the embedding), and the named inputs the CPU suite (tests/test_token_path_ref_cpu.py) proves usable before the GPU suite
(tests/test_gpu_token_path_kernels.py) runs them.  The soft-max family takes a `dtype`, so that the same formulas can be evaluated in
fp32: what that loses against fp64 is the floor the GPU bars rest on (FLOOR_CASES)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import slate_oracle as O

TINY = O.TINY
F64 = torch.float64


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def f32(x):
    """the value an entry receives for a `float` argument"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------- soft-max family
def gumbel_softmax(raw, e1, e2, tau, dtype=F64):
    """oracle.gumbel_softmax on log_softmax(raw) for the soft sample (z, and its straight-through form zst) and the hard token: the
    first argmax of logp + g2.  s1 / s2 are the two compared scores."""
    raw, e1, e2 = (t.to(dtype) for t in (raw, e1, e2))
    tau = f32(tau)
    lp = torch.log_softmax(raw, -1)
    z = O.gumbel_softmax(lp, e1, tau, False, -1)
    zst = O.gumbel_softmax(lp, e1, tau, True, -1)
    s1, s2 = lp - (e1 + TINY).log(), lp - (e2 + TINY).log()
    return dict(z=z, zst=zst, tokens=s2.argmax(-1), s1=s1, s2=s2)


GUMBEL_STD = {"well": 1.0, "peaked": 8.0}


@functools.lru_cache(maxsize=None)
def gumbel_inputs(kind, R, V):
    """raw [R, V] ~ N(0, std^2), e1 / e2 ~ Exp(1), fp32"""
    g = _gen(11, R, V, GUMBEL_STD[kind] * 10)
    raw = torch.randn(R, V, generator=g) * GUMBEL_STD[kind]
    e1, e2 = (torch.empty(R, V).exponential_(generator=g) for _ in range(2))
    return raw, e1, e2


TIE_PAIRS = {"thread": (37, 37 + 256), "waves": (100, 200)}       # columns v and v + 256 belong to one thread; 100 and 200 to waves 1 and 3


@functools.lru_cache(maxsize=None)
def gumbel_tie_inputs(where, V):
    """two columns with the same logit and the same noise that are the maximum of both scores, in every one of 3 rows"""
    raw, e1, e2 = (t.clone() for t in gumbel_inputs("well", 3, V))
    a, b = TIE_PAIRS[where]
    for t, v in ((raw, 9.0), (e1, 1e-3), (e2, 2e-3)):
        t[:, a] = v
        t[:, b] = v
    return raw, e1, e2


def softmax_bwd_rows(z, d, scale, dtype=F64):
    z, d = z.to(dtype), d.to(dtype)
    return z * (d - (z * d).sum(-1, keepdim=True)) * f32(scale)


@functools.lru_cache(maxsize=None)
def softmax_bwd_inputs(R, V):
    g = _gen(12, R, V)
    return torch.softmax(torch.randn(R, V, generator=g).double() * 2, -1).float(), torch.randn(R, V, generator=g)


STAT_V = {1: 64, 4: 250, 6: 320, 64: 4096}            # columns per segment count: a ragged last segment at 4, a wholly empty one at 6


def segment_stats(scores, nseg):
    """[R, V] -> per 64-column segment (max, sum exp(x - max)) in fp64, (-inf, 0) for an empty segment, and the segment's first argmax"""
    R, V = scores.shape
    x = torch.full((R, nseg * 64), -math.inf, dtype=F64)
    x[:, :V] = scores.double()
    x = x.view(R, nseg, 64)
    m, idx = x.max(-1)
    s = torch.where(m > -math.inf, (x - torch.where(m > -math.inf, m, torch.zeros_like(m))[..., None]).exp().sum(-1), torch.zeros_like(m))
    return m, s, idx + 64 * torch.arange(nseg)


@functools.lru_cache(maxsize=None)
def stat_inputs(nseg, R):
    """scores, hard scores and pred ~ N(0, 3^2) / N(0, 1) fp32; stat = the fp64 segment statistics rounded to fp32; hstat / hidx = the
    hard scores' segment maxima (fp32, exact) and their columns (0 for an empty segment); tok ~ U[0, V); pred with 8 padding columns"""
    V = STAT_V[nseg]
    g = _gen(13, nseg, R)
    scores, hard = torch.randn(R, V, generator=g) * 3, torch.randn(R, V, generator=g) * 3
    m, s, _ = segment_stats(scores, nseg)
    hm, _, hidx = segment_stats(hard, nseg)
    hidx = torch.where(hm > -math.inf, hidx, torch.zeros_like(hidx))
    tok = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    pred = torch.randn(R, V, generator=g)
    return dict(V=V, scores=scores, hard=hard, stat=torch.stack((m, s), -1).float(), hstat=hm.float(), hidx=hidx.int(), tok=tok, pred=pred)


def stat_combine(scores, pred, tok, scale, dtype=F64):
    """lse [R] and scale * sum(lse - pred[row, tok[row]])"""
    lse = torch.logsumexp(scores.to(dtype), -1)
    picked = pred.to(dtype).gather(1, tok.long()[:, None])[:, 0]
    return lse, ((lse - picked).sum() * f32(scale)).reshape(1)


def stat_tie(nseg, R):
    """hstat / hidx of R rows in which two segments hold the same maximum, the row's greatest; returns them with the column that must win"""
    g = _gen(14, nseg, R)
    hm = torch.randn(R, nseg, generator=g)
    hidx = (torch.randint(0, 64, (R, nseg), generator=g) + 64 * torch.arange(nseg)).int()
    want = torch.zeros(R, dtype=torch.int64)
    for r in range(R):
        a, b = sorted(torch.randperm(nseg, generator=g)[:2].tolist())
        hm[r, a] = hm[r, b] = 7.5
        want[r] = hidx[r, a]
    return hm, hidx, want


def exp_rows(y, lse, dtype=F64):
    return (y.to(dtype) - lse.to(dtype)[:, None]).exp()


@functools.lru_cache(maxsize=None)
def exp_rows_inputs(R, V):
    y = torch.randn(R, V, generator=_gen(15, R, V)) * 3
    return y, torch.logsumexp(y.double(), -1).float()


def decode_attn(qkv, t, d, h, dtype=F64):
    """row t of the causal soft-max attention of qkv [B, T, ld] = (q | k | v | padding): out [B, d]"""
    B = qkv.shape[0]
    dh = d // h
    x = qkv[:, :t + 1, :3 * d].to(dtype)
    q, k, v = (x[..., i * d:(i + 1) * d].reshape(B, t + 1, h, dh).transpose(1, 2) for i in range(3))        # [B, h, t + 1, dh]
    s = (q[:, :, t:t + 1] * dh ** -0.5) @ k.transpose(-1, -2)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, d)


DECODE_CASES = [(2, 16, 192, 4, 576), (1, 300, 192, 4, 576), (2, 20, 64, 1, 200), (1, 8, 32, 8, 96)]        # (B, T, d, h, ld)


def decode_ts(case):
    T = case[1]
    return [0, T - 1] + ([256] if T == 300 else [])


@functools.lru_cache(maxsize=None)
def decode_inputs(case):
    B, T, d, h, ld = case
    return torch.randn(B, T, ld, generator=_gen(16, *case))


# the cases of the soft-max family: key -> (fp64 outputs, fp32 outputs) of the same formulas; the GPU test's bars come from these
GUMBEL_CASES = [(kind, R, V, tau) for kind in ("well", "peaked") for V in (256, 768, 2048, 4096) for R in (1, 5) for tau in (1.0, 0.1)]
SOFTMAX_BWD_CASES = [(3, 256), (3, 768), (3, 4096)]
STAT_CASES = [(nseg, R) for nseg in (1, 4, 6, 64) for R in (1, 16, 17, 33)]
EXP_ROWS_CASES = [(3, 4), (7, 768)]
CE_SCALE, BWD_SCALE = 0.37, 0.37


def floor_cases():
    """yields (key, {output: (fp64, fp32)})"""
    for c in GUMBEL_CASES:
        kind, R, V, tau = c
        hi, lo = (gumbel_softmax(*gumbel_inputs(kind, R, V), tau, dtype=dt) for dt in (F64, torch.float32))
        yield ("gumbel",) + c, {n: (hi[n], lo[n]) for n in ("z", "zst")}
    for c in SOFTMAX_BWD_CASES:
        z, d = softmax_bwd_inputs(*c)
        yield ("softmax_bwd",) + c, {"d": tuple(softmax_bwd_rows(z, d, BWD_SCALE, dtype=dt) for dt in (F64, torch.float32))}
    for c in STAT_CASES:
        i = stat_inputs(*c)
        hi, lo = (stat_combine(i["scores"], i["pred"], i["tok"], CE_SCALE, dtype=dt) for dt in (F64, torch.float32))
        yield ("stat",) + c, {"lse": (hi[0], lo[0]), "ce": (hi[1], lo[1])}
    for c in EXP_ROWS_CASES:
        y, lse = exp_rows_inputs(*c)
        yield ("exp_rows",) + c, {"z": tuple(exp_rows(y, lse, dtype=dt) for dt in (F64, torch.float32))}
    for c in DECODE_CASES:
        for t in decode_ts(c):
            yield ("decode", c, t), {"out": tuple(decode_attn(decode_inputs(c), t, c[2], c[3], dtype=dt) for dt in (F64, torch.float32))}


def rel(a, b):
    """max |a - b| / max |b|"""
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-300)


def top_two_gap(score):
    """per row: the greatest value minus the second greatest"""
    t = score.double().topk(2, -1).values
    return t[:, 0] - t[:, 1]


# ------------------------------------------------------------------------------------------------------------------- everything else
def rowdot_bias64(g, act, bias):
    return (g.double() * (act.double() - bias.double())).sum(-1)


def embed_fwd(tokens, dic, bos, pe):
    """[B, T, d]: row 0 the BOS parameter, row t > 0 the dictionary row of token (b, t - 1), plus the positional table"""
    B, T = tokens.shape
    emb = dic.double()[tokens[:, :T - 1].long()]
    return torch.cat((bos.double().reshape(1, 1, -1).expand(B, 1, -1), emb), 1) + pe.double()[None, :T]


def embed_bwd(g, tokens, V):
    """ddict [V, d]: the rows (b, t > 0) of g added to the dictionary row of token (b, t - 1)"""
    B, T, d = g.shape
    return torch.zeros(V, d, dtype=F64).index_add_(0, tokens[:, :T - 1].reshape(-1).long(), g.double()[:, 1:].reshape(-1, d))


def embed_step(tokens, dic, bos, pe, t):
    B = tokens.shape[0]
    src = bos.double().reshape(1, -1).expand(B, -1) if t == 0 else dic.double()[tokens[:, t - 1].long()]
    return src + pe.double()[t]


@functools.lru_cache(maxsize=None)
def embed_inputs(B, T, V, d, tokens="random"):
    """tokens [B, T] int32 ("random", "const3" = all 3, "image" = image b holds b), dict [V, d], bos [d], pe [T, d], g [B, T, d]"""
    g = _gen(17, B, T, V, d)
    if tokens == "random":
        tok = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    elif tokens == "const3":
        tok = torch.full((B, T), 3, dtype=torch.int32)
    else:
        tok = torch.arange(B, dtype=torch.int32)[:, None].expand(B, T).contiguous()
    return tok, torch.randn(V, d, generator=g), torch.randn(d, generator=g), torch.randn(T, d, generator=g), torch.randn(B, T, d, generator=g)


def colsum(X, F_, out0, accumulate, scale):
    s = X.double()[:, :F_].sum(0) * f32(scale)
    return s + out0.double() if accumulate else s


def mse(obs, recon):
    """obs [B, C, H, W], recon [B, H, W, 4] -> (sum (recon - obs)^2 / B as [1], drecon [B, H, W, 4] with zero channels >= C)"""
    B, C = obs.shape[:2]
    e = recon.double()[..., :C] - obs.double().permute(0, 2, 3, 1)
    return (e ** 2).sum().reshape(1) / B, F.pad(2 * e / B, (0, 4 - C))


def pixel_shuffle(x):
    """NHWC [B, h, w, 4 C] -> [B, 2h, 2w, C]"""
    return F.pixel_shuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


def pixel_unshuffle(x, mask=None):
    """NHWC [B, 2h, 2w, C] -> [B, h, w, 4 C], times (mask > 0)"""
    y = F.pixel_unshuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    return y if mask is None else torch.where(mask > 0, y, torch.zeros_like(y))


def nchw_to_nhwc8(x):
    return F.pad(x.permute(0, 2, 3, 1), (0, 8 - x.shape[1])).contiguous()


def patchify4(x):
    B, C, S, _ = x.shape
    return F.unfold(x, 4, stride=4).transpose(1, 2).reshape(B * (S // 4) ** 2, C * 16).contiguous()


def pad_cols(x, C, Cout):
    """[R, >= C] -> [R, Cout]: the first C columns, zeros beyond"""
    return F.pad(x[:, :C], (0, Cout - C)) if Cout >= C else x[:, :Cout].clone()


def im2col5(x8, C, ldc):
    """x8 [B, H, W, 8] -> [B H W, ldc], column tap * C + c = the 5x5 window (zero outside the image), zero columns from 25 C on"""
    B, H, W, _ = x8.shape
    u = F.unfold(x8[..., :C].permute(0, 3, 1, 2), 5, padding=2).view(B, C, 25, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 25 * C)
    return F.pad(u, (0, ldc - 25 * C)).contiguous()


def unpack5(dWp, C):
    return dWp[:, :25 * C].reshape(64, 25, C).permute(0, 2, 1).reshape(64, C, 5, 5).contiguous()


def posgrid(S, dtype=torch.float32):
    """[S * S, 4] = (north, south, west, east) ramps, each step one correctly rounded operation of `dtype`"""
    r = torch.arange(S, dtype=dtype) / max(S - 1, 1) if S > 1 else torch.zeros(1, dtype=dtype)
    south, east = r[:, None].expand(S, S), r[None, :].expand(S, S)
    return torch.stack((1 - south, south, 1 - east, east), -1).reshape(S * S, 4).contiguous()


def posmap(Wpos, bpos, S, dtype=F64):
    """[S, S, C]: the position grid through the Linear(4, C), summed north, south, west, east, bias"""
    g = posgrid(S).to(dtype)
    W = Wpos.to(dtype)
    out = g[:, 0:1] * W[None, :, 0]
    for j in (1, 2, 3):
        out = out + g[:, j:j + 1] * W[None, :, j]
    return (out + bpos.to(dtype)).reshape(S, S, -1)


def onehot(tokens, V):
    return F.one_hot(tokens.long(), V).float()


def slot_init(mu, logsig, eps):
    return mu.double() + logsig.double().exp() * eps.double()


def slot_init_bwd(d, logsig, eps):
    return d.double().sum(0), (d.double() * eps.double()).sum(0) * logsig.double().exp()


def argmax_pos(pred, B, T, t, dense_rows):
    """[B]: the first argmax of image b's logits at position t"""
    rows = pred if dense_rows else pred.view(B, T, -1)[:, t]
    return rows.argmax(-1)
