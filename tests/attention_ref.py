"""Plain reference of the causal self-attention core (csrc/attention.hip, include/ocrl_hip.h ocrl_attention_fwd / _bwd) and the
inputs and cases the kernel tests run, chosen here so that the CPU suite can prove them non-vacuous (tests/test_attention_ref_cpu.py)
before the GPU suite (tests/test_gpu_attention_edges.py) uses them.

  o = (dropout(softmax(mask(q k^T / sqrt(dh))))) v,   dropout(P) = P * keep / (1 - p),   lse = logsumexp of the masked scores.

Dropout index contract (csrc/common.h attn_drop_ld): the keep decision of (image b, head, query q, key) is element
((b*h + head)*T + q)*T4 + key of the site's counter-RNG stream, T4 = T rounded up to a multiple of 4."""
import numpy as np
import torch

from tests.gpu_util import drop_thresh, dropout_keep


def keep_mask(seed, site, p, B, h, T):
    """bool [B,h,T,T]: the keep decisions of a self-attention dropout site, from the host restatement of the counter RNG"""
    T4 = (T + 3) & ~3
    m = dropout_keep(seed, site, p, np.arange(B * h * T * T4, dtype=np.uint64)).reshape(B, h, T, T4)
    return torch.from_numpy(np.ascontiguousarray(m[..., :T]))


def attention_ref(q, k, v, h, dO=None, keep=None, p=0.0, dtype=torch.float64):
    """q, k, v [B,T,d] (heads side by side, q unscaled); keep: bool [B,h,T,T] or None; returns o [B,T,d], lse [B,h,T] and, for a given
    dO [B,T,d], dq, dk, dv by autograd -- all evaluated in `dtype`"""
    B, T, d = q.shape
    dh = d // h
    x = [t.detach().to(dtype).clone().requires_grad_(dO is not None) for t in (q, k, v)]
    Q, K, V = (t.view(B, T, h, dh).transpose(1, 2) for t in x)
    S = (Q * dh ** -0.5) @ K.transpose(-1, -2)
    S = S.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    lse = torch.logsumexp(S, -1)
    Pm = torch.softmax(S, -1)
    if keep is not None:
        Pm = Pm * keep.to(dtype) * (1.0 / (1.0 - float(np.float32(p))))
    o = (Pm @ V).transpose(1, 2).reshape(B, T, d)
    out = dict(o=o.detach(), lse=lse.detach())
    if dO is not None:
        o.backward(dO.to(dtype))
        out.update(dq=x[0].grad, dk=x[1].grad, dv=x[2].grad)
    return out


def attention_rows(q, k, v, h, dO, keep, p):
    """the same operation as an explicit loop over (image, head, query) with a hand-written backward, fp64 (tiny shapes only)"""
    B, T, d = q.shape
    dh = d // h
    q, k, v, dO = (t.double() for t in (q, k, v, dO))
    sc, dsc = dh ** -0.5, 1.0 / (1.0 - float(np.float32(p)))
    o, lse = torch.zeros(B, T, d, dtype=torch.float64), torch.zeros(B, h, T, dtype=torch.float64)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for b in range(B):
        for hd in range(h):
            c = slice(hd * dh, (hd + 1) * dh)
            for t in range(T):
                Kt, Vt = k[b, :t + 1, c], v[b, :t + 1, c]
                s = Kt @ q[b, t, c] * sc
                e = torch.exp(s - s.max())
                pr = e / e.sum()
                lse[b, hd, t] = s.max() + torch.log(e.sum())
                w = keep[b, hd, t, :t + 1].double() * dsc if keep is not None else torch.ones(t + 1, dtype=torch.float64)
                o[b, t, c] = (pr * w) @ Vt
                dp = (Vt @ dO[b, t, c]) * w                    # d loss / d P (through the dropout)
                ds = pr * (dp - (pr * dp).sum())
                dq[b, t, c] += ds @ Kt * sc
                dk[b, :t + 1, c] += ds[:, None] * q[b, t, c][None, :] * sc
                dv[b, :t + 1, c] += (pr * w)[:, None] * dO[b, t, c][None, :]
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def make_inputs(B, T, h, dh, seed=0):
    """q, k, v, dO [B,T,d] fp32, standard normal, from a seed that depends on the shape"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + dh + 131 * B + 17 * h)
    d = h * dh
    return tuple(torch.randn(B, T, d, generator=g) for _ in range(4))


PLANT_KEY, PLANT_LOGIT = 1, -1.0e6


def make_wide_range_inputs(B, T, h, dh, seed=0):
    """Scores that span about +-60 (q and k scaled by 15**0.5: the score of a pair is then ~ 15 N(0,1), and the extremes of T*T/2 draws
    sit near 4 sigma), and one very large negative logit planted in every row that has more than one key: dimension 0 of each head is
    1 in every query and 0 in every key except key PLANT_KEY, where it is PLANT_LOGIT * sqrt(dh), so that score is PLANT_LOGIT + O(60).
    (Key 0 is not used: row 0 would then consist of that logit alone, P = 1 exactly, and dq of row 0 would be the rounding residue of
    dP - delta times 1e6 -- the conditioning of the formula, not a property of any implementation.)"""
    q, k, v, dO = make_inputs(B, T, h, dh, seed + 50)
    s = 15.0 ** 0.5
    q, k = q * s, k * s
    q.view(B, T, h, dh)[..., 0] = 1.0
    k.view(B, T, h, dh)[..., 0] = 0.0
    if T > PLANT_KEY:
        k.view(B, T, h, dh)[:, PLANT_KEY, :, 0] = PLANT_LOGIT * dh ** 0.5
    return q, k, v, dO


# ---- the cases of tests/test_gpu_attention_edges.py
LAYOUTS = ("packed", "dense", "padded")       # ld = 3d in one qkv tensor; three dense tensors, ld = d; one tensor with ld = 3d + 8
SEED_LO, SEED_HI = 20240611, (5 << 32) + 977  # below and above 2^32 (the high word of rng_key)
SITE_BLK, SITE_POOL = 16, 300 + 8 * 1 + 2     # SITE_BLK_BASE; the site ocrl_pool_transformer_dropout_mask(layer 1, which 2) dumps

# lengths at p = 0: (B, T, h, dh); every T at dh = 48, the tile seams 1 / 65 / 129 at every other width
LENGTHS = (1, 3, 9, 25, 63, 64, 65, 67, 127, 128, 129, 193, 260)
LENGTH_CASES = [(2, T, 3, 48) for T in LENGTHS] + [(3 if dh == 16 else 2, T, 4 if dh == 16 else 2, dh) for dh in (16, 32, 64) for T in (1, 65, 129)]

# dropout: (B, T, h, dh, p, seed, site)
DROPOUT_CASES = [
    (3, 16, 4, 16, 0.1, SEED_LO, SITE_BLK), (2, 16, 2, 64, 0.5, SEED_HI, SITE_POOL),
    (2, 64, 2, 32, 0.1, SEED_HI, SITE_POOL), (2, 64, 3, 48, 0.5, SEED_LO, SITE_BLK),
    (2, 68, 3, 48, 0.1, SEED_HI, SITE_BLK), (3, 68, 4, 16, 0.5, SEED_LO, SITE_POOL),
    (2, 132, 2, 64, 0.1, SEED_LO, SITE_POOL), (2, 132, 2, 32, 0.5, SEED_HI, SITE_BLK),
    (2, 200, 3, 48, 0.1, SEED_HI, SITE_POOL), (1, 200, 4, 16, 0.5, SEED_LO, SITE_BLK),
]
# dropout at T % 4 != 0: rows of the mask start on no group boundary of the dense index
ODD_DROPOUT_CASES = [(2, 9, 3, 48, 0.1, SEED_LO, SITE_POOL), (2, 25, 2, 32, 0.1, SEED_HI, SITE_BLK), (2, 67, 2, 64, 0.1, SEED_LO, SITE_BLK)]
# strides: every layout with and without dropout at one ragged two-tile shape
STRIDE_CASES = [(2, 67, 2, 32, p, SEED_HI, SITE_BLK) for p in (0.0, 0.1)]
REPRO_CASES = [(2, 132, 3, 48, 0.1, SEED_LO, SITE_BLK), (3, 129, 3, 48, 0.0, 0, 0)]


def all_dropout_cases():
    return [c for c in DROPOUT_CASES + ODD_DROPOUT_CASES + STRIDE_CASES + REPRO_CASES if c[4] > 0]


def non_vacuity(keep, p):
    """(every (image, head) triangle holds kept and dropped entries, dropped share of the in-triangle entries, its distance from
    round(p * 65536) / 65536 in binomial standard deviations)"""
    B, h, T, _ = keep.shape
    tri = torch.tril(torch.ones(T, T, dtype=torch.bool))
    inside = keep[:, :, tri]                                   # [B, h, T (T + 1) / 2]
    both = bool(((inside.sum(-1) > 0) & ((~inside).sum(-1) > 0)).all())
    n, pt = inside.numel(), drop_thresh(p) / 65536.0
    share = float((~inside).sum()) / n
    return both, share, abs(share - pt) / (pt * (1 - pt) / n) ** 0.5
