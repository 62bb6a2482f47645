"""Plain reference of the decoder's cross attention to the slots in its two forms (include/ocrl_hip.h: ocrl_xattn_fwd / _bwd, the folded
form of csrc/xattn.hip; ocrl_cross_attn_fwd / _bwd, the plain kernels of csrc/elementwise.hip), and the inputs and cases the kernel tests
run, chosen here so that the CPU suite can prove them non-vacuous (tests/test_cross_attn_ref_cpu.py) before the GPU suite
(tests/test_gpu_cross_attention.py) uses them.

  q = x Wq^T, ck = mem Wk^T, cv = mem Wv^T;  S = (q dh^-1/2) ck^T per head;  P = softmax(S);  Pd = P * keep_p / (1 - p);
  ao = Pd cv per head;  out = ao Wo^T;  y = resid + out * keep_o / (1 - p).

Dropout index contracts: keep_p of (image b, head, token t, slot) is element ((b*h + head)*T + t)*K + slot of site_p's counter-RNG stream
(no rounding of K up to 4), keep_o of (b, t, o) is element (b*T + t)*d + o of site_o's.

Every function takes `wrong`, a set of deliberately wrong restatements (WRONG below).  The CPU suite shows that each of them moves the
output it touches by more than 100 x the tolerance of the GPU test, at the very inputs that test runs: a kernel with one of these
mistakes cannot pass."""
import numpy as np
import torch

from tests.attention_ref import SEED_HI, SEED_LO
from tests.gpu_util import drop_thresh, dropout_keep

SITE_P, SITE_O = 16 + 8 * 1 + 2, 16 + 8 * 1 + 3          # SITE_BLK_BASE + 8 * block + {2 cross.attn, 3 cross.out}, block 1
WRONG = ("head_stride_K", "no_scale", "mask_stride_4", "no_rescale", "sites_swapped", "padded_weight", "heads_permuted")


def kp_of(K, h):
    """slots per head after padding (csrc/xattn.hip: xattn_plan)"""
    return 8 if (K <= 8 and h > 1) else 16


def keep_masks(seed, site_p, site_o, p, B, h, T, K, d, wrong=()):
    """(keep_p bool [B,h,T,K], keep_o bool [B,T,d]) from the host restatement of the counter RNG"""
    if "sites_swapped" in wrong:
        site_p, site_o = site_o, site_p
    Ks = (K + 3) & ~3 if "mask_stride_4" in wrong else K
    kp = dropout_keep(seed, site_p, p, np.arange(B * h * T * Ks, dtype=np.uint64)).reshape(B, h, T, Ks)[..., :K]
    ko = dropout_keep(seed, site_o, p, np.arange(B * T * d, dtype=np.uint64)).reshape(B, T, d)
    return torch.from_numpy(np.ascontiguousarray(kp)), torch.from_numpy(np.ascontiguousarray(ko))


def _dsc(p, wrong=()):
    return 1.0 if "no_rescale" in wrong else 1.0 / (1.0 - float(np.float32(p)))


def _attend(q, ck, cv, h, keep_p, p, wrong, dtype):
    """the attention core on [B,T,d] / [B,K,d] tensors of `dtype`: (S [B,h,T,K], P, Pd, ao [B,T,d])"""
    B, T, d = q.shape
    K, dh = ck.shape[1], d // h
    Q = q.view(B, T, h, dh).transpose(1, 2)
    Kh, Vh = (t.view(B, K, h, dh).transpose(1, 2) for t in (ck, cv))
    S = (Q * (1.0 if "no_scale" in wrong else dh ** -0.5)) @ Kh.transpose(-1, -2)
    if "padded_weight" in wrong:                                  # the padding columns of a head (score 0) take part in the soft-max
        pad = torch.zeros(B, h, T, kp_of(K, h) - K, dtype=dtype)
        P = torch.softmax(torch.cat([S, pad], -1), -1)[..., :K]
    else:
        P = torch.softmax(S, -1)
    Pd = P if keep_p is None else P * keep_p.to(dtype) * _dsc(p, wrong)
    ao = Pd @ Vh                                                  # [B,h,T,dh]
    if "heads_permuted" in wrong:
        ao = ao.roll(1, dims=1)
    return S, P, Pd, ao.transpose(1, 2).reshape(B, T, d)


def core_ref(Q, Km, Vm, h, keep_p=None, p=0.0, dO=None, wrong=(), dtype=torch.float64):
    """the plain kernels' operation: O [B,T,d], P [B,h,T,K] and, for a given dO, dQ, dKm, dVm by autograd, evaluated in `dtype`"""
    x = [t.detach().to(dtype).clone().requires_grad_(dO is not None) for t in (Q, Km, Vm)]
    _, P, _, O = _attend(x[0], x[1], x[2], h, keep_p, p, wrong, dtype)
    out = dict(O=O.detach(), P=P.detach())
    if dO is not None:
        O.backward(dO.to(dtype))
        out.update(dQ=x[0].grad, dKm=x[1].grad, dVm=x[2].grad)
    return out


def fold_ref(ck, cv, Wq, Wo, h, wrong=()):
    """the per-image operands of the folded form in the padded column layout col = head * KP + slot:
    Ab [B,NC,d]: Ab[(h,k), e] = dh^-1/2 sum_j Wq[h dh + j, e] ck[k, h dh + j];   Vo [B,NC,d]: Vo[(h,k), o] = sum_j cv[k, h dh + j] Wo[o, h dh + j].
    Padding columns are zero.  Differentiable; evaluated in the dtype of its arguments."""
    B, K, d = ck.shape
    dh, KP = d // h, kp_of(K, h)
    NC, stride = h * KP, (K if "head_stride_K" in wrong else KP)
    scale = 1.0 if "no_scale" in wrong else dh ** -0.5
    ckh, cvh = (t.view(B, K, h, dh).permute(0, 2, 1, 3) for t in (ck, cv))                    # [B,h,K,dh]
    A = torch.einsum("bhkj,hje->bhke", ckh, Wq.view(h, dh, d)) * scale
    V = torch.einsum("bhkj,ohj->bhko", cvh, Wo.view(d, h, dh))
    cols = (torch.arange(h)[:, None] * stride + torch.arange(K)[None, :]).reshape(-1)
    Ab = torch.zeros(B, NC, d, dtype=ck.dtype).index_copy(1, cols, A.reshape(B, h * K, d))
    Vo = torch.zeros(B, NC, d, dtype=ck.dtype).index_copy(1, cols, V.reshape(B, h * K, d))
    return Ab, Vo


def unfold_cols(t, h, K):
    """[.., NC] in the padded column layout -> [.., h, K] (the real slots)"""
    KP = kp_of(K, h)
    return t.reshape(*t.shape[:-1], h, KP)[..., :K]


def block_ref(x, resid, mem, Wq, Wk, Wv, Wo, h, keep_p=None, keep_o=None, p=0.0, gd=None, wrong=(), dtype=torch.float64, folded=False):
    """the whole attention branch of a decoder block.  gd [B,T,d] is the gradient wrt `out` (the branch's output before the output dropout,
    which is what the kernels take: dy * keep_o / (1 - p)).  Returns y, P, Pd, S, ck, cv, q, ao, out and, for a given gd, dx (through the
    attention branch only), dWq, dWo, dck, dcv, dq, dao, dS -- all in `dtype`.  folded = True evaluates scores and output through fold_ref's
    operands (scores = x Ab^T, out = Pd Vo), the arithmetic of csrc/xattn.hip; in exact arithmetic the two are the same function."""
    B, T, d = x.shape
    K = mem.shape[1]
    grad = gd is not None
    xx, W1, W2, W3, W4 = (t.detach().to(dtype).clone().requires_grad_(grad) for t in (x, Wq, Wk, Wv, Wo))
    m, r = mem.detach().to(dtype), resid.detach().to(dtype)
    ck, cv = m @ W2.t(), m @ W3.t()
    q = xx @ W1.t()
    if folded:
        assert not wrong
        Ab, Vo = fold_ref(ck, cv, W1, W4, h)
        KP = kp_of(K, h)
        S = unfold_cols(xx @ Ab.transpose(1, 2), h, K).permute(0, 2, 1, 3)                    # [B,h,T,K]
        P = torch.softmax(S, -1)
        Pd = P if keep_p is None else P * keep_p.to(dtype) * _dsc(p)
        Pc = torch.cat([Pd.permute(0, 2, 1, 3), torch.zeros(B, T, h, KP - K, dtype=dtype)], -1).reshape(B, T, h * KP)
        ao = None
        out = Pc @ Vo
    else:
        S, P, Pd, ao = _attend(q, ck, cv, h, keep_p, p, wrong, dtype)
        out = ao @ W4.t()
    y = r + (out if keep_o is None else out * keep_o.to(dtype) * _dsc(p, wrong))
    res = dict(y=y.detach(), P=P.detach(), Pd=Pd.detach(), S=S.detach(), ck=ck.detach(), cv=cv.detach(), q=q.detach(), out=out.detach())
    if ao is not None:
        res["ao"] = ao.detach()
    if grad:
        keepg = [t for t in (ck, cv, q, S, ao) if t is not None]
        for t in keepg:
            t.retain_grad()
        out.backward(gd.to(dtype))
        res.update(dx=xx.grad, dWq=W1.grad, dWo=W4.grad, dck=ck.grad, dcv=cv.grad, dq=q.grad, dS=S.grad)
        if ao is not None:
            res["dao"] = ao.grad
    return res


def uniform_out(x, resid, mem, Wq, Wk, Wv, Wo, h):
    """y with every probability 1 / K (what a soft-max that ignores its scores gives), fp64, no dropout"""
    m = mem.double()
    cv = m @ Wv.double().t()
    return resid.double() + (cv.mean(1, keepdim=True) @ Wo.double().t()).expand(-1, x.shape[1], -1)


# ---- inputs
def make_inputs(B, T, K, d, h, seed=0, gain=1.6):
    """x (a LayerNorm output: unit scale), resid, mem, gd fp32 standard normal; the four [d,d] weights N(0, 1/d) so that q, ck, cv are of
    unit scale, with `gain` on Wq: the scores of a head are then ~ gain * N(0,1), a soft-max that is neither uniform nor saturated.
    Returns dict(x, resid, mem, Wq, Wk, Wv, Wo, gd)."""
    g = torch.Generator().manual_seed(100003 * seed + 7 * T + 13 * d + 131 * B + 17 * h + 1009 * K)
    r = lambda *s: torch.randn(*s, generator=g)
    w = lambda: r(d, d) * d ** -0.5
    return dict(x=r(B, T, d), resid=r(B, T, d), mem=r(B, K, d), Wq=w() * gain, Wk=w(), Wv=w(), Wo=w(), gd=r(B, T, d))


def make_wide_range_inputs(B, T, K, d, h, seed=0):
    """scores spanning several tens: gain 15 on Wq gives scores ~ 15 N(0,1), whose extremes over B*h*T*K draws sit near +-50"""
    return make_inputs(B, T, K, d, h, seed + 50, gain=15.0)


def weights_of(inp):
    return inp["x"], inp["resid"], inp["mem"], inp["Wq"], inp["Wk"], inp["Wv"], inp["Wo"]


# ---- the cases of tests/test_gpu_cross_attention.py
D_MODELS = (64, 128, 192, 256)


def legal_heads(d):
    """head counts ocrl_slate_create accepts for d_model d: h | d, (d/h) % 4 == 0, d/h <= 64"""
    return [h for h in range(1, d + 1) if d % h == 0 and (d // h) % 4 == 0 and d // h <= 64]


def folded_heads(d):
    """head counts of `legal_heads` for which some slot count has a folded form: NC = h * KP in {16, 32, 64}"""
    return [h for h in legal_heads(d) if h in (1, 2, 4, 8)]


def slot_classes(h):
    """slot counts of the folded grid for a head count: K in {1, 3, 8} where KP = 8 applies, {9, 16} where KP = 16 applies (h = 8 has no
    folded form above 8 slots), {5, 16} for one head (KP = 16 at every K)"""
    if h == 1:
        return (5, 16)
    return (1, 3, 8) + ((9, 16) if h <= 4 else ())


def _drop_of(K, i):
    """dropout goes wherever K % 4 != 0 (rows of the probability mask then start off the group of four): (p, seed), alternating"""
    if K % 4 == 0:
        return 0.0, 0
    return (0.1, SEED_LO) if i % 2 == 0 else (0.5, SEED_HI)


def _folded_grid():
    cases, i = [], 0
    for d in D_MODELS:
        for h in folded_heads(d):
            for K in slot_classes(h):
                p, seed = _drop_of(K, i)
                cases.append((2, 36, K, d, h, p, seed))
                i += 1
    return cases


# folded: (B, T, K, d, h, p, seed).  The whole instantiation grid at T = 36, B = 2; the token sweep on one instantiation per KP
FOLDED_GRID = _folded_grid()
SWEEP_T = ((2, 1), (2, 15), (2, 16), (2, 17), (2, 36), (1, 200))                   # (B, T); T = 200: 13 tiles, three uneven splits
FOLDED_SWEEP = [(B, T, 3, 192, 4, 0.5 if T == 1 else 0.1, SEED_HI if i % 2 else SEED_LO) for i, (B, T) in enumerate(SWEEP_T)] + \
               [(B, T, 9, 128, 2, 0.5 if i % 2 else 0.0, SEED_LO if i % 2 else 0) for i, (B, T) in enumerate(SWEEP_T)]
# plain: (B, T, K, d, h, p, seed); every (MAXK, d/h), with the head counts the model sends to the plain kernels (16, 8 above 8 slots, 12,
# 6, 3) and 8 and 4 heads for the widths 24 and 48
PLAIN_DH = {4: (64, 16), 8: (64, 8), 16: (192, 12), 24: (192, 8), 32: (192, 6), 48: (192, 4), 64: (192, 3)}
PLAIN_GRID = [(2, 36, K, d, h) + _drop_of(K, i + j) for i, (dh, (d, h)) in enumerate(sorted(PLAIN_DH.items())) for j, K in enumerate((3, 8, 9, 16))]
PLAIN_LONG = [(2, 300, K, d, h) + _drop_of(K, i + j) for i, (dh, (d, h)) in enumerate(sorted(PLAIN_DH.items())) for j, K in enumerate((7, 13))]
PLAIN_SWEEP = [(2, T, K, 192, 4) + _drop_of(K, T) for T in (1, 15, 16, 17) for K in (7, 13)]
# both forms against one block_ref
SHARED = [(2, 36, 3, 192, 4, 0.1, SEED_LO), (2, 17, 9, 128, 2, 0.5, SEED_HI), (1, 200, 5, 64, 1, 0.1, SEED_HI)]
WIDE = [(2, 36, 7, 192, 4), (1, 200, 13, 128, 2)]                                     # (B, T, K, d, h) of the wide-range runs, both forms
REPRO = [(2, 36, 3, 192, 4, 0.1, SEED_LO), (2, 36, 13, 256, 4, 0.5, SEED_HI)]
BATCH_INDEPENDENCE = [(3, 36, 3, 192, 4, 0.1, SEED_LO), (3, 200, 9, 64, 2, 0.0, 0)]
UNSUPPORTED = [(9, 64, 8), (3, 192, 3), (3, 192, 6), (3, 192, 12), (3, 64, 16), (17, 64, 2), (3, 320, 4), (0, 64, 2)]      # (K, d, h)


def all_folded_cases():
    return FOLDED_GRID + FOLDED_SWEEP + SHARED + REPRO + BATCH_INDEPENDENCE


def all_plain_cases():
    return PLAIN_GRID + PLAIN_LONG + PLAIN_SWEEP + SHARED


def non_vacuity(keep, p):
    """(every (image, head) of keep [B,h,..] holds kept and dropped entries, dropped share, its distance from round(p * 65536) / 65536 in
    binomial standard deviations)"""
    flat = keep.reshape(keep.shape[0], keep.shape[1], -1)
    both = bool(((flat.sum(-1) > 0) & ((~flat).sum(-1) > 0)).all())
    n, pt = flat.numel(), drop_thresh(p) / 65536.0
    share = float((~flat).sum()) / n
    return both, share, abs(share - pt) / (pt * (1 - pt) / n) ** 0.5
