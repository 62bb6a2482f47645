"""Restatement of DQN's noisy linear layers, from the text of include/ocrl_hip_noisy.h: the layout of `factors`, the draw (the counter
RNG's bits from tests/gpu_util.py, then Box-Muller and f = copysign(sqrt|g|, g) in fp64), and `perturb` / `grad` in torch fp32 on the CPU:
every value of those two is a product and a sum of fp32 numbers, each rounded once, which fp32 torch arithmetic on the CPU reproduces to
the bit (no fused multiply-add is formed between separate torch operations).

Hand-counted layout (test_noisy_cpu.py): layers (6, 8), (8, 4), (4, 15), (4, 5) take blocks of 8, 8 | 8, 4 | 4, 16 | 4, 8 floats = 60."""
import numpy as np
import torch

from . import gpu_util as G

SITE_NOISY = 440
MAX_LAYERS, MAX_WIDTH = 10, 65536


def up4(n):
    return (n + 3) & ~3


def layout(layers):
    """([(f_in offset, f_out offset)] per layer, total floats) of `factors` for layers = (in, out) per layer"""
    offs, n = [], 0
    for i, o in layers:
        offs.append((n, n + up4(i)))
        n += up4(i) + up4(o)
    return offs, n


def bits(seed, draw, layer, side, n):
    """the two 32-bit words of elements 0 .. n - 1 of `side` (0 in, 1 out) of `layer` of draw `draw`: the word at the counter
    ((draw mod 2^32) << 32) | (layer << 28) | (side << 27) | i of site 440.  The high word enters the key (csrc/common.h rng_key), the low
    word is the counter: gpu_util.rng_bits4 for draw 0, and its body with the key of the draw otherwise."""
    low = (layer << 28) | (side << 27) | np.arange(n, dtype=np.uint64)
    hi = draw & G._M32
    if hi == 0:
        return G.rng_bits4(seed, SITE_NOISY, low)
    key = G.rng_key(seed, SITE_NOISY, hi)
    k2 = np.uint64((key * 0x9E3779B9 + 0x7F4A7C15) & G._M32)
    c = low ^ np.uint64(key)
    return G._mix32k(c, k2), (G._mix32k(c ^ np.uint64(0x68E31DA4), k2) + np.uint64(key)) & np.uint64(G._M32)


def u01_24(w):
    """csrc/common.h u01_24: fp32((w >> 8) + 0.5) / 2^24, the sum rounded to fp32; returned as fp64 (the value is exact)"""
    return ((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)).astype(np.float64) / 16777216.0


def gaussians(seed, draw, layer, side, n):
    """g of the header in fp64 (the constant 6.2831853 as the fp32 number the kernel multiplies by)"""
    x, y = bits(seed, draw, layer, side, n)
    u0, u1 = u01_24(x), u01_24(y)
    return np.sqrt(-2.0 * np.log(u0)) * np.cos(np.float64(np.float32(6.2831853)) * u1)


def f_of(g):
    g = np.asarray(g, dtype=np.float64)
    return np.copysign(np.sqrt(np.abs(g)), g)


def factors(layers, seed, draw, eps=None):
    """`factors` of a draw as an fp64 array in the header's layout, padding 0; `eps` (same layout) replaces g"""
    offs, n = layout(layers)
    out = np.zeros(n, dtype=np.float64)
    for l, ((i, o), (a, b)) in enumerate(zip(layers, offs)):
        for side, (start, m) in enumerate(((a, i), (b, o))):
            g = gaussians(seed, draw, l, side, m) if eps is None else np.asarray(eps, dtype=np.float64)[start:start + m]
            out[start:start + m] = f_of(g)
    return out


def split(layers, fac):
    """[(f_in [in], f_out [out])] per layer of a `factors` tensor"""
    offs, _ = layout(layers)
    return [(fac[a:a + i], fac[b:b + o]) for (i, o), (a, b) in zip(layers, offs)]


def perturb(layers, mu, sigma, fac):
    """w_eff of the header in fp32 on the CPU: mu / sigma = [weight, bias] per layer, fac the fp32 `factors`"""
    out = []
    for l, (fi, fo) in enumerate(split(layers, fac.float().cpu())):
        p = fo.unsqueeze(1) * fi.unsqueeze(0)
        out += [mu[2 * l].float().cpu() + sigma[2 * l].float().cpu() * p, mu[2 * l + 1].float().cpu() + sigma[2 * l + 1].float().cpu() * fo]
    return out


def grad(layers, dw, fac):
    """dsigma of the header in fp32 on the CPU"""
    out = []
    for l, (fi, fo) in enumerate(split(layers, fac.float().cpu())):
        p = fo.unsqueeze(1) * fi.unsqueeze(0)
        out += [dw[2 * l].float().cpu() * p, dw[2 * l + 1].float().cpu() * fo]
    return out


def make_layers(layers, seed=0, sigma_scale=1.0):
    """(mu, sigma) lists of random fp32 tensors for `layers`: sigma random too, of both signs"""
    g = torch.Generator().manual_seed(seed)
    mu, sigma = [], []
    for i, o in layers:
        mu += [(torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5, (torch.rand(o, generator=g) * 2 - 1) * 0.5]
        sigma += [torch.randn(o, i, generator=g) * sigma_scale / i ** 0.5, torch.randn(o, generator=g) * sigma_scale / i ** 0.5]
    return mu, sigma
