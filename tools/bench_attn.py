"""attention micro-benchmark through the C ABI (development aid): the forward, and the three forms of the backward side by side --
two-kernel (OCRL_ATTN_BWD=2), one-pass (1) and hand-off (3, ocrl_attention_bwd_ws) with dS workspaces for the whole batch and for
chunks of CHUNKS images (default 32,16).  P: dropout probability (default 0.1)."""
import ctypes, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import _lib
L = _lib.lib()
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
B, T, d, h = 128, 1024, 192, 4
p = float(os.environ.get("P", "0.1"))
chunks = [B] + [int(c) for c in os.environ.get("CHUNKS", "32,16").split(",") if c]
qkv = torch.randn(B, T, 3 * d, device="cuda")
q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
o = torch.empty(B, T, d, device="cuda"); lse = torch.empty(B, h, T, device="cuda")
dO = torch.randn(B, T, d, device="cuda"); dqkv = torch.empty_like(qkv); delta = torch.empty(B, h, T, device="cuda")
ds = torch.empty(L.ocrl_attention_bwd_ds_floats(B, T, h), device="cuda")
per_image = L.ocrl_attention_bwd_ds_floats(1, T, h)
def fwd(): _lib.check(L.ocrl_attention_fwd(P(q), P(k), P(v), P(o), P(lse), B, T, d, h, 3 * d, p, 1, 16, None))
def bwd(): _lib.check(L.ocrl_attention_bwd(P(q), P(k), P(v), P(o), P(lse), P(dO), P(dqkv[..., :d]), P(dqkv[..., d:2*d]), P(dqkv[..., 2*d:]), P(delta), B, T, d, h, 3 * d, p, 1, 16, None))
def bwd_ws(images):
    return lambda: _lib.check(L.ocrl_attention_bwd_ws(P(q), P(k), P(v), P(o), P(lse), P(dO), P(dqkv[..., :d]), P(dqkv[..., d:2*d]), P(dqkv[..., 2*d:]), P(delta),
                                                      B, T, d, h, 3 * d, p, 1, 16, P(ds), images * per_image, None))
def t(f, n=10):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
def form(flag, f, name, products):
    os.environ["OCRL_ATTN_BWD"] = flag
    ms = t(f)
    # executed products: one is B h 136 tiles of 64 x 64 x dh at T = 1024 (diagonal tiles whole); the rate is over the causal flops
    print(f"attn bwd {name} B{B} T{T} p={p}: {ms:.3f} ms {products / 2 * fl / ms / 1e9:.1f} TFLOP/s ({products} products)")
    return dqkv.clone()
fl = 4.0 * B * h * T * T * (d // h) / 2       # causal: half of 2 matmuls x 2 flop
ms = t(fwd); print(f"attn fwd B{B} T{T} p={p}: {ms:.3f} ms {fl/ms/1e9:.1f} TFLOP/s (causal flops)")
two = form("2", bwd, "two-kernel", 7)
one = form("1", bwd, "one-pass", 5)
for c in chunks:
    hand = form("3", bwd_ws(c), f"hand-off, dS chunks of {c} images ({c * per_image * 4 / 1e6:.0f} MB)", 5)
    print(f"    dk|dv bitwise equal to two-kernel: {torch.equal(hand[..., d:], two[..., d:])}; dq bitwise equal: {torch.equal(hand[..., :d], two[..., :d])}; "
          f"max |dq - dq two-kernel| = {(hand[..., :d] - two[..., :d]).abs().max().item():.3e}")
