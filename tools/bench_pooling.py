"""Latency of the slot-set pooling head through the C ABI (ocrl_pool_transformer_fwd/_bwd): default reference config
(6 slots x 192 -> d_model 128, 8 heads, ff 2048, 1 layer).  B = rollout batches (num_envs) and a PPO minibatch.

--feature-map: the same head over SLATE's CNN feature map (use_cnn_feat: 64x64 tokens of width 67, S = 4097, pos_emb 'ape') through
ocrl_pool_transformer_long_fwd/_bwd, L = 1 and 2: eval forward at B = 4, train forward + backward at B = 32 (frozen encoder: no dslots).
Besides the time it prints the rate at which the call moves the bytes the built form must move at least (slots read; the token rows
written once and read once in the forward; read again, their gradient written and read back in the backward)."""
import ctypes, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import _lib
from types import SimpleNamespace
from ocrl_amd.poolings.transformer import Transformer_Module
L = _lib.lib()
p = _lib.ptr
cfg = SimpleNamespace(rep_dim=192, num_slots=6, d_model=128, nhead=8, num_layers=1, dim_feedforward=2048, dropout=0.1, pos_emb="None")
torch.manual_seed(0)
w = [t.detach().cuda().contiguous() for t in Transformer_Module(cfg.rep_dim, cfg.num_slots, cfg)._param_list()]; g = [torch.empty_like(t) for t in w]
arr = (ctypes.c_void_p * len(w))(*[t.data_ptr() for t in w]); garr = (ctypes.c_void_p * len(g))(*[t.data_ptr() for t in g])
K, Din, d, h, ff, nl = cfg.num_slots, cfg.rep_dim, cfg.d_model, cfg.nhead, cfg.dim_feedforward, cfg.num_layers
def t(f, n=50):
    for _ in range(5): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
if "--feature-map" in sys.argv:
    S, Din = 4097, 67
    pe = torch.zeros(S, d, device="cuda")
    for nl in (1, 2):
        c = SimpleNamespace(**{**vars(cfg), "rep_dim": Din, "num_slots": S - 1, "num_layers": nl, "pos_emb": "ape"})
        wl = [t.detach().cuda().contiguous() for t in Transformer_Module(Din, S - 1, c)._param_list()]; gl = [torch.empty_like(t) for t in wl]
        arl = (ctypes.c_void_p * len(wl))(*[t.data_ptr() for t in wl]); garl = (ctypes.c_void_p * len(gl))(*[t.data_ptr() for t in gl])
        for B, train in ((4, False), (32, True)):
            x = torch.randn(B, S - 1, Din, device="cuda"); out = torch.empty(B, d, device="cuda"); dc = torch.randn(B, d, device="cuda")
            n = L.ocrl_pool_transformer_long_ws_floats(B, S - 1, Din, d, h, ff, nl); ws = torch.empty(n, device="cuda")
            fwd = lambda pd: _lib.check(L.ocrl_pool_transformer_long_fwd(p(x), arl, p(pe), p(out), B, S - 1, Din, d, h, ff, nl, pd, 7, p(ws), n, None))
            if train:
                f = lambda: (fwd(0.1), _lib.check(L.ocrl_pool_transformer_long_bwd(p(x), p(dc), arl, None, garl, B, S - 1, Din, d, h, ff, nl, 0.1, 7,
                                                                                    p(ws), n, None)))
                rows = 5
            else:
                f = lambda: fwd(0.0)
                rows = 2
            us = t(f, 20)
            nbytes = 4 * (B * (S - 1) * Din * (2 if train else 1) + rows * B * S * d)
            print(f"pooling feature map S{S} L{nl} B{B}: {'train forward+backward' if train else 'eval forward'} {us / 1e3:.3f} ms; "
                  f"{nbytes / 1e6:.1f} MB minimum traffic at {nbytes / us / 1e3:.0f} GB/s; workspace {n * 4 / 2**20:.0f} MiB")
    sys.exit(0)
for B in (4, 16, 32, 256, 2048):
    x = torch.randn(B, K, Din, device="cuda"); out = torch.empty(B, d, device="cuda"); dc = torch.randn(B, d, device="cuda"); dx = torch.empty_like(x)
    n = L.ocrl_pool_transformer_ws_floats(B, K, d, h, ff, nl); ws = torch.empty(n, device="cuda")
    fwd = lambda: _lib.check(L.ocrl_pool_transformer_fwd(p(x), arr, None, p(out), B, K, Din, d, h, ff, nl, 0.0, 0, p(ws), n, None))
    trn = lambda: (_lib.check(L.ocrl_pool_transformer_fwd(p(x), arr, None, p(out), B, K, Din, d, h, ff, nl, 0.1, 7, p(ws), n, None)),
                   _lib.check(L.ocrl_pool_transformer_bwd(p(x), p(dc), arr, None, garr, B, K, Din, d, h, ff, nl, 0.1, 7, p(ws), n, None)))
    print(f"pooling B{B}: eval forward {t(fwd):.1f} us, train forward+backward {t(trn):.1f} us")
