"""Relation Network pooling head (ocrl_pool_rn_fwd/_bwd): the default config (configs/pooling/rn.yaml: g_dims 4 x 256,
f_dims 256-128-64-64) over SLATE's 6 x 192 slots.  B = 16 (a rollout) and 256 / 2048 (PPO minibatches).

Runs: eval forward; train forward + backward with d slots (encoder fine-tuned through the head) and without (frozen encoder).  Each is
timed through the C ABI and for a torch-on-GPU restatement of the same head (nn.Linear layers over the pair rows, built with an
index_select gather; autograd for the backward).  The rate is the algorithmic count of the factored form over the time:
forward 4 K D g1 + 2 P sum g_{l-1} g_l + 2 sum f_{l-1} f_l per image (P = K (K-1) pairs), training 3x that.  B = 16 is launch-bound:
its rate measures launch overhead, not the matrix pipe."""
import ctypes
import itertools
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import _lib  # noqa: E402

PEAK = 157.3e12                       # fp32 MFMA, MI355X
K, D = 6, 192
G, F = [256, 256, 256, 256], [256, 128, 64, 64]
L = _lib.lib()
p = _lib.ptr


def timed(f, n=30):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def flops_per_image():
    P = K * (K - 1)
    fw = 4 * K * D * G[0] + 2 * P * sum(a * b for a, b in zip(G, G[1:])) + 2 * sum(a * b for a, b in zip([G[-1]] + F, F))
    return fw


class TorchRN(nn.Module):
    """the same head in torch: pair rows by index_select, nn.Linear + ReLU on every pair row, sum, nn.Linear + ReLU"""

    def __init__(self, ws):
        super().__init__()
        lins = []
        for i in range(0, len(ws), 2):
            lin = nn.Linear(ws[i].shape[1], ws[i].shape[0])
            lin.weight.data.copy_(ws[i])
            lin.bias.data.copy_(ws[i + 1])
            lins.append(lin)
        self.g = nn.ModuleList(lins[:len(G)])
        self.f = nn.ModuleList(lins[len(G):])
        pairs = list(itertools.permutations(range(K), 2))
        self.register_buffer("I", torch.tensor([i for i, _ in pairs]))
        self.register_buffer("J", torch.tensor([j for _, j in pairs]))

    def forward(self, s):
        x = torch.cat([s.index_select(1, self.I), s.index_select(1, self.J)], dim=-1)
        for lin in self.g:
            x = torch.relu(lin(x))
        x = x.sum(1)
        for lin in self.f:
            x = torch.relu(lin(x))
        return x


def main():
    torch.manual_seed(0)
    from types import SimpleNamespace
    from ocrl_amd.poolings import RN_Module
    mod = RN_Module(D, K, 1, SimpleNamespace(g_dims=G, f_dims=F))
    w = [t.detach().cuda().contiguous() for t in mod._param_list()]
    g = [torch.empty_like(t) for t in w]
    arr = (ctypes.c_void_p * len(w))(*[t.data_ptr() for t in w])
    garr = (ctypes.c_void_p * len(g))(*[t.data_ptr() for t in g])
    gd, fd = (ctypes.c_int * len(G))(*G), (ctypes.c_int * len(F))(*F)
    ref = TorchRN(w).cuda()
    fw = flops_per_image()
    print(f"RN default (K={K}, D={D}, g={G}, f={F}): {fw / 1e6:.2f} MFLOP per image forward, {3 * fw / 1e6:.2f} train")
    for B in (16, 256, 2048):
        x = torch.randn(B, K, D, device="cuda")
        dc = torch.randn(B, F[-1], device="cuda")
        out = torch.empty(B, F[-1], device="cuda")
        dx = torch.empty_like(x)
        n = L.ocrl_pool_rn_ws_floats(B, K, D, len(G), gd, len(F), fd)
        ws = torch.empty(n, device="cuda")

        def fwd():
            _lib.check(L.ocrl_pool_rn_fwd(p(x), arr, p(out), B, K, D, len(G), gd, len(F), fd, p(ws), n, None))

        def trn(dsl):
            fwd()
            _lib.check(L.ocrl_pool_rn_bwd(p(x), p(dc), arr, p(dsl), garr, B, K, D, len(G), gd, len(F), fd, p(ws), n, None))

        xr = x.clone().requires_grad_(True)

        def t_fwd():
            with torch.no_grad():
                ref(x)

        def t_trn(need_dx):
            ref.zero_grad(set_to_none=True)
            y = ref(xr if need_dx else x)
            y.backward(dc)

        with torch.no_grad():
            fwd()
            err = ((out - ref(x)).abs().max() / ref(x).abs().max()).item()
        rows = [("eval forward", timed(fwd), timed(t_fwd), fw),
                ("train fwd+bwd, dslots", timed(lambda: trn(dx)), timed(lambda: t_trn(True)), 3 * fw),
                ("train fwd+bwd, detached", timed(lambda: trn(None)), timed(lambda: t_trn(False)), 3 * fw)]
        regime = " (launch-bound)" if B <= 16 else ""
        for name, ms, ms_t, fl in rows:
            rate = B * fl / (ms * 1e-3)
            print(f"RN B{B}{regime} {name}: ABI {ms:.3f} ms ({rate / 1e12:.1f} TFLOP/s, {rate / PEAK:.2f} of peak); "
                  f"torch {ms_t:.3f} ms ({B * fl / (ms_t * 1e-3) / 1e12:.1f} TFLOP/s); ABI/torch {ms / ms_t:.2f}")
        print(f"RN B{B}: workspace {n * 4 / 2**20:.0f} MiB; ABI vs torch output rel diff {err:.1e}; train floor at peak "
              f"{B * 3 * fw / PEAK * 1e3:.3f} ms")


if __name__ == "__main__":
    main()
