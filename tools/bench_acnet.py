"""Actor-critic head and PPO minibatch step (ocrl_acnet_fwd, ocrl_acnet_ppo_fwd_bwd): configs/sb3_acnet/mlp.yaml on F = 128 features,
4 actions.  The forward at B = 4 (a rollout step at num_envs = 4) and B = 32; the PPO step at B = 32 (configs/sb3/ppo.yaml batch_size)
and B = 2048.

Each is timed through the C ABI and as an eager torch module doing the same arithmetic on the same GPU (nn.Linear layers, log_softmax,
the PPO loss and autograd's backward).  ms per call = the median over `--calls` (>= 200) individually timed calls after warm-up, each
between two events on the stream; the launch counts are the kernels rocprofv3 --kernel-trace sees (run the tool under it; `--only`
selects one case so that the trace holds nothing else):

    rocprofv3 --kernel-trace --stats -- python tools/bench_acnet.py --only fwd4 --calls 200
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import _lib  # noqa: E402
from tests import acnet_ref as R  # noqa: E402

F, A = 128, 4
DIMS, ACTS = ((64, 64), (64,), (64,)), ((1, 1), (2,), (2,))
HIP_LAUNCHES = {"fwd": 1, "ppo": 3}                   # acnet_fwd; acnet_adv_stats + acnet_ppo + acnet_reduce


def median_ms(f, calls, warm=20):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


class TorchNet(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.w = nn.ParameterList([nn.Parameter(t.clone()) for t in w])

    def forward(self, x):
        return R.forward(x, list(self.w), DIMS, ACTS)[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--only", default="", help="fwd4 | fwd32 | ppo32 | ppo2048 | torch (the eager torch cases alone)")
    a = ap.parse_args()
    L, p = _lib.lib(), _lib.ptr
    gen = torch.Generator().manual_seed(0)
    w = [(torch.randn(s, generator=gen) * (1.4 / s[-1] ** 0.5 if len(s) == 2 else 0.05)).cuda() for s in R.param_shapes(F, A, DIMS)]
    dw = [torch.empty_like(t) for t in w]
    tnet = TorchNet(w).cuda()
    st = _lib.stream()
    out = {}
    for B in (4, 32, 2048):
        x = torch.randn(B, F, generator=gen).cuda()
        d = _lib.acnet_desc(B, F, A, DIMS, ACTS)
        n = L.ocrl_acnet_ws_floats(ctypes.byref(d))
        ws, lg, vl = torch.empty(n, device="cuda"), torch.empty(B, A, device="cuda"), torch.empty(B, device="cuda")
        act = torch.randint(0, A, (B,), generator=gen).cuda()
        old, adv, ret = (torch.randn(B, generator=gen).cuda() * s for s in (0.1, 1.0, 1.0))
        old = old - 1.4
        scal, dx = torch.empty(6, device="cuda"), torch.empty_like(x)

        def hip_fwd():
            _lib.check(L.ocrl_acnet_fwd(ctypes.byref(d), p(x), _lib.ptrs(w), None, None, p(lg), p(vl), 0, None, 0, st))

        def hip_ppo():
            _lib.check(L.ocrl_acnet_ppo_fwd_bwd(ctypes.byref(d), p(x), _lib.ptrs(w), p(act), p(old), p(adv), p(ret), 0.2, 0.5, 0.0, 1, p(scal), p(dx),
                                                _lib.ptrs(dw), p(ws), n, st))

        def torch_fwd():
            with torch.no_grad():
                tnet(x)

        xg = x.clone().requires_grad_(True)

        def torch_ppo():
            tnet.zero_grad(set_to_none=True)
            xg.grad = None
            lgt, vlt = tnet(xg)
            R.ppo(lgt, vlt, act, old, adv, ret, 0.2, 0.5, 0.0, True)["loss"].backward()

        for tag, hip, ref in ((f"fwd{B}", hip_fwd, torch_fwd), (f"ppo{B}", hip_ppo, torch_ppo)):
            if tag in ("fwd2048", "ppo4"):
                continue
            if a.only in ("", tag):
                out[tag] = dict(hip_ms=round(median_ms(hip, a.calls), 5), hip_launches=HIP_LAUNCHES[tag[:3]])
            if a.only in ("", "torch", "torch_" + tag):
                out.setdefault(tag, {})["torch_ms"] = round(median_ms(ref, a.calls), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
