"""CNN_Linear pooling head (poolings.CNN_Linear_Module over ocrl_pool_cnn_fwd/_bwd) on SLATE-CNN's token map [B, 4096, 67], against two
baselines on the same GPU, neither of which is the code under test:

  generic   the NatureCNN encoder's kernels (ocrs.NatureCNN_Module over ocrl_naturecnn_fwd/_bwd with obs_channels = 67) on the
            permuted-to-NCHW copy of the tokens, the permute included: the path that existed before the channels-last first layer
            (it returns the weight gradients only)
  torch     the same layers as an fp32 nn.Sequential (TF32 off) on the NCHW view of the tokens

Cases: B in {4, 32, 256}; the forward under no_grad, forward + backward with detached tokens, forward + backward with the token gradient
(no generic column: that path has no input gradient).  The three sides are timed alternately with device events over 50 calls after a
warm-up, after their outputs are checked against each other; `--repeat N` repeats the whole table to show the run-to-run spread.
One line per case."""
import argparse
import os
import sys
import types

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import ocrs, poolings  # noqa: E402

S, D = 64, 67


def timed(f, n=50):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 32, 256])
    ap.add_argument("--only", choices=["hip", "generic", "torch"], default=None, help="run one side only, untimed (for a kernel trace)")
    args = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    head = poolings.CNN_Linear_Module(D, S * S, types.SimpleNamespace(rep_dim=512)).cuda()
    gen = ocrs.NatureCNN_Module(types.SimpleNamespace(rep_dim=512, use_cnn_feat=False, cnn_feat_size=4),
                                types.SimpleNamespace(obs_size=S, obs_channels=D)).cuda()
    layers = []
    for c in (m for m in head._net._net if isinstance(m, nn.Conv2d)):
        layers += [nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride), nn.ReLU()]
    ref = nn.Sequential(*layers, nn.Flatten(), nn.Linear(1024, 512), nn.ReLU()).cuda()
    with torch.no_grad():
        for dst in (gen, ref):
            for a, b in zip(dst.parameters(), head.parameters()):
                a.copy_(b)

    def nchw(t):
        return t.reshape(t.shape[0], S, S, D).permute(0, 3, 1, 2)

    sides = {"hip": (head, lambda t: head(t)), "generic": (gen, lambda t: gen(nchw(t).contiguous())), "torch": (ref, lambda t: ref(nchw(t)))}
    for rep in range(args.repeat):
        for B in args.batches:
            tokens = torch.rand(B, S * S, D, device="cuda")
            with torch.no_grad():
                outs = {k: f(tokens) for k, (_, f) in sides.items()}
            for k in ("generic", "torch"):
                err = ((outs["hip"] - outs[k]).abs().max() / outs[k].abs().max()).item()
                if not err <= 1e-5:                              # all sides are fp32: a larger difference is a wrong result, not noise
                    raise SystemExit(f"B={B}: HIP and {k} outputs differ by {err:.1e} of the output's max (bound 1e-5)")
            dout = torch.randn(B, 512, device="cuda")
            leaf = tokens.clone().requires_grad_(True)

            def run(kind, mode):
                m, f = sides[kind]
                if mode == "fwd":
                    with torch.no_grad():
                        f(tokens)
                    return
                for p in m.parameters():
                    p.grad = None
                leaf.grad = None
                f(leaf if mode == "dx" else tokens).backward(dout)

            if args.only:
                for mode in ("fwd", "dw", "dx"):
                    if not (args.only == "generic" and mode == "dx"):
                        run(args.only, mode)
                torch.cuda.synchronize()
                continue
            for mode, label in (("fwd", "fwd (no_grad)"), ("dw", "fwd+bwd, tokens detached"), ("dx", "fwd+bwd with dtokens")):
                kinds = ["hip", "torch"] if mode == "dx" else ["hip", "generic", "torch"]
                ms = {k: timed(lambda k=k: run(k, mode)) for k in kinds}
                gen_txt = f"generic {ms['generic']:.3f} ms (HIP/generic {ms['hip'] / ms['generic']:.2f}), " if "generic" in ms else ""
                print(f"[run {rep}] B={B} {label}: HIP {ms['hip']:.3f} ms, {gen_txt}torch fp32 {ms['torch']:.3f} ms "
                      f"(HIP/torch {ms['hip'] / ms['torch']:.2f})", flush=True)


if __name__ == "__main__":
    main()
