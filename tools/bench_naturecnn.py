"""NatureCNN / MultipleCNN encoders (ocrs.NatureCNN_Module / MultipleCNN_Module over ocrl_naturecnn_fwd/_bwd) against torch's own fp32
nn.Sequential of the same layers on the same GPU, at 64 x 64 x 3 (the reference RL setting).

Cases: the rollout forward (B = 4 under no_grad: num_envs images per env step), the PPO minibatch forward + backward (B = 32), a larger
minibatch (B = 256), and MultipleCNN with G = 5 modules (rollout and minibatch).  Both sides run through their Python surface, as PPO
calls them; each case is timed with device events over 50 calls after a warm-up, after the outputs are checked against each other
(the run stops if they differ by more than 1e-5 of the output's max).
One line per case.  The launch counts are those of the C entry points (L = 3 convolutions, G modules): forward L + G (+ 1 copy when
a gradient is needed), backward 1 + 2 G + L + 1."""
import os
import sys
import types

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import ocrs  # noqa: E402

S, C = 64, 3


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


def torch_copy(m):
    """the same module as torch layers: nn.Sequential(Conv2d, ReLU, ..., Flatten, Linear, ReLU) with m's weights"""
    seq = [nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride) for c in m._cnn if isinstance(c, nn.Conv2d)]
    layers = []
    for c in seq:
        layers += [c, nn.ReLU()]
    layers += [nn.Flatten(), nn.Linear(m._linear[0].in_features, m._linear[0].out_features), nn.ReLU()]
    t = nn.Sequential(*layers).cuda()
    src = [p for p in m.parameters()]
    with torch.no_grad():
        for a, b in zip(t.parameters(), src):
            a.copy_(b)
    return t


class TorchMulti(nn.Module):
    def __init__(self, mm):
        super().__init__()
        self.nets = nn.ModuleList([torch_copy(c) for c in mm._cnns])

    def forward(self, x):
        return torch.stack([n(x) for n in self.nets], 1)


def main():
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    env = types.SimpleNamespace(obs_size=S, obs_channels=C)
    one = ocrs.NatureCNN_Module(types.SimpleNamespace(rep_dim=512, use_cnn_feat=False, cnn_feat_size=4), env).cuda()
    multi = ocrs.MultipleCNN_Module(types.SimpleNamespace(rep_dim=512, num_modules=5), env).cuda()
    t_one, t_multi = torch_copy(one), TorchMulti(multi)
    cases = [("NatureCNN rollout fwd (no_grad)", one, t_one, 4, False, 1), ("NatureCNN PPO fwd+bwd", one, t_one, 32, True, 1),
             ("NatureCNN fwd+bwd", one, t_one, 256, True, 1), ("MultipleCNN G=5 rollout fwd (no_grad)", multi, t_multi, 4, False, 5),
             ("MultipleCNN G=5 PPO fwd+bwd", multi, t_multi, 32, True, 5)]
    for name, m, t, B, train, G in cases:
        obs = torch.rand(B, C, S, S, device="cuda")
        with torch.no_grad():
            a, b = m(obs), t(obs)
        err = ((a - b).abs().max() / b.abs().max()).item()
        if not err <= 1e-5:                                  # both sides are fp32: a larger difference is a wrong result, not noise
            raise SystemExit(f"{name} B={B}: HIP and torch outputs differ by {err:.1e} of the output's max (bound 1e-5)")
        dout = torch.randn(a.shape, device="cuda")
        if train:
            def ours():
                for p in m.parameters():
                    p.grad = None
                m(obs).backward(dout)

            def theirs():
                for p in t.parameters():
                    p.grad = None
                t(obs).backward(dout)
            launches = (3 + G + 1) + (1 + 2 * G + 3 + 1)
        else:
            def ours():
                with torch.no_grad():
                    m(obs)

            def theirs():
                with torch.no_grad():
                    t(obs)
            launches = 3 + G
        ms, ms_t = timed(ours), timed(theirs)
        print(f"{name} B={B}: HIP {ms:.3f} ms ({launches} launches), torch fp32 {ms_t:.3f} ms, HIP/torch {ms / ms_t:.2f}; "
              f"output rel diff {err:.1e}")


if __name__ == "__main__":
    main()
