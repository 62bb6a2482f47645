"""VAE module (ocrs.VAE_Module over ocrl_vae_fwd/_bwd) against torch's own fp32 nn layers with the same weights on the same GPU, at
64 x 64 x 3 (configs/ocr/vae.yaml: latent 256, cnn_feat_size 4, so n = 4 stages).

Cases: one pre-training step (get_loss forward + backward + torch Adam) at B = 24 (configs/_base.yaml), 64 and 256; the encoder-only
rollout forward under no_grad at B = 1, 4 and 16, with use_cnn_feat off (mu) and on (tokens).  Both sides run through their Python
surface with the same recorded eps; each case is timed with device events over 30 calls after a warm-up, after the outputs are
checked against each other (the run stops if they differ by more than 1e-4 of the output's max).  One line per case."""
import os
import sys
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import ocrs  # noqa: E402

S, C = 64, 3


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


def torch_loss(ps, obs, eps, n, f, kw, cnn, encoder_only=False):
    """the reference's VAE_Module arithmetic as torch fp32 layers over the parameter list"""
    it = iter(ps)
    nxt = lambda: (next(it), next(it))
    x = obs
    for _ in range(n):
        w, b = nxt(); x = F.relu(F.conv2d(x, w, b, stride=2))
        for _ in range(3):
            w, b = nxt(); x = F.relu(F.conv2d(x, w, b))
    w, b = nxt(); e = F.conv2d(x, w, b)
    B = obs.shape[0]
    wm, bm = nxt()
    if encoder_only:
        return e.permute(0, 2, 3, 1).reshape(B, -1, 64) if cnn else F.linear(e.reshape(B, -1), wm, bm)
    wv, bv = nxt(); wi, bi = nxt()
    mu, lv = F.linear(e.reshape(B, -1), wm, bm), F.linear(e.reshape(B, -1), wv, bv)
    h = F.linear(eps * torch.exp(0.5 * lv) + mu, wi, bi).reshape(B, 64, f, f)
    w, b = nxt(); h = F.relu(F.conv2d(h, w, b))
    for _ in range(n):
        w, b = nxt(); h = F.relu(F.conv2d(h, w, b, padding=1))
        for _ in range(3):
            w, b = nxt(); h = F.relu(F.conv2d(h, w, b))
        h = F.pixel_shuffle(h, 2)
    w, b = nxt(); recon = F.conv2d(h, w, b)
    mse = ((obs - recon) ** 2).sum() / B
    kld = torch.mean(-0.5 * torch.sum(1 + lv - mu ** 2 - lv.exp(), dim=1), dim=0)
    return mse + kw * kld


def module(cnn):
    cfg = types.SimpleNamespace(name="VAE", latent_dim=256, use_cnn_feat=cnn, cnn_feat_size=4, learning=types.SimpleNamespace(lr=1e-4, kld_weight=1e-4))
    torch.manual_seed(0)
    return ocrs.VAE_Module(cfg, types.SimpleNamespace(obs_size=S, obs_channels=C)).cuda()


def line(case, B, ours, theirs):
    print(f"vae {case:<22} B={B:<4d} hip {ours:8.3f} ms  torch {theirs:8.3f} ms  speedup {theirs / ours:5.2f}x", flush=True)


def main():
    g = torch.Generator().manual_seed(1)
    m = module(False)
    tps = [p.detach().clone().requires_grad_(True) for p in m.parameters()]
    opt_h = torch.optim.Adam(m.parameters(), lr=1e-4)
    opt_t = torch.optim.Adam(tps, lr=1e-4)
    for B in (24, 64, 256):
        obs = torch.rand(B, C, S, S, generator=g).cuda()
        eps = torch.randn(B, 256, generator=g).cuda()
        with torch.no_grad():                         # both sides start each case from the same weights
            for t, q in zip(tps, m.parameters()):
                t.copy_(q)
        a = m.loss_terms(obs, eps)[0]
        b = torch_loss(tps, obs, eps, 4, 4, 1e-4, False)
        assert abs(a.item() - b.item()) <= 1e-4 * abs(b.item()), (a.item(), b.item())

        def hip_step():
            opt_h.zero_grad()
            m.loss_terms(obs, eps)[0].backward()
            opt_h.step()

        def torch_step():
            opt_t.zero_grad()
            torch_loss(tps, obs, eps, 4, 4, 1e-4, False).backward()
            opt_t.step()
        line("train step", B, timed(hip_step), timed(torch_step))
    for cnn in (False, True):
        m = module(cnn)
        ps = [p.detach() for p in m.parameters()]
        for B in (1, 4, 16):
            obs = torch.rand(B, C, S, S, generator=g).cuda()
            with torch.no_grad():
                a, b = m(obs), torch_loss(ps, obs, None, 4, 4, 1e-4, cnn, encoder_only=True)
                assert (a - b).abs().max() <= 1e-4 * b.abs().max(), "encoder outputs differ"
                line(f"rollout {'tokens' if cnn else 'mu'}", B, timed(lambda: m(obs)), timed(lambda: torch_loss(ps, obs, None, 4, 4, 1e-4, cnn, True)))


if __name__ == "__main__":
    main()
