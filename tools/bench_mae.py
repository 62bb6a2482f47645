"""MAE-base (ocrs.MAE over ocrl_mae_fwd/_bwd) against the plain-torch restatement tests/mae_ref.py in float32 eager on the same GPU,
with the same weights and the same recorded masking noise, at 64 x 64, patch 8 (configs/ocr/mae.yaml).

Cases: get_loss + backward at B = 128; update (the same plus torch AdamW) at B = 128; forward (encode_full_patches) for one image
under no_grad.  Each case is timed with device events over `--steps` calls after `--warmup` calls, after the two sides' outputs are
checked against each other (the run stops if they differ by more than 1e-4 of the output's max).  One line per case.

    python tools/bench_mae.py [--batch 128] [--steps 20] [--warmup 3] [--hip-only]

--hip-only skips the torch side (for a kernel trace of the HIP path alone)."""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrl_amd import ocrs  # noqa: E402
from ocrl_amd.ocrs import mae as M  # noqa: E402
from tests import mae_ref as R  # noqa: E402

S, P = 64, 8


def timed(f, steps, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def line(case, B, ours, theirs):
    t = f"torch {theirs:9.3f} ms  speedup {theirs / ours:5.2f}x" if theirs is not None else ""
    print(f"mae-base {case:<22} B={B:<4d} hip {ours:9.3f} ms  {t}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mae: no GPU (there is nothing to measure on the CPU)")
    cfg = types.SimpleNamespace(name="MAE", vit_size="base", patch_size=P, return_cls=False, masking_ratio=0.75,
                                learning=types.SimpleNamespace(lr=1e-3, weight_decay=0.05))
    torch.manual_seed(0)
    w = ocrs.MAE(cfg, types.SimpleNamespace(obs_size=S, obs_channels=3))
    w.to("cuda")
    m = w._module
    enc, dec, keep = M.VIT["base"], M.DECODER, m.len_keep
    g = torch.Generator().manual_seed(1)
    B = a.batch
    obs = torch.rand(B, 3, S, S, generator=g).cuda()
    noise = torch.rand(B, m._num_patches, generator=g).cuda()
    tps = [p.detach().clone().requires_grad_(p.requires_grad) for p in m.parameters()]
    opt_t = torch.optim.AdamW([t for t in tps if t.requires_grad], lr=1e-3, betas=(0.9, 0.95))

    def hip_loss():
        m.zero_grad(set_to_none=True)
        m.get_loss(obs, noise=noise)["loss"].backward()

    def torch_loss():
        for t in tps:
            t.grad = None
        R.loss_terms(obs, tps, noise, P, enc, dec, keep)["loss"].backward()

    m.draw_noise = lambda o: noise
    hip_update = lambda: w.update(obs, None, 0)

    def torch_update():
        opt_t.zero_grad()
        R.loss_terms(obs, tps, noise, P, enc, dec, keep)["loss"].backward()
        opt_t.step()

    if not a.hip_only:
        x, y = m.get_loss(obs, noise=noise)["loss"], R.loss_terms(obs, tps, noise, P, enc, dec, keep)["loss"]
        assert abs(x.item() - y.item()) <= 1e-4 * abs(y.item()), (x.item(), y.item())
    line("get_loss + backward", B, timed(hip_loss, a.steps, a.warmup), None if a.hip_only else timed(torch_loss, a.steps, a.warmup))
    line("update", B, timed(hip_update, a.steps, a.warmup), None if a.hip_only else timed(torch_update, a.steps, a.warmup))
    one = obs[:1].contiguous()
    with torch.no_grad():
        ps = [t.detach() for t in m.parameters()]      # after the updates: the weights the module now holds
        if not a.hip_only:
            x, y = m(one), R.encode_full(one, ps, P, enc[1], enc[2])[:, 1:]
            assert (x - y).abs().max() <= 1e-4 * y.abs().max(), "encoder outputs differ"
        line("forward", 1, timed(lambda: m(one), 10 * a.steps, a.warmup),
             None if a.hip_only else timed(lambda: R.encode_full(one, ps, P, enc[1], enc[2]), 10 * a.steps, a.warmup))


if __name__ == "__main__":
    main()
