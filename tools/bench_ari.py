"""segmentation-ARI micro-benchmark (development aid).  At the IODINE bench shape (B 128, 64x64, 6 mask channels, 7 slot masks, channel-major)
and the Slot-Attention bench shape (B 128, 128x128, 6 mask channels, 6 attention maps stored [B, N, K]):
  before   the path get_loss took before ocrl_ari_counts: cat + multiply + two argmax passes on the GPU, the two label maps copied to the
           host, a numpy contingency table per image (ocrl_amd.utils.tools._adjusted_rand_score)
  after    segmentation_ari: one counting kernel, one kernel for the pair sums, 3 B int64 copied to the host
  kernel   ari_counts alone (memset + both kernels, device events), and its rate against the algorithmic bytes (Ct + K) * N * 4 per image
Host-clock timings end in the device-to-host copy both paths need; every figure is the median of the repeats after a warm-up."""
import os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrl_amd.utils.tools import _adjusted_rand_score, ari_counts, segmentation_ari

assert torch.cuda.is_available(), "bench_ari needs a GPU"
B = int(os.environ.get("B", "128"))


def before(masks, attns):
    fg_mask = 1 - masks[:, -1].unsqueeze(1)
    cat = torch.cat([attns * fg_mask, fg_mask], dim=1)
    t = torch.argmax(masks.flatten(2), dim=1).cpu().numpy()
    p = torch.argmax(cat.flatten(2), dim=1).cpu().numpy()
    return [_adjusted_rand_score(t[b], p[b]) for b in range(t.shape[0])]


def host_ms(f, n, warm=3):
    for _ in range(warm): f()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def event_ms(f, n, warm=5, inner=20):
    for _ in range(warm): f()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner): f()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def shape(tag, S, Ct, K, pixel_major):
    g = torch.Generator(device="cuda").manual_seed(S)
    lab = torch.randint(0, Ct, (B, S // 8, S // 8), device="cuda", generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    masks = torch.nn.functional.one_hot(lab, Ct).permute(0, 3, 1, 2).unsqueeze(2).float().contiguous()
    a = torch.softmax(2.0 * torch.randn(B, S * S, K, device="cuda", generator=g), dim=-1)
    attns = a.transpose(-1, -2).reshape(B, K, 1, S, S) if pixel_major else a.transpose(-1, -2).contiguous().reshape(B, K, 1, S, S)
    want = before(masks, attns)
    assert segmentation_ari(masks, attns) == want, "the two paths disagree"
    # the two paths alternate, so a drift of the machine hits both
    rb, ra = [], []
    for _ in range(3):
        rb.append(host_ms(lambda: before(masks, attns), 7))
        ra.append(host_ms(lambda: segmentation_ari(masks, attns), 21))
    mb, ma = statistics.median(r[0] for r in rb), statistics.median(r[0] for r in ra)
    k = event_ms(lambda: ari_counts(masks, attns, True), 9)
    gb = B * (Ct + K) * S * S * 4 / 1e9
    print(f"{tag}: B {B} {S}x{S} Ct {Ct} K {K} {'[B,N,K]' if pixel_major else '[B,K,N]'} maps, mean ari {np.mean(want):.4f}")
    print(f"  before (torch cat/mul/argmax + label copy + numpy per image): {mb:.3f} ms  (rounds: " + ", ".join(f"{r[0]:.3f}" for r in rb) + ")")
    print(f"  after  (segmentation_ari, incl. the 3 B int64 copy):          {ma:.3f} ms  (rounds: " + ", ".join(f"{r[0]:.3f}" for r in ra) + ")")
    print(f"  ratio before / after: {mb / ma:.1f}x")
    print(f"  ari_counts alone (memset + count + sums, device events): {k[0] * 1e3:.1f} us (min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f}); "
          f"{gb * 1e3:.1f} MB algorithmic -> {gb / (k[0] * 1e-3):.0f} GB/s")
    sys.stdout.flush()


shape("IODINE shape", 64, 6, 7, False)
shape("Slot-Attention shape", 128, 6, 6, True)
