"""What the classifier's fused step costs (``ocrl_clf_ce_fwd_bwd``, include/ocrl_hip_classifier.h) against the generic path on the same
build: ``ocrl_qnet_fwd`` with save, the cross-entropy and its gradient formed by torch from the returned logits
(``torch.nn.functional.cross_entropy`` + ``backward`` + ``argmax``), then ``ocrl_qnet_bwd``.  The classifier's own head (one hidden
layer of 64, ReLU), batch 128, 4 labels, on F = 128 features (a Transformer / MLP pooling head) and F = 1152 (Identity pooling of
6 slots x 192).

    fused_ms / generic_ms   the median over `--rounds` rounds of the median over `--calls` individually timed calls after warm-up, each
                            between two events on the stream (tools/bench_acnet.py's method); the two paths alternate within a round
    *_spread                the largest minus the smallest of the rounds' medians: what a difference has to exceed
    eval_ms                 the same entry point evaluating (dw == NULL: two launches, no backward)
    max_grad_diff           the largest difference between the two paths' gradients over the largest gradient, at the timed size

Both sides are timed from Python through ctypes, as ``Classifier`` calls them."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import _lib  # noqa: E402
from tools.bench_acnet import median_ms  # noqa: E402

SHAPES = [(128, 128, 4), (128, 1152, 4)]
DIMS, ACTS = (64,), (1,)


def make(B, F, A):
    g = torch.Generator().manual_seed(B + F)
    ps, k = [], F
    for n in DIMS + (A,):
        ps += [((torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5).cuda(), ((torch.rand(n, generator=g) * 2 - 1) / k ** 0.5).cuda()]
        k = n
    return torch.randn(B, F, generator=g).cuda(), ps, torch.randint(0, A, (B,), generator=g).cuda()


def bench_shape(B, F, A, calls, rounds):
    L = _lib.lib()
    x, ps, labels = make(B, F, A)
    d = _lib.qnet_desc(B, F, A, DIMS, ACTS)
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    ws = torch.empty(n, device="cuda")
    scal, logits, dx = torch.empty(3, device="cuda"), torch.empty(B, A, device="cuda"), torch.empty(B, F, device="cuda")
    dw, dw2, dx2 = [torch.empty_like(p) for p in ps], [torch.empty_like(p) for p in ps], torch.empty(B, F, device="cuda")
    r, st = ctypes.byref(d), _lib.stream()
    px, pp, pl, ps_, pz, pdx, pdw, pws = _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(labels), _lib.ptr(scal), _lib.ptr(logits), _lib.ptr(dx), _lib.ptrs(dw), _lib.ptr(ws)
    pdx2, pdw2 = _lib.ptr(dx2), _lib.ptrs(dw2)

    def fused():
        _lib.check(L.ocrl_clf_ce_fwd_bwd(r, px, pp, pl, ps_, pz, pdx, pdw, pws, n, st))

    def evaluate():
        _lib.check(L.ocrl_clf_ce_fwd_bwd(r, px, pp, pl, ps_, pz, None, None, pws, n, st))

    def generic():
        _lib.check(L.ocrl_qnet_fwd(r, px, pp, pz, 1, pws, n, st))
        z = logits.detach().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(z, labels)
        loss.backward()
        acc = (z.detach().argmax(dim=1) == labels).float().mean()
        dq = z.grad.contiguous()
        _lib.check(L.ocrl_qnet_bwd(r, px, pp, _lib.ptr(dq), pdx2, pdw2, pws, n, st))
        return loss, acc

    fused()
    generic()
    torch.cuda.synchronize()
    gmax = max(g.abs().max().item() for g in [dx2] + dw2)
    diff = max((a - b).abs().max().item() for a, b in zip([dx] + dw, [dx2] + dw2)) / gmax
    fm, gm, em = [], [], []
    for _ in range(rounds):                                 # alternate: a drift of the machine lands on both sides
        fm.append(median_ms(fused, calls))
        gm.append(median_ms(generic, calls))
        em.append(median_ms(evaluate, calls))
    return dict(fused_ms=round(statistics.median(fm), 5), fused_spread=round(max(fm) - min(fm), 5), generic_ms=round(statistics.median(gm), 5),
                generic_spread=round(max(gm) - min(gm), 5), eval_ms=round(statistics.median(em), 5), max_grad_diff=float(f"{diff:.2e}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classifier: no GPU: nothing is measured without one")
    out = {f"B{B}_F{F}_A{A}": bench_shape(B, F, A, a.calls, a.rounds) for B, F, A in SHAPES}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
