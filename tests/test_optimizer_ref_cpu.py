"""tests/optim_ref.py (the fp64 clip + Adam step the GPU optimiser tests are graded against) pinned to torch.optim.Adam +
torch.nn.utils.clip_grad_norm_ in fp64: both sides do the same operations in the same precision, so they agree to 1e-12 of each
tensor's largest entry; a NaN / inf gradient entry gives a NaN / inf norm on both sides and the same poisoned elements."""
import pytest
import torch

from tests.optim_ref import ref_step

TOL = 1e-12


def layout(gen, sizes_per_group=((7, 130, 64), (33, 5, 256, 12), (1, 97))):
    """three groups of tensors on a flat buffer, every tensor padded to a multiple of four as the engines do"""
    tensors, off = [], 0
    for grp, sizes in enumerate(sizes_per_group):
        for n in sizes:
            tensors.append((off, n, grp))
            off += (n + 3) & ~3
    return tensors, off


def rand_grad(gen, size, tensors, has_grad):
    g = torch.zeros(size, dtype=torch.float64)
    for (o, n, _), h in zip(tensors, has_grad):
        if h:
            g[o:o + n] = torch.randn(n, generator=gen, dtype=torch.float64) * 10 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 4 - 3)
    return g


def close(a, b, tag):
    assert torch.equal(torch.isnan(a), torch.isnan(b)), tag
    fin = ~torch.isnan(b)
    if fin.any():
        den = max(float(b[fin].abs().max()), 1e-300)
        assert float((a[fin] - b[fin]).abs().max()) <= TOL * den, (tag, float((a[fin] - b[fin]).abs().max()), den)


def run_both(steps, norm_type, clip, gscale=1.0, poison=None, seed=0):
    gen = torch.Generator().manual_seed(seed)
    tensors, size = layout(gen)
    has_grad = [i not in (2, 5) for i in range(len(tensors))]          # one tensor of group 0 and one of group 1 never get a gradient
    lrs = (1e-3, 2e-3, 4e-3)
    p = torch.zeros(size, dtype=torch.float64)
    for o, n, _ in tensors:
        p[o:o + n] = torch.randn(n, generator=gen, dtype=torch.float64) * 0.1
    params = [torch.nn.Parameter(p[o:o + n].clone()) for o, n, _ in tensors]
    opt = torch.optim.Adam([{"params": [q for q, (_, _, g) in zip(params, tensors) if g == grp], "lr": lrs[grp]} for grp in range(3)])
    p_init, m, v = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    for t in range(1, steps + 1):
        g = rand_grad(gen, size, tensors, has_grad) * (0.02 if t % 3 == 0 else 1.0)      # some steps clip and some do not
        if poison is not None and t == steps:
            g[tensors[4][0] + 3] = poison
        for q, (o, n, _), h in zip(params, tensors, has_grad):
            q.grad = (g[o:o + n] * gscale).clone() if h else None
        live = [q for q in params if q.grad is not None]
        if clip:
            norm = torch.nn.utils.clip_grad_norm_(live, clip, norm_type=float("inf") if norm_type == "inf" else 2.0)
        else:
            norm = None
        opt.step()
        r = ref_step(p, g, m, v, tensors, lrs, clip, norm_type, t, gscale, has_grad)
        p, m, v = r.p, r.m, r.v
        if norm is not None:
            if torch.isfinite(norm):
                assert abs(float(norm) - float(r.norm)) <= TOL * float(norm), (t, float(norm), float(r.norm))
            else:
                assert str(float(norm)) == str(float(r.norm)), (float(norm), float(r.norm))
    for i, (q, (o, n, _), h) in enumerate(zip(params, tensors, has_grad)):
        close(p[o:o + n], q.detach(), f"p[{i}]")
        if h:
            st = opt.state[q]
            close(m[o:o + n], st["exp_avg"], f"m[{i}]")
            close(v[o:o + n], st["exp_avg_sq"], f"v[{i}]")
            assert float(st["step"]) == steps
        else:
            assert q not in opt.state or not opt.state[q]
            assert float(m[o:o + n].abs().max()) == 0.0 and float(v[o:o + n].abs().max()) == 0.0
    return p, r, p_init


@pytest.mark.parametrize("steps", [1, 25])
@pytest.mark.parametrize("norm_type", ["inf", 2])
@pytest.mark.parametrize("clip", [0.0, 0.05, 5.0])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_ref_step_matches_torch_adam(steps, norm_type, clip, gscale):
    run_both(steps, norm_type, clip, gscale, seed=steps)


def test_clip_coefficient_takes_both_branches():
    """the cases above really exercise coef = 1 and coef < 1"""
    _, r, _ = run_both(1, "inf", 5.0e3)
    assert float(r.coef) == 1.0
    _, r, _ = run_both(1, "inf", 0.05)
    assert 0.0 < float(r.coef) < 1.0
    _, r, _ = run_both(1, 2, 0.05, gscale=0.5)
    assert 0.0 < float(r.coef) < 1.0


@pytest.mark.parametrize("norm_type", ["inf", 2])
@pytest.mark.parametrize("steps", [1, 4])
def test_nan_gradient_poisons_norm_and_every_weight(norm_type, steps):
    p, r, _ = run_both(steps, norm_type, 0.05, poison=float("nan"))
    assert torch.isnan(r.norm) and torch.isnan(r.coef)
    tensors, _ = layout(None)
    for i, (o, n, _) in enumerate(tensors):
        assert bool(torch.isnan(p[o:o + n]).all()) == (i not in (2, 5)), i          # every tensor that has a gradient, and no other


@pytest.mark.parametrize("norm_type", ["inf", 2])
def test_inf_gradient_zeroes_the_step_elsewhere(norm_type):
    """norm = inf -> coef = 0: the element itself becomes inf * 0 = NaN; from a fresh state everything else stays where it was"""
    p, r, p0 = run_both(1, norm_type, 0.05, poison=float("inf"))
    assert torch.isinf(r.norm) and float(r.coef) == 0.0
    tensors, _ = layout(None)
    bad = tensors[4][0] + 3
    assert torch.isnan(p[bad])
    keep = torch.ones_like(p, dtype=torch.bool)
    keep[bad] = False
    assert torch.equal(p[keep], p0[keep])
