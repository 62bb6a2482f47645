"""Run-to-run bitwise reproducibility of a full training step (forward, backward, clip + Adam; train mode, device RNG).  With
hand-written kernels and no sanitizer on the GPU this is the repo's race detector: a data race, an uninitialised read or
an order-dependent float accumulation shows up as two runs that differ.  Every reduction on the path therefore runs in a fixed
order (two-stage partials, or exact fixed-point integer atomics for the token-embedding scatter-add)."""
import pytest
import torch

from oracle import slate_oracle as O
from tests.gpu_util import dims_from_cfg, load_params
from tests.gpu_util import rng_key as _rng_key

pytestmark = pytest.mark.gpu

CASES = [
    ("slate 32x32", dict(obs_size=32, vocab_size=512, num_slots=5, num_iterations=2, num_dec_blocks=2), 3),
    ("slate 64x64 / vocab 4096 / 4 blocks", dict(obs_size=64, num_slots=6, num_iterations=3), 4),
    ("slate 16 slots", dict(obs_size=32, vocab_size=256, num_slots=16, num_iterations=2, num_dec_blocks=1), 2),
    ("slot-attention (use_bcdec) 32x32", dict(obs_size=32, vocab_size=256, num_slots=6, num_iterations=3, num_dec_blocks=1, use_bcdec=True), 3),
]


@pytest.mark.parametrize("tag,over,B", CASES)
def test_two_runs_are_bitwise_identical(tag, over, B):
    from ocrl_amd.engine import SlateEngine
    cfg = O.default_cfg(**over)
    P = O.formula_params(cfg)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(1)).cuda()
    runs = []
    for _ in range(2):
        eng = SlateEngine(dims_from_cfg(cfg), max_batch=B)
        load_params(eng, P)
        trace = []
        for step in range(3):
            tau, lrs = O.schedules(cfg, step)
            eng.forward(obs, tau, train=True, seed=77 + step)           # Gumbel / slot noise / 21 dropout sites from the device RNG
            eng.backward()
            torch.cuda.synchronize()
            g = eng.flat_g.cpu().clone()
            eng.clip_adam(lrs, cfg.clip)
            trace.append((eng.metrics.cpu().clone(), g))       # loss terms + the gradient norm the clip measured
        torch.cuda.synchronize()
        runs.append((trace, eng.flat_p.cpu().clone(), eng.flat_m.cpu().clone(), eng.flat_v.cpu().clone()))
        del eng
    (ta, pa, ma, va), (tb, pb, mb, vb) = runs
    for step, ((m1, g1), (m2, g2)) in enumerate(zip(ta, tb)):
        assert torch.isfinite(g1).all()
        assert torch.equal(m1[:4], m2[:4]), (tag, step, m1, m2)
        assert torch.equal(g1, g2), (tag, step, int((g1 != g2).sum()), float((g1 - g2).abs().max()))
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)


def test_iodine_two_runs_are_bitwise_identical():
    """IODINE (BASELINE config 4's slot / iteration counts at 32x32): forward with the device RNG, backward, L2 clip + Adam, three steps"""
    from oracle import iodine_oracle as IO
    from tests.test_gpu_iodine import dims
    from ocrl_amd.engine import IodineEngine
    cfg = IO.default_cfg(obs_size=32, num_slots=7, num_iterations=5)
    B = 3
    P = IO.formula_params(cfg)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(2)).cuda()
    runs = []
    for _ in range(2):
        eng = IodineEngine(dims(cfg), max_batch=B)
        load_params(eng, P)
        trace = []
        for step in range(3):
            eng.forward(obs, seed=50 + step)
            eng.backward()
            torch.cuda.synchronize()
            g = eng.flat_g.cpu().clone()
            eng.clip_adam(cfg.lr, cfg.clip)
            trace.append((eng.metrics.cpu().clone(), g))
        torch.cuda.synchronize()
        runs.append((trace, eng.flat_p.cpu().clone()))
        del eng
    (ta, pa), (tb, pb) = runs
    for step, ((m1, g1), (m2, g2)) in enumerate(zip(ta, tb)):
        assert torch.isfinite(g1).all()
        assert torch.equal(m1[:4], m2[:4]), (step, m1, m2)
        assert torch.equal(g1, g2), (step, int((g1 != g2).sum()), float((g1 - g2).abs().max()))
    assert torch.equal(pa, pb)


def test_device_rng_quality():
    """the counter RNG behind dropout / Gumbel / slot noise (csrc/common.h rng_bits4): keep rates per element slot, serial correlation,
    independence across sites and seeds, on the dumped keep-masks of 2^21 elements"""
    import ctypes
    from ocrl_amd import _lib
    from ocrl_amd.engine import SlateEngine
    cfg = O.default_cfg(obs_size=16, vocab_size=256, num_slots=3, num_iterations=1, num_dec_blocks=1)
    eng = SlateEngine(dims_from_cfg(cfg), max_batch=1)
    load_params(eng, O.formula_params(cfg))
    obs = torch.rand(1, 3, 16, 16, device="cuda")
    n = 1 << 21

    def masks(seed, site):
        eng.forward(obs, 1.0, train=True, seed=seed)        # sets the step's seed and dropout probability (0.1)
        return eng.dropout_mask(site, (n,)).cpu().double()

    a, b, c = masks(11, 17), masks(11, 18), masks(12, 17)
    for m in (a, b, c):
        assert abs(m.mean().item() - 0.9) < 2e-3, m.mean()
        for e in range(4):                                  # the four elements of a 64-bit draw
            assert abs(m[e::4].mean().item() - 0.9) < 3e-3, (e, m[e::4].mean())
    corr = lambda x, y: float(((x - x.mean()) * (y - y.mean())).mean() / (x.std() * y.std()))
    assert abs(corr(a[:-1], a[1:])) < 4e-3 and abs(corr(a[:-4], a[4:])) < 4e-3 and abs(corr(a[:-64], a[64:])) < 4e-3      # serial
    assert abs(corr(a, b)) < 4e-3 and abs(corr(a, c)) < 4e-3                                                                   # site / seed
    assert not torch.equal(a, b) and not torch.equal(a, c)


def test_device_rng_streams_are_not_translates():
    """Two (seed, site) streams must not be XOR-translates of each other.  With the key only xor-ed into the counter, stream B at group i
    equalled stream A at group i ^ (kA ^ kB): a whole dropout / Gumbel field re-used as a block permutation.  The test picks two seeds whose
    keys differ only in the low 19 bits (found with the host restatement of rng_key), so the translate, if it existed, would map the
    dumped 2^19 groups onto themselves, and requires the translated masks to agree at chance level only."""
    from ocrl_amd.engine import SlateEngine
    site, nbits = 17, 19
    seen, pair = {}, None
    for s in range(1, 1 << 14):
        k = _rng_key(s, site)
        if (k >> nbits) in seen:
            pair = (seen[k >> nbits], s)
            break
        seen[k >> nbits] = s
    assert pair is not None
    d = _rng_key(pair[0], site) ^ _rng_key(pair[1], site)
    assert 0 < d < (1 << nbits)
    cfg = O.default_cfg(obs_size=16, vocab_size=256, num_slots=3, num_iterations=1, num_dec_blocks=1)
    eng = SlateEngine(dims_from_cfg(cfg), max_batch=1)
    load_params(eng, O.formula_params(cfg))
    obs = torch.rand(1, 3, 16, 16, device="cuda")
    n = 4 << nbits

    def groups(seed):
        eng.forward(obs, 1.0, train=True, seed=seed)
        return eng.dropout_mask(site, (n,)).cpu().view(-1, 4)

    a, b = groups(pair[0]), groups(pair[1])
    idx = torch.arange(1 << nbits) ^ d
    agree = (a[idx] == b).all(1).double().mean().item()        # a whole group of four keep decisions equal
    chance = (0.9 * 0.9 + 0.1 * 0.1) ** 4
    assert abs(agree - chance) < 0.01, (agree, chance, d)
