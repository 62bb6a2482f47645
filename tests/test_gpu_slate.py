"""Whole-path parity: the HIP SLATE step (through the C ABI) against the CPU oracle on identical weights,
inputs and injected noise.  Stated tolerances (fp32, different summation order):
  loss terms 1e-5 rel; activations 1e-4 rel (max-norm); parameters after Adam steps 1e-5 rel;
  gradients GRAD_TOL of each tensor's max (floored at 1e-5 x the largest gradient) against an fp64 run of the oracle that uses the
  ReLU decisions of the HIP forward (tests/gpu_util.py: a pre-activation inside rounding noise of zero may fall either way in any
  fp32 evaluation, and one such flip moves a weight gradient by ~1/N of its max; holding the masks fixed removes that coin toss
  and lets the tolerance be tight.  GRAD_TOL = 3x the worst value measured over all cases of this file and test_gpu_fullconfig.py)."""
import numpy as np
import pytest
import torch

from tests.gpu_util import assert_knife_edge, dims_from_cfg, grad_floor, hip_relu_masks, load_params, log, mask_matched_fp64_grads, relerr
from oracle import slate_oracle as O

pytestmark = pytest.mark.gpu
GRAD_TOL = 5e-5      # worst measured: 2.0e-5 (config Z, self-attention q/k projections, T = 4096); <= 9e-6 in every other case

SMALL = dict(obs_size=16, vocab_size=256, num_slots=6, num_iterations=3, num_dec_blocks=2)
MID = dict(obs_size=32, vocab_size=512, num_slots=5, num_iterations=2, num_dec_blocks=2)
LONG = dict(obs_size=64, vocab_size=256, num_slots=4, num_iterations=1, num_dec_blocks=1)     # T = 256: four causal key tiles
K16 = dict(obs_size=16, vocab_size=256, num_slots=16, num_iterations=2, num_dec_blocks=1)     # BASELINE config 5's slot count (two slot blocks)
K11 = dict(obs_size=16, vocab_size=256, num_slots=11, num_iterations=2, num_dec_blocks=1)     # uneven slot blocks (6 + 5)
RAGGED = dict(obs_size=24, vocab_size=256, num_slots=3, num_iterations=2, num_dec_blocks=1)   # 24x24: partial conv tiles, T = 36 < one attention tile, N = 576
V4096 = dict(obs_size=16, vocab_size=4096, num_slots=4, num_iterations=2, num_dec_blocks=1)   # real vocabulary: the 16-values-per-thread vocabulary kernels
HARD = dict(obs_size=16, vocab_size=256, num_slots=4, num_iterations=2, num_dec_blocks=1, hard=True)   # straight-through dVAE sample
# several slot-attention heads (ocrs/common/slot_attn.py:54-92): 12, 16 and 15 soft-max columns
HEADS2 = dict(obs_size=16, vocab_size=256, num_slots=6, num_iterations=3, num_dec_blocks=2, num_slot_heads=2)
HEADS4 = dict(obs_size=16, vocab_size=256, num_slots=4, num_iterations=2, num_dec_blocks=1, num_slot_heads=4)
HEADS3 = dict(obs_size=32, vocab_size=256, num_slots=5, num_iterations=2, num_dec_blocks=1, num_slot_heads=3)


def make_engine(cfg, B):
    from ocrl_amd.engine import SlateEngine
    return SlateEngine(dims_from_cfg(cfg), max_batch=B + 1)      # the workspace is sized for a larger batch than the one that runs


def dev_noise(cfg, noise):
    B = noise["z"].shape[0]
    T = (cfg.obs_size // 4) ** 2
    f = lambda t: t.permute(0, 2, 3, 1).reshape(B, T, cfg.vocab_size).contiguous().cuda()
    return dict(z=f(noise["z"]), z_hard=f(noise["z_hard"]), slots=noise["slots"].contiguous().cuda())


def site_masks(eng, cfg, B):
    """dropout keep-masks of the last forward, keyed for the oracle"""
    T = (cfg.obs_size // 4) ** 2
    d, h, K = cfg.d_model, cfg.num_dec_heads, cfg.num_slots
    M = {"z_pos": eng.dropout_mask(1, (B, T + 1, d)).cpu()}
    for b in range(cfg.num_dec_blocks):
        s = 16 + 8 * b
        M[f"blk{b}.self.attn"] = eng.dropout_mask(s + 0, (B, h, T, (T + 3) & ~3))[..., :T].cpu()      # key stride T4: csrc/common.h attn_drop_ld
        M[f"blk{b}.self.out"] = eng.dropout_mask(s + 1, (B, T, d)).cpu()
        M[f"blk{b}.cross.attn"] = eng.dropout_mask(s + 2, (B, h, T, K)).cpu()
        M[f"blk{b}.cross.out"] = eng.dropout_mask(s + 3, (B, T, d)).cpu()
        M[f"blk{b}.ffn"] = eng.dropout_mask(s + 4, (B, T, d)).cpu()
    return M


def compare_forward(tag, eng, cfg, res, B, noise, tau):
    S, E = cfg.obs_size, cfg.obs_size // 4
    T, N, V, K, D, d = E * E, S * S, cfg.vocab_size, cfg.num_slots, cfg.slot_size, cfg.d_model
    errs = {}
    zraw = eng.tensor("zraw", (B, T, V)).double().cpu()
    if not cfg.hard:
        # soft samples: the head GEMM's epilogue leaves the Gumbel scores (logits + g1) / tau, not the logits (z is rebuilt from them on
        # the fly); with the injected Exp(1) noise e1, g1 = -log(e1 + tiny), so the logits are recovered for the z_logits comparison
        e1 = dev_noise(cfg, noise)["z"].double().cpu().reshape(B, T, V)
        zraw = zraw * tau + torch.log(e1 + 1.17549435e-38)
    zl = torch.log_softmax(zraw, -1)
    errs["z_logits"] = relerr(zl, res["z_logits"].permute(0, 2, 3, 1).reshape(B, T, V))
    errs["z"] = relerr(eng.tensor("z_st" if cfg.hard else "z", (B, T, V)), res["z"].permute(0, 2, 3, 1).reshape(B, T, V))
    tok = eng.tensor("tokens", (B, T), torch.int32).cpu().long()
    errs["tokens_mismatch"] = float((tok != res["tokens"]).sum().item())
    errs["recon"] = relerr(eng.tensor("recon", (B, S, S, 4))[..., :3].permute(0, 3, 1, 2), res["recon"])
    errs["feats"] = relerr(eng.tensor("feats", (B, N, 64)), res["feats"])
    errs["slots"] = relerr(eng.tensor("slots", (B, K, D)), res["slots"])
    errs["attn"] = relerr(eng.tensor("attn", (B, N, K)), res["attn"])
    errs["dec_out"] = relerr(eng.tensor("dec_out", (B, T, d)), res["dec_out"])
    m = eng.metrics.cpu()
    errs["dvae_mse"] = abs(m[0].item() - res["dvae_mse"].item()) / abs(res["dvae_mse"].item())
    errs["cross_entropy"] = abs(m[1].item() - res["cross_entropy"].item()) / abs(res["cross_entropy"].item())
    errs["loss"] = abs(m[2].item() - res["loss"].item()) / abs(res["loss"].item())
    log(f"[{tag}] forward: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    return errs


def compare_grads(tag, eng, trainer, cfg=None, P=None, obs=None, noise=None, step=0, drop_masks=None):
    """every parameter gradient of the HIP backward against (a) the fp32 oracle's autograd (logged) and (b) an fp64 run of the oracle
    under the HIP forward's ReLU decisions (graded: returns its worst per-tensor error)"""
    names = [p.name for p in eng.params if trainer.P[p.name].grad is not None]
    gmax = max(trainer.P[n].grad.abs().max().item() for n in names)
    worst32, rows32 = 0.0, []
    for p in eng.params:
        ref = trainer.P[p.name].grad
        if ref is None:
            assert float(eng.view(eng.flat_g, p).abs().max()) == 0.0, p.name          # no gradient in this mode
            continue
        e = relerr(eng.view(eng.flat_g, p), ref.reshape(p.shape), floor=grad_floor(p.name, gmax))
        rows32.append((e, p.name))
        worst32 = max(worst32, e)
    rows32.sort(reverse=True)
    if cfg is None:
        log(f"[{tag}] grads vs fp32 oracle: worst {worst32:.2e}; top: " + "; ".join(f"{n}={e:.1e}" for e, n in rows32[:6]))
        return worst32, rows32
    B = obs.shape[0]
    t64, fr = mask_matched_fp64_grads(cfg, P, obs, noise, step, hip_relu_masks(eng, cfg, B), drop_masks)
    assert_knife_edge(fr, tag)
    worst, rows = 0.0, []
    for p in eng.params:
        ref = t64.P[p.name].grad
        if ref is None:
            continue
        e = relerr(eng.view(eng.flat_g, p), ref.reshape(p.shape), floor=grad_floor(p.name, gmax))
        rows.append((e, p.name))
        worst = max(worst, e)
    rows.sort(reverse=True)
    log(f"[{tag}] grads vs mask-matched fp64 oracle: worst {worst:.2e} ({fr.flips} of {fr.units} ReLU decisions differ from fp64's own"
        + (f", largest |pre-activation| among them {max(fr.min_flipped):.1e}" if fr.flips else "") + f"); vs fp32 oracle as is: worst {worst32:.2e} "
        f"({rows32[0][1]}); top: " + "; ".join(f"{n}={e:.1e}" for e, n in rows[:5]))
    return worst, rows


@pytest.mark.parametrize("tag,over,B", [("small", SMALL, 2), ("mid", MID, 3), ("long", LONG, 2), ("k16", K16, 2), ("k11", K11, 2), ("hard", HARD, 2), ("ragged", RAGGED, 3), ("v4096", V4096, 2),
                                         ("heads2", HEADS2, 2), ("heads4", HEADS4, 3), ("heads3", HEADS3, 2)])
def test_forward_backward_eval(tag, over, B):
    """dropout off: every stage of the forward, then every parameter gradient"""
    cfg = O.default_cfg(**over)
    P = O.formula_params(cfg)
    eng = make_engine(cfg, B)
    load_params(eng, P)
    # seed 100 puts one FFN pre-activation of the "mid" case at 6e-7: a ReLU on the rounding knife-edge, whose mask (and with it a
    # whole gradient row) flips with the summation order of the slot means.  Seed 102 keeps every pre-activation above 5e-6.
    g = torch.Generator().manual_seed(102 if tag == "mid" else 100)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=g)
    noise = O.make_noise(cfg, B, 7)
    step = 10
    tau, _ = O.schedules(cfg, step)
    tr = O.OracleTrainer(cfg, P)
    res = tr.loss_and_grads(obs, noise, step, None)
    eng.forward(obs.cuda(), tau, train=False, seed=1, noise=dev_noise(cfg, noise))
    torch.cuda.synchronize()
    errs = compare_forward(tag, eng, cfg, res, B, noise, tau)
    assert errs["tokens_mismatch"] == 0
    for k in ("dvae_mse", "cross_entropy", "loss"):
        assert errs[k] < 1e-5, (k, errs[k])
    for k in ("z_logits", "z", "recon", "feats", "slots", "attn", "dec_out"):
        assert errs[k] < 1e-4, (k, errs[k])
    eng.backward()
    torch.cuda.synchronize()
    worst, rows = compare_grads(tag, eng, tr, cfg, P, obs, noise, step)
    assert worst < GRAD_TOL, rows[:5]


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_odd_token_count_is_refused(dropout):
    """obs_size = 12 (T = 9 tokens): outside self-attention the step's kernels assume T % 4 == 0, so the configuration is refused with
    the reason when the engine is created -- with and without dropout -- instead of being computed wrong"""
    cfg = O.default_cfg(obs_size=12, vocab_size=256, num_slots=3, num_iterations=2, num_dec_blocks=1, dropout=dropout)
    with pytest.raises(RuntimeError, match="obs_size 12 gives 9 tokens.*multiple of 8"):
        make_engine(cfg, 2)


@pytest.mark.parametrize("over", [SMALL, LONG])
def test_train_mode_dropout_parity(over):
    """train mode: the oracle consumes the exact keep-masks the kernels derived from the seed"""
    cfg = O.default_cfg(**over)
    B = 2
    P = O.formula_params(cfg)
    eng = make_engine(cfg, B)
    load_params(eng, P)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(5))
    noise = O.make_noise(cfg, B, 11)
    eng.forward(obs.cuda(), 1.0, train=True, seed=1234, noise=dev_noise(cfg, noise))
    eng.backward()
    torch.cuda.synchronize()
    masks = site_masks(eng, cfg, B)
    keep = np.mean([m.mean().item() for m in masks.values()])
    assert abs(keep - 0.9) < 0.01, keep
    tr = O.OracleTrainer(cfg, P)
    res = tr.loss_and_grads(obs, noise, 0, masks)
    m = eng.metrics.cpu()
    e = abs(m[2].item() - res["loss"].item()) / abs(res["loss"].item())
    log(f"[dropout] loss rel err {e:.2e} keep-rate {keep:.4f}")
    assert e < 1e-5
    worst, rows = compare_grads("dropout", eng, tr, cfg, P, obs, noise, 0, masks)
    assert worst < GRAD_TOL, rows[:5]


def test_update_steps_match_oracle():
    """three full update() steps (clip + Adam, schedules) against the oracle trainer: a whole-path smoke check.  At these warm-up
    learning rates (lr_enc <= 1e-8, lr_dec <= 3e-8) the bars do not constrain groups 1 and 2; the optimiser's own parity is in
    tests/test_gpu_optimizer.py"""
    cfg = O.default_cfg(**SMALL)
    B = 2
    P = O.formula_params(cfg)
    eng = make_engine(cfg, B)
    load_params(eng, P)
    tr = O.OracleTrainer(cfg, P)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(9))
    for step in range(3):
        noise = O.make_noise(cfg, B, 20 + step)
        tau, lrs = O.schedules(cfg, step)
        res = tr.update(obs, noise, step, None)
        eng.forward(obs.cuda(), tau, train=False, seed=step, noise=dev_noise(cfg, noise))
        eng.backward()
        eng.clip_adam(lrs, cfg.clip)
        torch.cuda.synchronize()
        m = eng.metrics.cpu()
        el = abs(m[2].item() - res["loss"].item()) / abs(res["loss"].item())
        en = abs(m[3].item() - float(res["norm"])) / float(res["norm"])
        worst = max(relerr(eng.view(eng.flat_p, p), tr.P[p.name].reshape(p.shape)) for p in eng.params)
        log(f"[update] step {step}: loss err {el:.2e} norm err {en:.2e} worst param err {worst:.2e}")
        assert el < 1e-5 and en < 1e-5 and worst < 1e-5


def test_encode_matches_forward_slots():
    cfg = O.default_cfg(**SMALL)
    B = 2
    P = O.formula_params(cfg)
    eng = make_engine(cfg, B)
    load_params(eng, P)
    obs = torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(3))
    noise = O.make_noise(cfg, B, 4)
    eng.encode(obs.cuda(), seed=0, slot_noise=noise["slots"].cuda())
    torch.cuda.synchronize()
    feats = O.cnn_encode(P, obs)
    slots, attn = O.slot_encoder(P, feats, noise["slots"], cfg)
    e1, e2 = relerr(eng.tensor("slots", (B, 6, 192)), slots), relerr(eng.tensor("attn", (B, 256, 6)), attn)
    log(f"[encode] slots {e1:.2e} attn {e2:.2e}")
    assert e1 < 1e-4 and e2 < 1e-4
    a = eng.tensor("attn", (B, 256, 6)).sum(-1)
    assert torch.allclose(a, torch.ones_like(a), atol=1e-5)      # softmax over slots sums to one at every position


def test_encode_graph_replay_matches_eager(monkeypatch):
    """the inference path at tiny batches (model(obs), slate_module.py:181-196) replays a captured hipGraph from its second call at a
    batch size on (csrc/slate_model.cpp SlateModel::encode): every replay must see the new observation and the new noise seed, i.e.
    equal the eager launches bit for bit"""
    cfg = O.default_cfg(**SMALL)
    P = O.formula_params(cfg)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("OCRL_ENCODE_GRAPH", mode)
        eng = make_engine(cfg, 4)
        load_params(eng, P)
        res = []
        for i in range(5):
            B = 2 if i != 3 else 4          # a second batch size in between: its own warm-up and graph
            obs = torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(40 + i)).cuda()
            eng.encode(obs, seed=90 + i)
            torch.cuda.synchronize()
            res.append((eng.tensor("slots", (B, 6, 192)).cpu().clone(), eng.tensor("attn", (B, 256, 6)).cpu().clone()))
        outs[mode] = res
    for (s1, a1), (s0, a0) in zip(outs["1"], outs["0"]):
        assert torch.equal(s1, s0) and torch.equal(a1, a0)
    assert not torch.equal(outs["1"][1][0], outs["1"][2][0])          # different observations / seeds give different slots


def test_soft_sample_on_request():
    """The fused heads keep the Gumbel scores, not z: ocrl_slate_soft_z rebuilds z = softmax(scores) between forward and backward
    (get_loss(with_rep=True), slate_module.py:239-241) and refuses once the backward has overwritten the scores with their gradient;
    the hard sample's tokens are the arg-max of the second Gumbel draw, i.e. distributed like z's underlying categorical."""
    cfg = O.default_cfg(**V4096)
    B = 2
    eng = make_engine(cfg, B)
    load_params(eng, O.formula_params(cfg))
    S = cfg.obs_size
    T, V = (S // 4) ** 2, cfg.vocab_size
    obs = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(3)).cuda()
    noise = O.make_noise(cfg, B, 11)
    tau = 0.7
    eng.forward(obs, tau, train=False, seed=2, noise=dev_noise(cfg, noise))
    scores = eng.tensor("zraw", (B, T, V)).clone()
    lse = eng.tensor("z_lse", (B, T)).clone()
    z = eng.tensor("z", (B, T, V)).clone()
    assert torch.allclose(lse.double(), torch.logsumexp(scores.double(), -1), atol=1e-5)
    assert relerr(z, torch.softmax(scores.double(), -1)) < 2e-6
    e2 = dev_noise(cfg, noise)["z_hard"]
    hard = ((scores * tau + torch.log(dev_noise(cfg, noise)["z"] + 1.17549435e-38)) - torch.log(e2 + 1.17549435e-38)).argmax(-1)   # logits + g2
    assert (hard.cpu() == eng.tensor("tokens", (B, T), torch.int32).cpu().long()).float().mean() > 0.999
    eng.backward()
    with pytest.raises(RuntimeError, match="soft_z"):
        eng.tensor("z", (B, T, V))


def test_device_rng_statistics():
    """no injected noise: Gumbel / slot noise / dropout come from the device RNG; check determinism per seed,
    sensitivity to the seed, and that z rows are distributions"""
    cfg = O.default_cfg(**SMALL)
    B = 2
    eng = make_engine(cfg, B)
    load_params(eng, O.formula_params(cfg))
    obs = torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(3)).cuda()
    T, V = 16, cfg.vocab_size
    out = []
    for seed in (5, 5, 6):
        eng.forward(obs, 1.0, train=True, seed=seed)
        torch.cuda.synchronize()
        out.append((eng.metrics.cpu().clone(), eng.tensor("z", (B, T, V)).cpu().clone(), eng.tensor("slots0", (B, 6, 192)).cpu().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][1], out[2][1])
    z = out[0][1]
    assert torch.allclose(z.sum(-1), torch.ones(B, T), atol=1e-4) and (z >= 0).all()
    s0 = out[0][2]
    mu = O.formula_params(cfg)["_slotattn.slot_mu"]
    sig = torch.exp(O.formula_params(cfg)["_slotattn.slot_log_sigma"])
    eps = (s0 - mu) / sig
    assert abs(eps.mean().item()) < 0.1 and abs(eps.std().item() - 1.0) < 0.1
    assert torch.isfinite(out[0][0][:3]).all()


def test_device_hard_sample_follows_the_softmax():
    """Device-RNG mode draws the hard Gumbel sample (slate_module.py:127: argmax of logits + Gumbel noise, i.e. a draw from
    Categorical(soft-max(logits))) by inverse CDF over per-segment masses (csrc/elementwise.hip softmax_stat_combine_kernel).  Over many
    seeds the token counts must follow soft-max(logits) of each position: per vocabulary entry the standardised count deviation stays
    inside +-5 sigma, and entries no position gives mass to are never drawn."""
    cfg = O.default_cfg(obs_size=16, vocab_size=256, num_slots=3, num_iterations=1, num_dec_blocks=1)
    B, T, V = 8, 16, cfg.vocab_size
    P = O.formula_params(cfg)
    eng = make_engine(cfg, B)
    load_params(eng, P)
    # flatter logits than the closed-form weights give: scale the head so that many entries carry mass
    eng.param("_dvae._encoder.7.weight").mul_(0.05)
    eng.param("_dvae._encoder.7.bias").mul_(0.05)
    obs = torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(3)).cuda()
    eng.forward(obs, 1.0, train=False, seed=1)
    h = eng.tensor("dvae_enc6", (B * T, 64)).double().cpu()
    W = eng.param("_dvae._encoder.7.weight").reshape(V, 64).double().cpu()
    bias = eng.param("_dvae._encoder.7.bias").double().cpu()
    prob = torch.softmax(h @ W.T + bias, -1)                       # [B*T, V]
    nrun = 400
    counts = torch.zeros(B * T, V, dtype=torch.float64)
    for seed in range(nrun):
        eng.forward(obs, 1.0, train=False, seed=1000 + seed)
        tok = eng.tensor("tokens", (B * T,), torch.int32).cpu().long()
        counts[torch.arange(B * T), tok] += 1
    exp = nrun * prob
    var = (nrun * prob * (1 - prob)).sum(0)
    z = (counts.sum(0) - exp.sum(0)) / var.clamp_min(1e-9).sqrt()
    live = var > 1.0
    assert live.sum() >= 8, "the test needs several vocabulary entries with mass"
    assert z[live].abs().max() < 5.0, (z[live].abs().max(), int(live.sum()))
    assert counts.sum(0)[exp.sum(0) < 1e-6].sum() == 0                 # entries without mass are never drawn
    # per position: the most likely token is drawn about as often as its probability says
    top = prob.argmax(-1)
    ptop = prob[torch.arange(B * T), top]
    ctop = counts[torch.arange(B * T), top]
    zt = (ctop - nrun * ptop) / (nrun * ptop * (1 - ptop)).clamp_min(1e-9).sqrt()
    assert zt.abs().max() < 5.0, zt.abs().max()
    log(f"[hard sample] {nrun} seeds x {B * T} positions: max |z| over {int(live.sum())} vocabulary entries {z[live].abs().max():.2f}, over the positions' top tokens {zt.abs().max():.2f}")


BC = dict(obs_size=16, vocab_size=256, num_slots=6, num_iterations=3, num_dec_blocks=1, use_bcdec=True)
BC32 = dict(obs_size=32, vocab_size=256, num_slots=4, num_iterations=2, num_dec_blocks=1, use_bcdec=True)
BC12 = dict(obs_size=16, vocab_size=256, num_slots=12, num_iterations=2, num_dec_blocks=1, use_bcdec=True)      # more than 8 slots


@pytest.mark.parametrize("tag,over,B", [("bcdec16", BC, 2), ("bcdec32", BC32, 3), ("bcdec_k12", BC12, 2),
                                         ("bcdec_heads2", dict(BC, num_slot_heads=2), 2), ("bcdec32_heads4", dict(BC32, num_slot_heads=4), 2)])
def test_broadcast_decoder_config_matches_oracle(tag, over, B):
    """Slot-Attention configuration (use_bcdec): loss, reconstruction, every gradient, then two update() steps"""
    cfg = O.default_cfg(**over)
    P = O.formula_params(cfg)
    eng = make_engine(cfg, B)
    load_params(eng, P)
    S, K, D = cfg.obs_size, cfg.num_slots, cfg.slot_size
    obs = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(21))
    tr = O.OracleTrainer(cfg, P)
    for step in range(2):
        noise = O.make_noise(cfg, B, 30 + step)
        tau, lrs = O.schedules(cfg, step)
        tr2 = O.OracleTrainer(cfg, {n: p.detach() for n, p in tr.P.items()})
        res = tr2.loss_and_grads(obs, noise, step, None)
        eng.forward(obs.cuda(), tau, train=False, seed=step, noise=dict(slots=noise["slots"].cuda()))
        eng.backward()
        torch.cuda.synchronize()
        m = eng.metrics.cpu()
        el = abs(m[2].item() - res["loss"].item()) / abs(res["loss"].item())
        er = relerr(eng.tensor("recon", (B, S, S, 4))[..., :3].permute(0, 3, 1, 2), res["recon_bc"])
        es = relerr(eng.tensor("slots", (B, K, D)), res["slots"])
        worst, rows = compare_grads(f"{tag} step {step}", eng, tr2, cfg, {n: p.detach() for n, p in tr.P.items()}, obs, noise, step)
        log(f"[{tag}] step {step}: loss {el:.2e} recon {er:.2e} slots {es:.2e}")
        assert el < 1e-5 and er < 1e-4 and es < 1e-4 and worst < GRAD_TOL, rows[:5]
        tr.update(obs, noise, step, None)
        eng.clip_adam(lrs, cfg.clip)
        torch.cuda.synchronize()
        wp = max(relerr(eng.view(eng.flat_p, p), tr.P[p.name].reshape(p.shape)) for p in eng.params)
        log(f"[{tag}] step {step}: worst param err after update {wp:.2e}")
        assert wp < 1e-5


@pytest.mark.parametrize("tag,over,B", [("small", SMALL, 2), ("a64", dict(obs_size=64, num_slots=6, num_iterations=3), 2)])
def test_autoregressive_generation_matches_oracle(tag, over, B):
    """_gen_imgs (slate_module.py:163-179): the KV-cached greedy decode + dVAE decode against the reference's growing-prefix loop restated
    on the oracle (a64: real 64x64 configuration, T = 256 tokens, vocab 4096, 4 blocks)"""
    import torch.nn.functional as F
    cfg = O.default_cfg(**over)
    P = O.formula_params(cfg)
    eng = make_engine(cfg, B)
    load_params(eng, P)
    S, E = cfg.obs_size, cfg.obs_size // 4
    obs = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(3))
    noise = O.make_noise(cfg, B, 4)
    eng.forward(obs.cuda(), 1.0, train=False, seed=0, noise=dev_noise(cfg, noise))
    eng.generate()
    torch.cuda.synchronize()
    T, V = E * E, cfg.vocab_size
    # oracle: grow the prefix exactly as the reference does
    feats = O.cnn_encode(P, obs)
    slots, _ = O.slot_encoder(P, feats, noise["slots"], cfg)
    mem = F.linear(slots, P["_slotproj.weight"])
    inp = P["_bos_token._bos_token"].expand(B, 1, -1)
    toks = []
    for t in range(T):
        dec = O.transformer_decoder(P, inp + P["_z_pos.pe"][:, :inp.shape[1]], mem, cfg)
        nxt = F.linear(dec, P["_out.weight"])[:, -1].argmax(-1)
        toks.append(nxt)
        inp = torch.cat([inp, F.embedding(nxt, P["_dict.dictionary.weight"]).unsqueeze(1)], 1)
    toks = torch.stack(toks, 1)
    zg = F.one_hot(toks, V).float().transpose(1, 2).reshape(B, V, E, E)
    rec = O.dvae_decode(P, zg)
    got_tok = eng.tensor("tokens", (B, T), torch.int32).cpu().long()
    assert torch.equal(got_tok, toks), (got_tok, toks)
    e = relerr(eng.tensor("recon", (B, S, S, 4))[..., :3].permute(0, 3, 1, 2), rec)
    mse = ((obs - rec) ** 2).sum() / B
    em = abs(eng.metrics.cpu()[4].item() - mse.item()) / mse.item()
    log(f"[gen_imgs {tag}] {T} tokens exact, recon {e:.2e} mse {em:.2e}")
    assert e < 1e-4 and em < 1e-5


def test_side_stream_overlap_matches_single_stream(monkeypatch):
    """OCRL_OVERLAP=1..5 run the dVAE branch on a side stream (fork/join with events; 2 = beside the slot-attention kernels only, 3 = backward
    beside the decoder backward, 4 / 5 = forward forked at the start of the step / after the encoder convolutions; 5 is the default):
    same losses and gradients -- since every reduction has a fixed order, bit for bit"""
    cfg = O.default_cfg(**MID)
    B = 3
    P = O.formula_params(cfg)
    g = torch.Generator().manual_seed(3)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=g).cuda()
    noise = dev_noise(cfg, O.make_noise(cfg, B, 9))
    outs = []
    for flag in ("0", "1", "2", "3", "4", "5"):
        monkeypatch.setenv("OCRL_OVERLAP", flag)
        eng = make_engine(cfg, B)
        load_params(eng, P)
        for _ in range(2):          # twice: buffers reused across steps under overlap
            eng.forward(obs, 0.9, train=True, seed=5, noise=noise)
            eng.backward()
        torch.cuda.synchronize()
        outs.append((eng.metrics.cpu().clone(), eng.flat_g.cpu().clone()))
    gmax = outs[0][1].abs().max()
    for o in outs[1:]:
        assert torch.allclose(outs[0][0][:3], o[0][:3], rtol=1e-6)
        assert (outs[0][1] - o[1]).abs().max() <= 1e-5 * gmax
        assert torch.equal(outs[0][1], o[1])          # the stream a kernel runs on does not change its arithmetic


def test_execution_switches_agree(monkeypatch):
    """The other per-engine execution switches against the default build on one training-mode step (device dropout, injected noise):
    OCRL_DW_SIDE=0 / 1 (weight-gradient products on the main stream / the dVAE side stream instead of their own) must not change a bit;
    OCRL_XATTN=0 (unfused cross-attention kernels instead of the folded form) and OCRL_CONV_X3=1 (exploratory split-precision
    convolutions) are other summation orders of the same arithmetic: losses to 1e-6, every gradient to 2e-5 of the largest."""
    cfg = O.default_cfg(**MID)
    B = 3
    P = O.formula_params(cfg)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(3)).cuda()
    noise = dev_noise(cfg, O.make_noise(cfg, B, 9))

    base = {"OCRL_DW_SIDE": "2", "OCRL_XATTN": "1", "OCRL_CONV_X3": "0"}       # the default build, whatever the session's environment says

    def run(env):
        for k, v in {**base, **env}.items():
            monkeypatch.setenv(k, v)          # restored by the fixture when the test ends
        eng = make_engine(cfg, B)
        load_params(eng, P)
        for _ in range(2):
            eng.forward(obs, 0.9, train=True, seed=5, noise=noise)
            eng.backward()
        torch.cuda.synchronize()
        return eng.metrics.cpu().clone(), eng.flat_g.cpu().clone()

    m0, g0 = run({})
    gmax = g0.abs().max()
    for env, exact in (({"OCRL_DW_SIDE": "0"}, True), ({"OCRL_DW_SIDE": "1"}, True), ({"OCRL_XATTN": "0"}, False), ({"OCRL_CONV_X3": "1"}, False)):
        m, g = run(env)
        d = float((g - g0).abs().max() / gmax)
        log(f"[switch {env}] loss {float(m[2]):.6f} vs {float(m0[2]):.6f}; gradient difference {d:.2e} of the largest gradient")
        assert torch.allclose(m[:3], m0[:3], rtol=1e-6)
        if exact:
            assert torch.equal(g, g0), env
        else:
            assert 0.0 < d < 2e-5, (env, d)          # a different kernel really ran, and agrees


STREAM_MODES = [     # (OCRL_OVERLAP, OCRL_DW_SIDE, OCRL_SA_INPUT, OCRL_TOKENS_LATE or None)
    ("mid", MID, [("5", "2", "1", None), ("5", "1", "1", None), ("5", "0", "0", None), ("3", "2", "2", None), ("4", "1", "1", "1"),
                  ("2", "2", "1", None), ("1", "2", "0", None)]),       # overlap 2 keeps the weight gradients on the main stream
    ("bc32", BC32, [("0", "2", "1", None), ("3", "2", "1", None), ("5", "2", "1", None)]),    # the dVAE side's scratch is the main one's
]


@pytest.mark.parametrize("tag,over,modes", STREAM_MODES, ids=[m[0] for m in STREAM_MODES])
def test_stream_modes_keep_every_bit(tag, over, modes, monkeypatch):
    """The stream switches in combination, and under use_bcdec (the two tests above vary one switch at a time under the default of the
    others): which stream a launch goes to, and which scratch region it is handed with it, changes no bit of the losses or of the flat
    gradient against the single-stream engine (OCRL_OVERLAP=0).  OCRL_SA_INPUT is no stream switch -- the fused backward sums six
    gradients in another order -- so each combination is held against the single-stream engine with its own
    OCRL_SA_INPUT.  B = 3 leaves the image-pair grouping of the slot side a ragged group; two steps per engine, because the buffers are
    reused across steps.  OCRL_XATTN / OCRL_CONV_X3 change the summation order too and stay pinned."""
    cfg = O.default_cfg(**over)
    B = 3
    P = O.formula_params(cfg)
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(3)).cuda()
    noise = O.make_noise(cfg, B, 9)
    noise = dict(slots=noise["slots"].contiguous().cuda()) if over.get("use_bcdec") else dev_noise(cfg, noise)
    monkeypatch.setenv("OCRL_XATTN", "1")
    monkeypatch.setenv("OCRL_CONV_X3", "0")

    def run(overlap, dw, sa_in, late):
        monkeypatch.setenv("OCRL_OVERLAP", overlap)
        monkeypatch.setenv("OCRL_DW_SIDE", dw)
        monkeypatch.setenv("OCRL_SA_INPUT", sa_in)
        if late is None:
            monkeypatch.delenv("OCRL_TOKENS_LATE", raising=False)
        else:
            monkeypatch.setenv("OCRL_TOKENS_LATE", late)
        eng = make_engine(cfg, B)
        load_params(eng, P)
        for _ in range(2):
            eng.forward(obs, 0.9, train=True, seed=5, noise=noise)
            eng.backward()
        torch.cuda.synchronize()
        return eng.metrics.cpu()[:3].clone(), eng.flat_g.cpu().clone()

    single = {}        # OCRL_SA_INPUT -> the single-stream engine's result
    for mode in modes:
        sa_in = mode[2]
        if sa_in not in single:
            single[sa_in] = run("0", "2", sa_in, None)
            assert float(single[sa_in][1].abs().max()) > 0.0
        m, g = run(*mode)
        assert torch.equal(m, single[sa_in][0]), mode
        assert torch.equal(g, single[sa_in][1]), mode


def test_full_size_batch_additivity():
    """BASELINE config A shapes (128x128, 6 slots, 3 iterations, vocab 4096, 4 decoder blocks) are beyond the CPU oracle's reach in
    a test; the domain's size-independent property is additivity over images: every loss is sum/B and no operator mixes images, so
    B * (loss, gradient) of a batch equals the sum over its halves (same weights, same per-image noise, dropout off)."""
    cfg = O.default_cfg(obs_size=128, num_slots=6, num_iterations=3)
    B = 4
    P = O.formula_params(cfg)
    g = torch.Generator().manual_seed(42)
    obs = torch.rand(B, 3, 128, 128, generator=g).cuda()
    T, V, K, D = 1024, cfg.vocab_size, cfg.num_slots, cfg.slot_size
    gg = torch.Generator(device="cuda").manual_seed(7)
    noise = dict(z=torch.empty(B, T, V, device="cuda").exponential_(generator=gg), z_hard=torch.empty(B, T, V, device="cuda").exponential_(generator=gg),
                 slots=torch.randn(B, K, D, device="cuda", generator=gg))
    eng = make_engine(cfg, B)
    load_params(eng, P)

    def run(sl):
        n = {k: v[sl].contiguous() for k, v in noise.items()}
        m = eng.forward(obs[sl].contiguous(), 0.7, train=False, seed=1, noise=n)
        eng.backward()
        torch.cuda.synchronize()
        nb = obs[sl].shape[0]
        return m[:3].cpu().double() * nb, eng.flat_g.cpu().double() * nb

    l_all, g_all = run(slice(0, B))
    l_a, g_a = run(slice(0, B // 2))
    l_b, g_b = run(slice(B // 2, B))
    assert torch.isfinite(l_all).all() and torch.isfinite(g_all).all()
    err_l = ((l_a + l_b - l_all).abs() / l_all.abs().clamp_min(1e-12)).max().item()
    err_g = ((g_a + g_b - g_all).abs().max() / g_all.abs().max()).item()
    log(f"[full-size additivity] loss terms {err_l:.2e}, gradients {err_g:.2e} (|g|max {g_all.abs().max().item():.3e})")
    assert err_l < 1e-5 and err_g < 1e-4
