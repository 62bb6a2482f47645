"""GPU checks of PPO and A2C training a SLATE / Slot-Attention encoder end to end: the algorithm leaves the encoder's parameters in the
engine's flat buffer and steps their range together with the policy, under one joint L2 clip (ocrl_flat_clip_*_l2_multi).

Everything runs at the tiny 16x16 SLATE configuration of smoke(), an MLP pooling head of width 32, 4 environments, n_steps = 4,
batch_size = 8, n_epochs = 1.  An update is graded against a composed reference: the gradient of the minibatch computed outside the
algorithm (extract_features -> the loss -> backward, with the encoder's noise counter set as train() finds it), the policy's and the
encoder's parts concatenated in fp64, and one fp64 step of tests/ppo_ref.clip_adam_l2 / tests/a2c_ref.rmsprop_tf_l2 on the
concatenation.  Bounds are those of tests/test_gpu_flat_multi.py: the norm within 1e-6 relative, dp / lr within 4 x STEP_DEV.  STEP_DEV
is the rounding of p + dp: half an ulp of p over lr, 5e-6 at |p| < 0.5 and lr = 3e-3.  The encoder's LayerNorm weights are 1, where an
ulp is four times that of 0.25 .. 0.5, so the learning rate here is LR = 1e-2: half an ulp of |p| < 2 over LR is 6e-6, again inside it."""
import json
import math
import os
import types

import pytest
import torch

from tests import a2c_ref as A
from tests import ppo_ref as P
from tests.gpu_util import log
from tests.test_gpu_ppo import STEP_DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
TINY = ["ocr.dvae.vocab_size=256", "ocr.slotattr.num_slots=6", "ocr.slotattr.num_iterations=3", "ocr.tfdec.num_dec_blocks=2", "env.obs_size=16"]
SHARED = TINY + ["num_envs=4", "env.max_steps=6", "env.rew_type=dense", "device=cuda:0"]
E, T, BATCH, LR, MAX_NORM = 4, 4, 8, 1e-2, 0.5
ENC = ("_enc.", "_enc_pos.", "_slotattn.")
CASES = [("ppo", False), ("ppo", True), ("a2c", False), ("a2c", True)]
IDS = ["ppo-slate", "ppo-slotattn", "a2c-slate", "a2c-slotattn"]


def config(algo, bcdec, *over):
    from ocrl_amd.utils.config import compose
    return compose(CFG, "train_sb3", [f"ocr={'slotattn' if bcdec else 'slate'}", "pooling=transformer", f"sb3={algo}", "sb3_acnet=mlp",
                                      "env=target-N4C4S3S1"] + SHARED + list(over))


def build(algo, bcdec, ckpt="", finetuning=False, env=None, seed=13):
    """the algorithm over OCRExtractor(SLATE module, MLP pooling) on the Target task"""
    from ocrl_amd import envs, sb3s
    c = config(algo, bcdec)
    pool = types.SimpleNamespace(name="MLP", dims=[32], acts=["relu"], ocr_checkpoint=types.SimpleNamespace(run_id="", local_file=ckpt, finetuning=finetuning))
    cfg = types.SimpleNamespace(ocr=c.ocr, env=c.env, pooling=pool, sb3_acnet=c.sb3_acnet, num_envs=E, device="cuda:0")
    env = envs.TargetEnv(c.env, E, seed=31, device="cuda") if env is None else env
    kw = dict(n_steps=T, seed=seed, device="cuda:0", learning_rate=LR, max_grad_norm=MAX_NORM, ent_coef=0.01,
              policy_kwargs=dict(config=cfg, features_extractor_class=sb3s.OCRExtractor, features_extractor_kwargs=dict(config=cfg)))
    if algo == "ppo":
        return sb3s.PPO(sb3s.CustomActorCriticPolicy, env, batch_size=BATCH, n_epochs=1, **kw)
    # normalised advantages: the raw ones of an untrained critic give a joint gradient norm of a few 1e-2 over half a million weights, and
    # an RMSprop step LR * g on a LayerNorm weight of 1.0 then lies below half an ulp (6e-8) and rounds away: "every encoder tensor moved"
    # needs a gradient of the order PPO's normalised advantages give
    return sb3s.A2C(sb3s.CustomActorCriticPolicy, env, normalize_advantage=True, **kw)


def module_of(algo):
    from ocrl_amd.ocrs.flat_module import FlatParamModule
    mods = [m for m in algo.policy.modules() if isinstance(m, FlatParamModule)]
    assert len(mods) == 1
    return mods[0]


def joint(algo, policy_flat, engine_flat):
    """the concatenation the step sees, in fp64 on the CPU: the policy's buffer, then the encoder's range of the engine's"""
    lo, n = algo._enc_range
    return torch.cat([policy_flat, engine_flat[lo:lo + n]]).detach().double().cpu()


def state_of(algo):
    """(s0, s1) of the optimiser over the concatenation; s1 is None for RMSprop"""
    if algo.ALGO == "A2C" and algo.use_rms_prop:
        return torch.cat([algo.square_avg, algo.enc_sq]).double().cpu(), None
    return torch.cat([algo.flat_m, algo.enc_m]).double().cpu(), torch.cat([algo.flat_v, algo.enc_v]).double().cpu()


def minibatch_loss(algo, mb):
    from ocrl_amd.sb3s import a2c_loss, ppo_loss
    features = algo.policy.extract_features(algo._obs(mb.observations))
    if algo.ALGO == "PPO":
        return ppo_loss(algo.policy, features, mb.actions, mb.old_log_prob, mb.advantages, mb.returns, algo.clip_range, algo.vf_coef, algo.ent_coef,
                        algo.normalize_advantage)[0]
    return a2c_loss(algo.policy, features, mb.actions, mb.advantages, mb.returns, algo.vf_coef, algo.ent_coef, algo.normalize_advantage)[0]


def fp64_step(algo, p, g, s0, s1, t):
    if s1 is None:
        return A.rmsprop_tf_l2(p, g, s0, MAX_NORM, LR, A.ALPHA, algo.rms_prop_eps)
    return P.clip_adam_l2(p, g, s0, s1, MAX_NORM, LR, t)


def check_first_update(tag, algo):
    """one rollout, then train() against the composed reference; returns nothing, asserts everything of case 2 of the module docstring"""
    mod = module_of(algo)
    eng = mod.engine
    lo, n = algo._enc_range
    algo.collect_rollouts()
    perm = torch.randperm(T * E, generator=torch.Generator().manual_seed(5))
    s0, s1 = state_of(algo)
    if s1 is None:
        assert (s0 == 1).all()
    else:
        assert (s0 == 0).all() and (s1 == 0).all()                   # the RL step's own state starts fresh, whatever the engine's holds
    p0 = joint(algo, algo.flat_p, eng.flat_p)
    all0 = {k: v.detach().clone() for k, v in algo.policy.state_dict().items()}
    eng_p0, eng_m0, eng_v0 = eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone()
    # ---- the gradient outside the algorithm, with the encoder's noise counter where train() will find it
    mb = next(algo.rollout_buffer.get(BATCH, perm)) if algo.ALGO == "PPO" else algo.rollout_buffer.flat()
    seed0 = mod._step_seed
    algo.policy.train()
    algo.flat_g.zero_()
    minibatch_loss(algo, mb).backward()
    g = joint(algo, algo.flat_g, eng.flat_g)
    assert g[:algo.flat_g.numel()].abs().max() > 0 and g[algo.flat_g.numel():].abs().max() > 0
    assert torch.equal(eng.flat_p, eng_p0) and torch.equal(joint(algo, algo.flat_p, eng.flat_p), p0)          # no step was taken
    ref = fp64_step(algo, p0, g, s0, s1, 1)
    # ---- the algorithm's own update: the first optimiser step of train() is recorded, the later ones (PPO's second minibatch) run on
    mod._step_seed = seed0
    seen = []
    step = algo._optimizer_step

    def recording_step():
        step()
        if not seen:
            seen.append((joint(algo, algo.flat_p, eng.flat_p), algo._norm.clone(), joint(algo, algo.flat_g, eng.flat_g)))
    algo._optimizer_step = recording_step
    stats = algo.train(perms=[perm]) if algo.ALGO == "PPO" else algo.train()
    del algo._optimizer_step
    p1, norm1, g1 = seen[0]
    e_g = (g1 - g).abs().max().item() / g.abs().max().item()
    e_n = abs(norm1.item() - ref.norm.item()) / ref.norm.item()
    dev = ((p1 - p0) - (ref.p - p0)).abs().max().item() / LR
    log(f"e2e {tag}: joint norm {ref.norm.item():.4f} (coef {ref.coef.item():.4f}), gradient of train() against the outside one {e_g:.2e}, "
        f"norm rel err {e_n:.2e}, dp/lr dev {dev:.2e} (bound {4 * STEP_DEV:.1e}), {stats['n_updates']} updates")
    assert e_n <= 1e-6 and dev <= 4 * STEP_DEV
    assert stats["n_updates"] == (2 if algo.ALGO == "PPO" else 1) and math.isfinite(stats["loss"])
    if algo.ALGO == "A2C":                                          # one update: the reported norm is that update's
        assert abs(stats["grad_norm"] - ref.norm.item()) <= 1e-6 * ref.norm.item()
    # ---- what moved and what did not
    named = dict(mod.named_parameters())
    for q in eng.params:
        moved = not torch.equal(named[q.name].detach(), all0["features_extractor._ocr." + q.name])
        assert moved == q.name.startswith(ENC), q.name
    outside = torch.ones(eng.flat_size, dtype=torch.bool, device=eng.device)
    outside[lo:lo + n] = False
    assert torch.equal(eng.flat_p[outside].view(torch.int32), eng_p0[outside].view(torch.int32))
    assert not torch.equal(eng.flat_p[lo:lo + n], eng_p0[lo:lo + n])
    assert torch.equal(eng.flat_m.view(torch.int32), eng_m0.view(torch.int32)) and torch.equal(eng.flat_v.view(torch.int32), eng_v0.view(torch.int32))
    assert mod.engine is eng
    assert any(not torch.equal(v, all0[k]) for k, v in algo.policy.state_dict().items() if "features_extractor._pooling" in k)
    assert not torch.equal(algo.policy.action_net.weight.detach(), all0["action_net.weight"])


# ------------------------------------------------------------------------------------------------------------ 1. construction
@pytest.mark.parametrize("algo,bcdec", CASES, ids=IDS)
def test_the_algorithm_accepts_a_trainable_slate_encoder(algo, bcdec):
    a = build(algo, bcdec)
    mod = module_of(a)
    eng = mod.engine
    assert mod.backend == "SLATE" and mod.finetune_through_slots and mod._use_bcdec == bcdec and a._encoder is mod
    assert eng.max_batch == max(E, T * E if algo == "a2c" else BATCH)
    lo, n = a._enc_range
    live = [q for q in eng.params if q.name.startswith(ENC)]
    assert lo == min(q.offset for q in live) and lo + n == max(q.offset + q.numel for q in live) and lo % 4 == 0
    assert all(q.group == 1 for q in live) and not any(lo <= q.offset < lo + n for q in eng.params if q not in live)
    # the encoder's parameters stayed views of the engine's buffer; the others became views of the algorithm's
    inside = lambda t, flat: flat.data_ptr() <= t.data_ptr() < flat.data_ptr() + 4 * flat.numel()
    enc_ids = {id(p) for p in mod.parameters()}
    for name, p in a.policy.named_parameters():
        if p.dtype != torch.float32:
            continue
        assert inside(p, eng.flat_p if id(p) in enc_ids else a.flat_p), name
        if id(p) in enc_ids:
            assert inside(p.grad, eng.flat_g), name
    assert a.flat_p.numel() == sum((p.numel() + 3) & ~3 for p in a.policy.parameters() if p.requires_grad and id(p) not in enc_ids)


def test_other_flat_modules_are_still_refused():
    from ocrl_amd import sb3s
    from ocrl_amd.ocrs.iodine import Iodine_Module
    from ocrl_amd.ocrs.slate import SLATE_Module
    from ocrl_amd.utils.config import compose
    from tests.test_gpu_acnet import _acnet_cfg
    space = lambda shape=None, n=None: types.SimpleNamespace(shape=shape, n=n)
    env = types.SimpleNamespace(num_envs=2, observation_space=space((4,)), action_space=space(n=4))
    pol = lambda: sb3s.CustomActorCriticPolicy(space((4,)), space(n=4), config=types.SimpleNamespace(sb3_acnet=_acnet_cfg("mlp")))
    ci = compose(CFG, "train_sb3", ["ocr=iodine", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "env=target-N4C4S3S1", "env.obs_size=16"])
    cs = config("ppo", False)
    for algo in (sb3s.PPO, sb3s.A2C):
        p = pol()
        p.planted = Iodine_Module(ci.ocr, ci.env)
        with pytest.raises(NotImplementedError, match="a trainable Iodine encoder behind the extractor keeps its own flat buffers"):
            algo(p, env, n_steps=4)
        p = pol()
        p.one, p.two = SLATE_Module(cs.ocr, cs.env), SLATE_Module(cs.ocr, cs.env)
        p.one.finetune_through_slots = p.two.finetune_through_slots = True
        p.one.to("cuda:0"), p.two.to("cuda:0")
        with pytest.raises(NotImplementedError, match="a trainable SLATE encoder behind the extractor keeps its own flat buffers"):
            algo(p, env, n_steps=4)
        p = pol()
        p.one = SLATE_Module(cs.ocr, cs.env)                         # its slots are detached: nothing would train it
        p.one.to("cuda:0")
        with pytest.raises(NotImplementedError, match="stepping it from"):
            algo(p, env, n_steps=4)


# ------------------------------------------------------------------------------------------------------------ 2. one update
@pytest.mark.parametrize("algo,bcdec", CASES, ids=IDS)
def test_one_update_against_the_composed_reference(algo, bcdec):
    check_first_update(f"{algo} bcdec{int(bcdec)} from scratch", build(algo, bcdec))


# ------------------------------------------------------------------------------------------------------------ 3. fine-tuning
@pytest.mark.parametrize("algo,bcdec", CASES, ids=IDS)
def test_fine_tuning_starts_the_optimiser_afresh(algo, bcdec, tmp_path):
    """a pre-training checkpoint with non-zero Adam moments: they reach the engine's flat_m / flat_v, which the RL step neither reads nor
    writes; its own state for the encoder's range starts at zero (Adam) / ones (RMSprop)"""
    from ocrl_amd import ocrs
    c = config(algo, bcdec)
    src = ocrs.SLATE(c.ocr, c.env)
    src.to("cuda:0")
    eng = src._module.engine
    gen = torch.Generator(device="cuda").manual_seed(3)
    for q in eng.params:
        eng.view(eng.flat_m, q).copy_(0.01 * torch.randn(q.shape, device="cuda", generator=gen))
        eng.view(eng.flat_v, q).copy_(1e-4 * (0.5 + torch.rand(q.shape, device="cuda", generator=gen)))
    eng.adam_step = 5
    path = str(tmp_path / "slate.pth")
    torch.save(src.save(), path)
    a = build(algo, bcdec, ckpt=path, finetuning=True)
    mod = module_of(a)
    assert torch.equal(mod.engine.flat_p, eng.flat_p) and torch.equal(mod.engine.flat_m, eng.flat_m) and torch.equal(mod.engine.flat_v, eng.flat_v)
    assert mod.engine.adam_step == 5 and mod.engine.flat_m.abs().max() > 0
    check_first_update(f"{algo} bcdec{int(bcdec)} fine-tuning", a)
    assert mod.engine.adam_step == 5


# ------------------------------------------------------------------------------------------------------------ 4. reproducibility, resume
def everything(algo):
    out = {k: v.detach().clone() for k, v in algo.policy.state_dict().items()}
    out.update({f"opt.{k}": v.clone() for k, v in algo._optimizer_state().items() if torch.is_tensor(v)})
    return out


@pytest.mark.parametrize("algo,bcdec", CASES, ids=IDS)
def test_learn_is_reproducible_and_resumes_bit_for_bit(algo, bcdec, tmp_path):
    """two rollouts of 16 steps.  The resumed run is a fresh algorithm (another seed: other initial weights, fresh optimiser state) that
    loads the file saved after the first rollout and takes over the environment where the first left it."""
    runs = []
    for _ in range(2):
        a = build(algo, bcdec)
        eng = module_of(a).engine
        a.learn(2 * T * E)
        assert module_of(a).engine is eng and a.num_timesteps == 2 * T * E
        runs.append(everything(a))
    assert runs[0].keys() == runs[1].keys() and any(k.startswith("opt.enc_") for k in runs[0])
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
        assert torch.isfinite(runs[0][k].float()).all(), k
    first = build(algo, bcdec)
    first.learn(T * E)
    path = str(tmp_path / "agent.pt")
    first.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    want = {"square_avg", "step", "enc_sq"} if algo == "a2c" else {"m", "v", "step", "enc_m", "enc_v"}
    assert set(ck["optimizer"]) == want | {"sampling_rows", "enc_step_seed"}
    fresh = build(algo, bcdec, env=first.env, seed=99)
    assert not torch.equal(fresh.flat_p, first.flat_p) and not torch.equal(module_of(fresh).engine.flat_p, module_of(first).engine.flat_p)
    assert fresh.load(path) is fresh
    fresh._last_obs, fresh._last_starts = first._last_obs, first._last_starts
    eng = module_of(fresh).engine
    fresh.learn(2 * T * E)
    assert module_of(fresh).engine is eng and fresh.num_timesteps == 2 * T * E
    got = everything(fresh)
    for k in runs[0]:
        assert torch.equal(got[k], runs[0][k]), k
    # a file without the encoder's state, or with another range, is refused before anything changes
    before = everything(fresh)
    for bad in ({k: v for k, v in ck["optimizer"].items() if not k.startswith("enc_")},
                {k: (v[:-4] if k in ("enc_m", "enc_sq") else v) for k, v in ck["optimizer"].items()}):
        torch.save({**ck, "optimizer": bad}, str(tmp_path / "bad.pt"))
        with pytest.raises(ValueError, match="encoder"):
            fresh.load(str(tmp_path / "bad.pt"))
        after = everything(fresh)
        assert all(torch.equal(after[k], before[k]) for k in before)


# ------------------------------------------------------------------------------------------------------------ 5. the entry points
@pytest.mark.parametrize("algo,ocr,over", [("ppo", "slate", ["sb3.algo_kwargs.n_steps=16", "sb3.algo_kwargs.batch_size=8"]), ("a2c", "slotattn", [])],
                         ids=["ppo-slate", "a2c-slotattn"])
def test_train_sb3_trains_the_encoder_and_test_sb3_loads_the_agent(algo, ocr, over, tmp_path):
    import test_sb3
    import train_sb3
    base = [f"ocr={ocr}", "pooling=transformer", f"sb3={algo}", "sb3_acnet=mlp", "env=target-N4C4S3S1"] + SHARED + over
    per_iter = 16 if algo == "ppo" else 4                             # a2c.yaml: n_steps 5 // 4 environments = 1
    model = train_sb3.main(base + [f"max_steps={2 * per_iter}", f"eval.freq={per_iter}", "eval.n_episodes=4", f"run_dir={tmp_path / 'run'}"])
    mod = module_of(model)
    assert model.iteration == 2 and mod.finetune_through_slots and torch.isfinite(mod.engine.flat_p).all()
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert [l["step"] for l in lines] == [per_iter, 2 * per_iter]
    for l in lines:
        for k in ("train/loss", "train/grad_norm", "eval/mean_reward", "eval/success_rate"):
            assert isinstance(l[k], (int, float)) and math.isfinite(l[k]), (k, l)
        assert l["train/grad_norm"] > 0
    agent = tmp_path / "run" / "checkpoints" / "model_latest.pth"
    assert any(k.startswith("features_extractor._ocr._enc.") for k in torch.load(str(agent), map_location="cpu", weights_only=True)["policy"])
    row = test_sb3.main(base + [f"agent_checkpoint.local_file={agent}", "n_eval_episodes=4", f"run_dir={tmp_path / 'test'}"])
    assert row["episodes"] == 4 and math.isfinite(row["mean_reward"]) and 0 <= row["success_rate"] <= 1
