"""What DQN's three device pieces cost (ocrl_amd.sb3s.DQN; include/ocrl_hip_dqn.h), against the eager torch chains with the same
arithmetic: the default Q head (net_arch (64, 64), ReLU) on F = 128 features, 4 actions.

    act4 / act32        ms per ``DQNPolicy.act`` (``ocrl_dqn_act``: forward, coin and choice in one launch) on E = 4 and 32 feature rows;
                        the eager side is the same head as an nn.Sequential, ``torch.rand`` for the coin and the random action,
                        ``argmax`` and ``where``
    train_step          ms per ``DQN.train_step()`` at batch 32 behind a frozen SLATE extractor at 64x64 (sample, gather, the target's Q,
                        the extractor, ``dqn_loss``, backward, clip + Adam); the eager side shares the extractor and replaces the rest:
                        ``randint`` and indexing of the ring, the head as an nn.Sequential, ``smooth_l1_loss``, ``backward``,
                        ``clip_grad_norm_`` and ``torch.optim.Adam`` over the same parameters
    gather32 / gather1024  ``ocrl_replay_gather`` of B = 32 and 1024 transitions of 64x64 uint8 frames: ms per call and GB/s over the bytes
                        read and written (two frames in, two out per transition); the eager side is five torch index calls

    train_step_gt / train_step_slate   ms per ``DQN.train_step()`` at batch 32 behind the ground-truth encoder (state rows) and behind the
                        frozen SLATE extractor, for the default path and for the extensions of include/ocrl_hip_replay.h: double_q,
                        n_step = 3 and prioritized_replay each alone, and all three together (configs/sb3/dqn_per.yaml)
    per100k             ``ocrl_per_sample`` + ``ocrl_per_update`` of a batch of 32 on a store of NE = 100000 ids: ms per pair of calls
    gather_nstep32      ``ocrl_replay_gather_nstep`` of 32 transitions of 64x64 frames at n = 1 and n = 3 beside ``ocrl_replay_gather``

The parent commit's ``train_step`` for DESIGN.md §7 is this tool's ``train_step`` run from a checkout of the parent built beside this one,
the two alternating in one session.

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method); both sides are timed from Python, as the loop calls them."""
import argparse
import copy
import json
import os
import sys
import tempfile
import types

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_sb3  # noqa: E402
from ocrl_amd import ocrs  # noqa: E402
from ocrl_amd.sb3s import DQNPolicy, ReplayBuffer  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tools.bench_acnet import median_ms  # noqa: E402

F, A, B = 128, 4, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_head(policy):
    """the policy's Q head as a plain nn.Sequential holding copies of its parameters"""
    return copy.deepcopy(policy.q_net.q_net)


def bench_act(calls, out):
    space = lambda **kw: types.SimpleNamespace(**kw)
    for E in (4, 32):
        torch.manual_seed(0)
        pol = DQNPolicy(space(shape=(F,)), space(n=A)).cuda()
        pol.set_sampling(1)
        pol.exploration_rate = 0.1
        head = torch_head(pol)
        x = torch.randn(E, F, device="cuda")

        def eager():
            with torch.no_grad():
                q = head(x)
                u = torch.rand(E, 2, device="cuda")
                return torch.where(u[:, 0] < 0.1, (u[:, 1] * A).long(), q.argmax(dim=1))

        out[f"act{E}"] = dict(hip_ms=round(median_ms(lambda: pol.act(x), calls), 5), torch_ms=round(median_ms(eager, calls), 5))


def bench_train_step(calls, out):
    with tempfile.TemporaryDirectory() as tmp:
        base = ["ocr=slate", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0",
                "sb3.algo_kwargs.buffer_size=4096", f"sb3.algo_kwargs.batch_size={B}"]
        c = compose(os.path.join(ROOT, "configs"), "train_sb3", base)
        src = ocrs.SLATE(c.ocr, c.env)
        src.to("cuda:0")
        torch.save(src.save(), os.path.join(tmp, "slate.pth"))
        c = compose(os.path.join(ROOT, "configs"), "train_sb3", base + [f"pooling.ocr_checkpoint.local_file={os.path.join(tmp, 'slate.pth')}"])
        env, _, model = train_sb3.build(c)
    for _ in range(64):                                     # 256 transitions of real frames
        model.collect_step()
    buf = model.replay_buffer
    N, E = buf.n_slots, buf.n_envs
    ext = copy.deepcopy(model.target.features_extractor, {id(model.policy.features_extractor._ocr): model.policy.features_extractor._ocr})
    head, thead = torch_head(model.policy), torch_head(model.target)
    params = [p for p in list(ext.parameters()) + list(head.parameters())]
    for p in params:
        p.data = p.data.clone()
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=model.learning_rate, eps=1e-8)
    target_ext = model.target.features_extractor

    def eager():
        t = torch.randint(0, buf.pos, (B,), device="cuda")
        e = torch.randint(0, E, (B,), device="cuda")
        obs, nxt = buf.observations[t, e], buf.observations[(t + 1) % N, e]
        a, r, d = buf.actions[t, e], buf.rewards[t, e], buf.dones[t, e]
        with torch.no_grad():
            y = r + torch.where(d.bool(), torch.zeros_like(r), model.gamma * thead(target_ext(nxt.float() / 255.0)).max(dim=1).values)
        q = head(ext(obs.float() / 255.0)).gather(1, a.reshape(-1, 1)).squeeze(1)
        opt.zero_grad()
        nn.functional.smooth_l1_loss(q, y).backward()
        nn.utils.clip_grad_norm_(params, model.max_grad_norm)
        opt.step()

    out["train_step"] = dict(hip_ms=round(median_ms(model.train_step, calls), 5), torch_ms=round(median_ms(eager, calls), 5), batch=B,
                             n_floats=model.flat_p.numel())


VARIANTS = {"default": [], "double_q": ["+sb3.algo_kwargs.double_q=True"], "n_step3": ["+sb3.algo_kwargs.n_step=3"],
            "prioritized": ["+sb3.algo_kwargs.prioritized_replay=True"],
            "all": ["+sb3.algo_kwargs.double_q=True", "+sb3.algo_kwargs.n_step=3", "+sb3.algo_kwargs.prioritized_replay=True"]}


def bench_variants(calls, out):
    """train_step() of the default path and of each extension, behind the GT encoder and behind a frozen SLATE extractor"""
    with tempfile.TemporaryDirectory() as tmp:
        for ocr in ("gt", "slate"):
            base = [f"ocr={ocr}", "pooling=mlp", "sb3=dqn", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4", "device=cuda:0",
                    "sb3.algo_kwargs.buffer_size=4096", f"sb3.algo_kwargs.batch_size={B}"]
            if ocr == "slate":
                c = compose(os.path.join(ROOT, "configs"), "train_sb3", base)
                src = ocrs.SLATE(c.ocr, c.env)
                src.to("cuda:0")
                torch.save(src.save(), os.path.join(tmp, "slate.pth"))
                base.append(f"pooling.ocr_checkpoint.local_file={os.path.join(tmp, 'slate.pth')}")
            res = {}
            for name, over in VARIANTS.items():
                _, _, model = train_sb3.build(compose(os.path.join(ROOT, "configs"), "train_sb3", base + over))
                model._total_timesteps = 1 << 20
                for _ in range(64):
                    model.collect_step()
                res[name] = round(median_ms(model.train_step, calls), 5)
            out[f"train_step_{ocr}"] = res


def bench_per(calls, out):
    from ocrl_amd import _lib
    L, NE = _lib.lib(), 100000
    raw = torch.empty(L.ocrl_per_bytes(NE) // 8, device="cuda", dtype=torch.int64)
    _lib.check(L.ocrl_per_init(_lib.ptr(raw), NE, _lib.stream()))
    _lib.check(L.ocrl_per_set_range(_lib.ptr(raw), NE, 0, NE - 12, 1, _lib.stream()))
    idx, w = torch.empty(B, device="cuda", dtype=torch.int64), torch.empty(B, device="cuda")
    td = torch.rand(B, device="cuda") * 3
    state = {"u": 0}

    def pair():
        state["u"] += 1
        _lib.check(L.ocrl_per_sample(_lib.ptr(raw), NE, 7, state["u"], B, 0.4, None, _lib.ptr(idx), _lib.ptr(w), _lib.stream()))
        _lib.check(L.ocrl_per_update(_lib.ptr(raw), NE, _lib.ptr(idx), _lib.ptr(td), B, 0.6, 1e-6, _lib.stream()))

    out["per100k"] = dict(sample_update_ms=round(median_ms(pair, calls), 5), batch=B, launches=3)


def bench_gather_nstep(calls, out):
    N, E, shape = 512, 4, (3, 64, 64)
    buf = ReplayBuffer(N * E, E, shape, "cuda", torch.uint8)
    buf.observations.random_(0, 256)
    buf.actions.zero_()
    buf.rewards.normal_()
    buf.dones.zero_()
    idx = torch.randint(0, N * E, (B,), device="cuda")
    out[f"gather_nstep{B}"] = dict(gather_ms=round(median_ms(lambda: buf.gather(idx), calls), 5),
                                   n1_ms=round(median_ms(lambda: buf.gather(idx, 1, 0.99), calls), 5),
                                   n3_ms=round(median_ms(lambda: buf.gather(idx, 3, 0.99), calls), 5))


def bench_gather(calls, out):
    N, E, shape = 512, 4, (3, 64, 64)
    buf = ReplayBuffer(N * E, E, shape, "cuda", torch.uint8)
    buf.observations.random_(0, 256)
    buf.actions.zero_()
    buf.rewards.zero_()
    buf.dones.zero_()
    for n in (32, 1024):
        idx = torch.randint(0, N * E, (n,), device="cuda")

        def eager():
            t, e = idx // E, idx % E
            return buf.observations[t, e], buf.observations[(t + 1) % N, e], buf.actions[t, e], buf.rewards[t, e], buf.dones[t, e]

        ms = median_ms(lambda: buf.gather(idx), calls)
        out[f"gather{n}"] = dict(hip_ms=round(ms, 5), torch_ms=round(median_ms(eager, calls), 5), gb_per_s=round(4 * n * buf.obs_bytes / ms / 1e6, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    out = {}
    bench_act(a.calls, out)
    bench_gather(a.calls, out)
    bench_gather_nstep(a.calls, out)
    bench_per(a.calls, out)
    bench_train_step(a.calls, out)
    bench_variants(a.calls, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
