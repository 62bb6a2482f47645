"""What the PPO loop (ocrl_amd.sb3s.ppo) pays per environment step and per minibatch update, against the torch chain it replaces:
configs/sb3_acnet/mlp.yaml on F = 128 features, 4 actions.

    act4 / act32   ms per ``policy.forward`` on E = 4 and E = 32 rows with the sampler inside the head's launch (``set_sampling``:
                   ocrl_acnet_act) and with the eager tail (ocrl_acnet_fwd, then log_softmax, exp, multinomial, gather)
    step           ms per optimiser step on the policy's parameters: ocrl_flat_clip_adam_l2 on the flat buffers against
                   clip_grad_norm_ + torch.optim.Adam(eps=1e-5) over the parameter list

``--encoder`` times instead what stepping a trainable SLATE encoder from PPO costs (encoder_mode below).

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method); both sides are timed from Python, as the loop calls them."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import _lib  # noqa: E402
from ocrl_amd.sb3s import CustomActorCriticPolicy  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tools.bench_acnet import median_ms  # noqa: E402

F, A = 128, 4


def encoder_mode(calls, rounds):
    """--encoder: what stepping a trainable 64x64 SLATE encoder from PPO costs.
    multi    ocrl_flat_clip_adam_l2_multi on two segments of the real sizes: the mlp.yaml policy over the Transformer pooling head, and the
             encoder range of configs/ocr/slate.yaml at 64x64
    single   ocrl_flat_clip_adam_l2 on one buffer of the summed length: the cheapest that step could be
    train    one PPO.train() of one minibatch of 32 rows (features, ppo_loss, backward, the step, one device read) with the trainable
             encoder, against the same with a frozen, pre-trained one
    multi and single alternate over `rounds` rounds of `calls` calls; each entry lists the rounds' medians."""
    import tempfile

    import train_sb3
    from ocrl_amd import ocrs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "env=target-N4C4S3S1", "device=cuda:0", "num_envs=4",
            "sb3.algo_kwargs.n_steps=32", "sb3.algo_kwargs.batch_size=32", "+sb3.algo_kwargs.n_epochs=1"]
    cfg = lambda *over: compose(os.path.join(root, "configs"), "train_sb3", base + list(over))
    _, _, live = train_sb3.build(cfg())
    n_pol, n_enc = live.flat_p.numel(), live._enc_range[1]
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream()
    bufs = lambda n: [torch.zeros(n, device="cuda").normal_() if k == 1 else torch.zeros(n, device="cuda") for k in range(4)]
    a4, b4, one = bufs(n_pol), bufs(n_enc), bufs(n_pol + n_enc)
    seg = _lib.flat_segments([(p(a4[0]), p(a4[1]), p(a4[2]), p(a4[3]), n_pol), (p(b4[0]), p(b4[1]), p(b4[2]), p(b4[3]), n_enc)])
    nws_m, nws_s = L.ocrl_flat_clip_multi_ws_floats(), L.ocrl_flat_clip_adam_ws_floats()
    ws_m, ws_s, norm = torch.empty(nws_m, device="cuda"), torch.empty(nws_s, device="cuda"), torch.empty(1, device="cuda")
    step = [0]

    def multi():
        step[0] += 1
        _lib.check(L.ocrl_flat_clip_adam_l2_multi(seg, 2, 0.5, 3e-4, 0.9, 0.999, 1e-5, step[0], p(norm), p(ws_m), nws_m, st))

    def single():
        step[0] += 1
        _lib.check(L.ocrl_flat_clip_adam_l2(p(one[0]), p(one[1]), p(one[2]), p(one[3]), n_pol + n_enc, 0.5, 3e-4, 0.9, 0.999, 1e-5, step[0], p(norm),
                                            p(ws_s), nws_s, st))

    ms = dict(multi=[], single=[])
    for _ in range(rounds):
        ms["multi"].append(round(median_ms(multi, calls), 5))
        ms["single"].append(round(median_ms(single, calls), 5))
    out = dict(policy_floats=n_pol, encoder_floats=n_enc, multi_ms=ms["multi"], single_ms=ms["single"])
    with tempfile.TemporaryDirectory() as tmp:
        src = ocrs.SLATE(cfg().ocr, cfg().env)
        src.to("cuda:0")
        path = os.path.join(tmp, "slate.pth")
        torch.save(src.save(), path)
        _, _, frozen = train_sb3.build(cfg(f"pooling.ocr_checkpoint.local_file={path}"))
    for name, model in (("train_live_ms", live), ("train_frozen_ms", frozen)):
        model.collect_rollouts()
        out[name] = [round(median_ms(model.train, max(calls // 4, 10), warm=5), 4) for _ in range(rounds)]
    print(json.dumps({"encoder": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--encoder", action="store_true", help="time the multi-segment step and a PPO minibatch with a trainable SLATE encoder")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.encoder:
        return encoder_mode(a.calls, a.rounds)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = types.SimpleNamespace(sb3_acnet=compose(os.path.join(root, "configs", "sb3_acnet"), "mlp"))
    torch.manual_seed(0)
    pol = CustomActorCriticPolicy(types.SimpleNamespace(shape=(F,)), types.SimpleNamespace(n=A), config=cfg).cuda()
    out = {}
    with torch.no_grad():
        for E in (4, 32):
            x = torch.randn(E, F, device="cuda")
            pol.set_sampling(0)
            fused = median_ms(lambda: pol(x), a.calls)
            pol.set_sampling(None)
            eager = median_ms(lambda: pol(x), a.calls)
            out[f"act{E}"] = dict(fused_ms=round(fused, 5), eager_tail_ms=round(eager, 5))
    params = list(pol.parameters())
    n = sum((p.numel() + 3) & ~3 for p in params)
    L, p = _lib.lib(), _lib.ptr
    fp, fg, fm, fv = (torch.zeros(n, device="cuda") for _ in range(4))
    fg.normal_()
    nws = L.ocrl_flat_clip_adam_ws_floats()
    ws, norm, st = torch.empty(nws, device="cuda"), torch.empty(1, device="cuda"), _lib.stream()
    step = [0]

    def hip_step():
        step[0] += 1
        _lib.check(L.ocrl_flat_clip_adam_l2(p(fp), p(fg), p(fm), p(fv), n, 0.5, 3e-4, 0.9, 0.999, 1e-5, step[0], p(norm), p(ws), nws, st))

    for q in params:
        q.grad = torch.randn_like(q)
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()

    out["step"] = dict(n_tensors=len(params), n_floats=n, hip_ms=round(median_ms(hip_step, a.calls), 5), torch_ms=round(median_ms(torch_step, a.calls), 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
