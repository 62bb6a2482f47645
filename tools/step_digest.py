"""sha256 digests of what a named case computes, one JSON line: two forward / backward / clip_adam steps from fixed formula parameters
(losses, the flat gradient after each step, the flat parameters at the end); with --encode three encode() calls (eager, capture and
replay under OCRL_ENCODE_GRAPH=1), encode_backward() and the encoder-only update; with --generate the generated tokens.  The case
`sa_unit` is the slot-attention unit entry points instead: every output and weight gradient at three shapes; `attn_unit` the causal
self-attention entry points: the forward and the three backward forms at four head widths, with and without dropout.  Two builds of
the library (OCRL_HIP_LIB) that issue the same launches print the same line under every OCRL_* switch: a host-side refactor is held to
that, since the suite's fixture comparisons have tolerances."""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import iodine_oracle as IO, slate_oracle as O                                   # noqa: E402
from tests import slot_attn_ref as R                                                        # noqa: E402
from tests.gpu_util import dims_from_cfg, load_params                                       # noqa: E402
from tests.test_gpu_iodine import dims as iodine_dims                                       # noqa: E402
from tests.test_gpu_slate import BC32, HEADS2, MID, SMALL, dev_noise                        # noqa: E402

SLATE_CASES = {"mid": MID, "small": SMALL, "bc32": BC32, "heads2": HEADS2}
IODINE = dict(obs_size=32, num_slots=7, num_iterations=5)       # tests/test_gpu_determinism.py's two-run size
# (B, N, K, D, H, I, heads): one group form, the uneven two-block split, two heads
SA_UNIT_CASES = [R.Case(3, 200, 5, 128, 192, 3, 1), R.Case(2, 300, 11, 192, 128, 2, 1), R.Case(2, 1024, 6, 192, 192, 3, 2)]
B = 3


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def slate(over, encode, generate):
    from ocrl_amd.engine import SlateEngine
    cfg = O.default_cfg(**over)
    eng = SlateEngine(dims_from_cfg(cfg), max_batch=B)
    load_params(eng, O.formula_params(cfg))
    S, K, D = cfg.obs_size, cfg.num_slots, cfg.slot_size
    obs = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(3)).cuda()
    out = {}
    for step in range(2):
        noise = O.make_noise(cfg, B, 9 + step)
        noise = dict(slots=noise["slots"].contiguous().cuda()) if cfg.use_bcdec else dev_noise(cfg, noise)
        eng.forward(obs, 0.9, train=True, seed=5 + step, noise=noise)
        eng.backward()
        out[f"metrics{step}"], out[f"grad{step}"] = digest(eng.metrics[:3]), digest(eng.flat_g)
        eng.clip_adam((3e-4, 1e-4, 3e-4), 0.05)
        out[f"norm{step}"] = digest(eng.metrics[3:4])
    out["params"] = digest(eng.flat_p)
    if generate:
        eng.generate()
        out["tokens"] = digest(eng.tensor("tokens", (B, (S // 4) ** 2), torch.int32))
        out["gen_mse"] = digest(eng.metrics[4:5])
    if encode:
        for i in range(3):
            eng.encode(torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(40 + i)).cuda(), seed=90 + i)
            out[f"slots{i}"], out[f"attn{i}"] = digest(eng.tensor("slots", (B, K, D))), digest(eng.tensor("attn", (B, S * S, K)))
        eng.encode_backward(torch.randn(B, K, D, generator=torch.Generator().manual_seed(8)).cuda())
        out["enc_grad"] = digest(eng.flat_g)
        eng.clip_adam((3e-4, 1e-4, 3e-4), 0.05)
        out["enc_params"] = digest(eng.flat_p)
    return out


def iodine():
    from ocrl_amd.engine import IodineEngine
    cfg = IO.default_cfg(**IODINE)
    eng = IodineEngine(iodine_dims(cfg), max_batch=B)
    load_params(eng, IO.formula_params(cfg))
    obs = torch.rand(B, 3, cfg.obs_size, cfg.obs_size, generator=torch.Generator().manual_seed(2)).cuda()
    out = {}
    for step in range(2):
        eng.forward(obs, seed=50 + step)
        eng.backward()
        out[f"grad{step}"] = digest(eng.flat_g)
        eng.clip_adam(cfg.lr, cfg.clip)
        out[f"metrics{step}"] = digest(eng.metrics[:4])
    out["params"] = digest(eng.flat_p)
    return out


def sa_unit():
    """the slot-attention unit entry points (ocrl_slot_attention_mh_fwd / _bwd) on the prepared inputs of SA_UNIT_CASES"""
    out = {}
    for c in SA_UNIT_CASES:
        assert c in R.EXISTING
        got = R.run_kernel(c, R.prepare(c).inputs)
        for k in R.TENSORS:
            out[f"{R.case_id(c)}.{k}"] = digest(got[k])
        for n in R.NAMES:
            out[f"{R.case_id(c)}.{n}"] = digest(got["grads"][n])
    return out


def attn_unit():
    """the causal self-attention entry points on q, k, v as column blocks of one packed [B, T, 3d] buffer: o and lse of
    ocrl_attention_fwd; dq, dk, dv of ocrl_attention_bwd under OCRL_ATTN_BWD=2 and =1 and of ocrl_attention_bwd_ws under =3 with a
    workspace for the whole batch and (B = 3) for two images, i.e. chunks of 2 + 1"""
    import ctypes
    from ocrl_amd import _lib
    L = _lib.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    for B_, T, h in ATTN_UNIT_SHAPES:
        for dh in (16, 32, 48, 64):
            d = dh * h
            gen = torch.Generator().manual_seed(1000 * T + dh)
            qkv = torch.randn(B_, T, 3 * d, generator=gen).cuda()
            dO = torch.randn(B_, T, d, generator=gen).cuda()
            q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
            o, lse, delta = torch.empty(B_, T, d, device="cuda"), torch.empty(B_, h, T, device="cuda"), torch.empty(B_, h, T, device="cuda")
            per_image = L.ocrl_attention_bwd_ds_floats(1, T, h)
            ds = torch.empty(B_ * per_image, device="cuda")
            for p in (0.0, 0.1):
                tag = f"B{B_}T{T}h{h}dh{dh}p{p}"
                _lib.check(L.ocrl_attention_fwd(P(q), P(k), P(v), P(o), P(lse), B_, T, d, h, 3 * d, p, 7, 16, None))
                out[f"{tag}.o"], out[f"{tag}.lse"] = digest(o), digest(lse)
                forms = [("2", None), ("1", None), ("3", B_)] + ([("3", 2)] if B_ == 3 else [])
                for form, images in forms:
                    os.environ["OCRL_ATTN_BWD"] = form
                    g = torch.full_like(qkv, float("nan"))
                    gq, gk, gv = g[..., :d], g[..., d:2 * d], g[..., 2 * d:]
                    if images is None:
                        _lib.check(L.ocrl_attention_bwd(P(q), P(k), P(v), P(o), P(lse), P(dO), P(gq), P(gk), P(gv), P(delta), B_, T, d, h, 3 * d, p, 7, 16, None))
                    else:
                        ds.fill_(float("nan"))
                        _lib.check(L.ocrl_attention_bwd_ws(P(q), P(k), P(v), P(o), P(lse), P(dO), P(gq), P(gk), P(gv), P(delta), B_, T, d, h, 3 * d, p, 7, 16,
                                                           P(ds), images * per_image, None))
                    for n, t in (("dq", gq), ("dk", gk), ("dv", gv)):
                        out[f"{tag}.bwd{form}" + (f"ws{images}" if images else "") + "." + n] = digest(t)
    os.environ.pop("OCRL_ATTN_BWD", None)
    return out


# (B, T, h): two tiles with a one-row ragged tail; three tiles, T4 != T; the one-pass form's two 128-key blocks over four query tiles
ATTN_UNIT_SHAPES = [(2, 65, 2), (3, 129, 2), (2, 200, 3)]
UNITS = {"iodine": iodine, "sa_unit": sa_unit, "attn_unit": attn_unit}

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("case", choices=sorted(SLATE_CASES) + sorted(UNITS))
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--generate", action="store_true")
    ap.add_argument("--tag", default="", help="copied into the output line (the switch combination of the run)")
    a = ap.parse_args()
    res = UNITS[a.case]() if a.case in UNITS else slate(SLATE_CASES[a.case], a.encode, a.generate)
    print(json.dumps(dict(case=a.case, tag=a.tag, **res)))
