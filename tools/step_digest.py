"""sha256 digests of what a named case computes, one JSON line: two forward / backward / clip_adam steps from fixed formula parameters
(losses, the flat gradient after each step, the flat parameters at the end); with --encode three encode() calls (eager, capture and
replay under OCRL_ENCODE_GRAPH=1), encode_backward() and the encoder-only update; with --generate the generated tokens.  The case
`sa_unit` is the slot-attention unit entry points instead: every output and weight gradient at three shapes.  Two builds of
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("case", choices=sorted(SLATE_CASES) + ["iodine", "sa_unit"])
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--generate", action="store_true")
    ap.add_argument("--tag", default="", help="copied into the output line (the switch combination of the run)")
    a = ap.parse_args()
    res = iodine() if a.case == "iodine" else sa_unit() if a.case == "sa_unit" else slate(SLATE_CASES[a.case], a.encode, a.generate)
    print(json.dumps(dict(case=a.case, tag=a.tag, **res)))
