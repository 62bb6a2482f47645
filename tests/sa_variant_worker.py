"""One development form of the slot-attention kernels (tests/test_gpu_slot_attention.py test_development_forms).  OCRL_SA_FWD, OCRL_SA_BWD
and OCRL_SA_GROUP are read once per process, so each setting runs in a fresh process with the knobs in its environment: set A of
tests/slot_attn_ref.py (every slot count, one head) through the same reference and grader as the default forms; the errors go to the
JSON file named on the command line and the parent asserts them.  The first HIP error (or any other exception) ends the process with a
non-zero status before a further case is started."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("OCRL_SA_FWD", "OCRL_SA_BWD", "OCRL_SA_GROUP")


def main():
    out = sys.argv[1]
    from tests import slot_attn_ref as R
    res = dict(env={k: os.environ[k] for k in KNOBS if k in os.environ}, cases=[])
    for c in R.SET_A:
        pr = R.prepare(c)
        got = R.run_kernel(c, pr.inputs)          # raises on a HIP error and on a non-finite output
        e = R.errors(c, pr.ref, got, R.cpu32(c))
        res["cases"].append(dict(case=list(c), seed=pr.seed, G=R.plan(c.K, c.D, c.H, c.heads)["G"], attn_sum=R.attn_sum_error(got["attn"])[0],
                                 errors={k: list(v) for k, v in e.items()}))
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
