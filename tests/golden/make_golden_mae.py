"""Generate tests/golden/mae_pos_embed.npz: the reference's fixed 2-D sin-cos position tables, which pin ``ocrl_amd.ocrs.mae.sincos_2d``.

Needs a checkout of the reference: its ``ocrs/mae/util/pos_embed.py`` is loaded by file path (importing the ``ocrs`` package would hit
its ``timm == 0.3.2`` assertion).  That file uses ``np.float``, which numpy no longer has, so it is set to ``float`` first.  Only the
arrays are written: ``D<dim>_g<grid>`` = get_2d_sincos_pos_embed(dim, grid, cls_token=True) as float64.

    python tests/golden/make_golden_mae.py <path to the reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((64, 4), (768, 8))      # (width, grid)


def fixture_path():
    return os.path.join(HERE, "mae_pos_embed.npz")


def key(dim, grid):
    return f"D{dim}_g{grid}"


def main(ref):
    if not hasattr(np, "float"):
        np.float = float
    spec = importlib.util.spec_from_file_location("ref_pos_embed", os.path.join(ref, "ocrs", "mae", "util", "pos_embed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {key(d, g): np.asarray(mod.get_2d_sincos_pos_embed(d, g, cls_token=True), dtype=np.float64) for d, g in CASES}
    np.savez_compressed(fixture_path(), **out)
    print("wrote", fixture_path(), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OCRL_REFERENCE", ""))
