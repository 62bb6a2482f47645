"""Generate the golden vectors of the Transformer pooling head over a CNN feature map (SLATE with ``use_cnn_feat``: thousands of
tokens of width channels + 3 = 67), pinning ``oracle/pooling_oracle.py`` to the reference at those shapes.

Runs ONLY in the build container (needs /root/reference; import recipe = SURVEY.md Appendix C, shared with make_golden_pooling.py):
imports the reference's ``Transformer_Module`` with rep_dim 67 and pos_emb 'ape', loads closed-form weights, runs it in eval mode on
closed-form tokens, asserts the oracle agrees and writes ``pooling_cnnfeat.npz``.  The tokens are a formula (``tokens()``, no RNG), so
the fixture stores only the outputs and strided samples of dslots and of every parameter gradient.

    python tests/golden/make_golden_pooling_long.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pooling_oracle as PO  # noqa: E402

# (tag, num_slots = tokens, num_layers, batch)
CASES = [("s257_l1", 256, 1, 2), ("s257_l2", 256, 2, 2), ("s1025_l1", 1024, 1, 1)]
REP = 67


def tokens(B, K, D):
    """closed-form feature-map tokens [B, K, D] (the values a conv feature map + raw pixels could take)"""
    i = torch.arange(B * K * D, dtype=torch.float64).reshape(B, K, D)
    return (torch.sin(0.0137 * i + 0.3) + 0.5 * torch.cos(0.00071 * i)).float()


def cotangent(B, d):
    return torch.cos(torch.arange(B * d, dtype=torch.float64) * 0.29 + 0.1).reshape(B, d).float()


def sample(t):
    t = t.double().flatten()
    return np.concatenate([np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()]), t[:: max(1, t.numel() // 509)][:509].numpy()])


def main():
    from make_golden_pooling import import_reference, ref_config
    Mod = import_reference()
    fx = {}
    for tag, K, L, B in CASES:
        cfg = PO.default_cfg(rep_dim=REP, num_slots=K, num_layers=L, pos_emb="ape")
        m = Mod(cfg.rep_dim, cfg.num_slots, ref_config(cfg))
        P = PO.formula_params(cfg)
        sd = m.state_dict()
        names = [n for n, _ in PO.param_shapes(cfg)]
        assert [k for k in sd if not k.endswith(".pe")] == names, "parameter inventory differs from the reference"
        assert tuple(sd["_trans._pos.pe"].shape) == (K + 1, 1, cfg.d_model)
        m.load_state_dict({**sd, **P})
        m.eval()
        x, cot = tokens(B, K, REP), cotangent(B, cfg.d_model)
        s = x.clone().requires_grad_(True)
        out = m(s)
        (out * cot).sum().backward()
        ref_g = {n: p.grad.clone() for n, p in m.named_parameters()}
        o_out, o_g, o_ds = PO.loss_and_grads(P, x, cfg, cot)
        err = (o_out - out.detach()).abs().max().item() / out.detach().abs().max().item()
        assert err < 2e-5, (tag, "out", err)
        gmax = max(v.abs().max().item() for v in ref_g.values())
        for n in names:
            e = (o_g[n] - ref_g[n]).abs().max().item() / max(ref_g[n].abs().max().item(), 1e-4 * gmax)
            assert e < 2e-4, (tag, n, e)
        e = (o_ds - s.grad).abs().max().item() / s.grad.abs().max().item()
        assert e < 2e-4, (tag, "dslots", e)
        print(f"[{tag}] oracle == reference (out {err:.1e})")
        fx[tag + ":cfg"] = np.array([REP, K, cfg.d_model, cfg.nhead, L, cfg.dim_feedforward, 1, B])
        fx[tag + ":out"] = out.detach().numpy()
        fx[tag + ":dslots"] = sample(s.grad)
        for n in names:
            fx[tag + ":g:" + n] = sample(ref_g[n])
    np.savez_compressed(os.path.join(HERE, "pooling_cnnfeat.npz"), **fx)


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    main()
