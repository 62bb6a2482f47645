"""Restatement of the NatureCNN pooling heads CNN_Linear and CNN_Transformer (reference: poolings/cnn_linear/cnn_linear_module.py,
poolings/cnn_transformer/cnn_transformer_module.py, poolings/common/naturecnn.py, utils/tools.py slot_to_img) in plain torch, in any
dtype, on the CPU: the fp64 yardstick of tests/test_gpu_pool_cnn.py, pinned to the reference by tests/golden/pooling_cnn.npz
(tests/test_pool_cnn_cpu.py).  The transformer half is oracle/pooling_oracle.py, unmodified."""
import math

import torch
import torch.nn.functional as F

from oracle import pooling_oracle as PO

STRIDES = (4, 2, 1)


def slot_to_img(tokens):
    """[B, N, D] -> [B, D, sqrt N, sqrt N]"""
    B, N, D = tokens.shape
    s = math.isqrt(N)
    assert s * s == N
    return tokens.reshape(B, s, s, D).permute(0, 3, 1, 2)


def cnn(tokens, w, rep):
    """w: conv weight / bias pairs in layer order, then the Linear's when rep; returns [B, rep] or the map as tokens [B, oh ow, 64]"""
    x = slot_to_img(tokens)
    for l in range(3):
        x = F.relu(F.conv2d(x, w[2 * l], w[2 * l + 1], stride=STRIDES[l]))
    if rep:
        return F.relu(F.linear(x.flatten(1), w[6], w[7]))
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])


def transformer_cfg(config, K):
    """pooling_oracle config of the transformer behind K CNN tokens; rows of the sin/cos table do not depend on its length"""
    c = PO.default_cfg(rep_dim=64, num_slots=K, d_model=config.d_model, nhead=config.nhead, num_layers=config.num_layers,
                       pos_emb="None" if config.pos_emb == "None" else "ape")
    return c


def forward(P, tokens, kind, config):
    """P: the module's state_dict (name -> tensor, `pe` ignored); kind "CNN_Linear" or "CNN_Transformer" """
    if kind == "CNN_Linear":
        return cnn(tokens, [P[f"_net._net.{i}.{n}"] for i in (0, 2, 4, 7) for n in ("weight", "bias")], config.rep_dim)
    t = cnn(tokens, [P[f"_cnn._net.{i}.{n}"] for i in (0, 2, 4) for n in ("weight", "bias")], 0)
    return PO.forward({k: v for k, v in P.items() if k.startswith("_trans.")}, t, transformer_cfg(config, t.shape[1]))


def loss_and_grads(P, tokens, kind, config, cot, dtype=torch.float64):
    """out, d<out, cot>/dP (by name), d<out, cot>/dtokens"""
    Q = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in P.items() if not k.endswith(".pe")}
    s = tokens.detach().cpu().to(dtype).requires_grad_(True)
    out = forward(Q, s, kind, config)
    (out * cot.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in Q.items()}, s.grad
