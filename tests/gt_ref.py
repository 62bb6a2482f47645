"""Restatements the GT tests compare against; numpy, fp64 where arithmetic is involved.

``state_obs``: the reference's ``render(mode="state")`` (envs/synthetic_envs/base.py:365-394) on this project's rows, which carry ids
and the scale itself where the reference's ``_objs`` carries names and the scale.  ``gt_mlp``: the per-object MLP of GT_Module
(ocrs/gt/gt_module.py:14-27) with its gradients by formula."""
import numpy as np

STATE_SCALES = (np.float32(0.15), np.float32(0.22))          # SCALES of the reference's base.py, as the fp32 values the rows hold


def state_obs(rows):
    """rows [..., R, 5] (colour id, shape id, scale, x, y; zero rows = the reference's padding) -> the state observation, fp32"""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.zeros(rows.shape, dtype=np.float32)
    flat, o = rows.reshape(-1, 5), out.reshape(-1, 5)
    for i, r in enumerate(flat):
        if r[0] == -1:
            o[i, :3] = -1                                     # base.py:369-371: the position is not copied
            continue
        if not r.any():
            continue                                          # zero padding (base.py:383-387)
        o[i, 0], o[i, 1] = r[0], r[1]
        o[i, 2] = STATE_SCALES.index(r[2]) if r[2] in STATE_SCALES else -1     # the reference raises; the library writes -1
        o[i, 3:] = r[3:]
    return out


def gt_mlp(x, params, acts):
    """x [..., D] fp64 through params = [W_0, b_0, ..] (W [out, in]) with a ReLU after layer l when acts[l] == "relu" ->
    (outputs of every layer, pre-activations of every layer)"""
    h, hs, zs = np.asarray(x, dtype=np.float64), [], []
    for l, act in enumerate(acts):
        z = h @ np.asarray(params[2 * l], dtype=np.float64).T + np.asarray(params[2 * l + 1], dtype=np.float64)
        h = np.maximum(z, 0.0) if act == "relu" else z
        zs.append(z)
        hs.append(h)
    return hs, zs


def gt_mlp_grads(x, params, acts, dout):
    """the gradients of sum(out * dout): (dx, [dW_0, db_0, dW_1, ..]) in fp64, by formula"""
    hs, zs = gt_mlp(x, params, acts)
    D = np.asarray(x).shape[-1]
    ins = [np.asarray(x, dtype=np.float64).reshape(-1, D)] + [h.reshape(-1, h.shape[-1]) for h in hs[:-1]]
    g = np.asarray(dout, dtype=np.float64).reshape(-1, hs[-1].shape[-1])
    grads = [None] * len(params)
    for l in range(len(acts) - 1, -1, -1):
        if acts[l] == "relu":
            g = g * (zs[l].reshape(g.shape) > 0)
        grads[2 * l], grads[2 * l + 1] = g.T @ ins[l], g.sum(0)
        g = g @ np.asarray(params[2 * l], dtype=np.float64)
    return g.reshape(np.asarray(x).shape), grads
