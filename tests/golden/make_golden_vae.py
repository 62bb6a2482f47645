"""Generate the golden vectors of the VAE module from the reference's own ``VAE_Module``.

Runs ONLY in the build container (needs /root/reference): imports ``ocrs.vaes.vae_module.VAE_Module`` with its heavy imports stubbed
(``utils.tools``, ``ocrs.base``), loads closed-form weights (``closed_form``), feeds seeded observations (``observations``) and seeded
noise (``noise``, substituted for ``torch.randn_like``), and runs ``get_loss(obs, with_rep=True)`` forward and
``loss + (rep * cotangent).sum()`` backward in fp64.  It writes tests/golden/vae.npz: per case the state_dict names and shapes,
rep_dim / num_slots, the metrics, mu, rep, recon (moments and a strided sample), and every parameter gradient (whole when it has at
most FULL_MAX entries, else moments and a strided sample).
The helpers below need neither the reference nor a GPU: the tests import them to rebuild the same inputs, and ``ref_loss`` is the
fp64 torch restatement of the reference's loss that the fixture pins.

    python tests/golden/make_golden_vae.py
"""
import contextlib
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# tag: (obs_size, batch, config)
CASES = {
    "default": (64, 2, dict(latent_dim=256, use_cnn_feat=False, cnn_feat_size=4, kld_weight=1e-4)),
    "cnnfeat_kld5": (64, 2, dict(latent_dim=256, use_cnn_feat=True, cnn_feat_size=4, kld_weight=5.0)),
    "s32": (32, 3, dict(latent_dim=32, use_cnn_feat=False, cnn_feat_size=4, kld_weight=1e-4)),
}
OBS_CHANNELS = 3
NSAMPLE = 61
FULL_MAX = 256


def fixture_path():
    return os.path.join(HERE, "vae.npz")


def config(tag, latent_dim=None, use_cnn_feat=None, cnn_feat_size=None, kld_weight=None):
    c = dict(CASES[tag][2])
    for k, v in dict(latent_dim=latent_dim, use_cnn_feat=use_cnn_feat, cnn_feat_size=cnn_feat_size, kld_weight=kld_weight).items():
        if v is not None:
            c[k] = v
    kw = c.pop("kld_weight")
    return types.SimpleNamespace(name="VAE", **c, learning=types.SimpleNamespace(lr=1e-4, kld_weight=kw))


def env_config(obs_size):
    return types.SimpleNamespace(obs_size=obs_size, obs_channels=OBS_CHANNELS)


def closed_form(shape, t):
    """tensor t of the module: a smooth pseudo-random pattern, weights scaled by 1/sqrt(fan_in) so that ReLUs stay half open"""
    n = int(np.prod(shape))
    k = torch.arange(n, dtype=torch.float64)
    v = torch.sin(k * 0.7548776662 + 1.37 * t + 0.3) + 0.35 * torch.cos(k * 0.5698402910 + 0.71 * t)
    if len(shape) >= 2:
        v = v * (1.6 / math.sqrt(int(np.prod(shape[1:]))))
    else:
        v = v * 0.05
    return v.reshape(shape)


def load_closed_form(module):
    with torch.no_grad():
        for t, (_, p) in enumerate(module.named_parameters()):
            p.copy_(closed_form(tuple(p.shape), t).to(p.dtype))


def observations(B, S, seed):
    return torch.rand(B, OBS_CHANNELS, S, S, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def noise(B, L, seed):
    return torch.randn(B, L, generator=torch.Generator().manual_seed(seed + 1000), dtype=torch.float64)


def cotangent(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 2000), dtype=torch.float64) * 0.1


def ref_loss(obs, params, eps, n, f, kld_weight, use_cnn_feat):
    """fp64 restatement of vae_module.py get_loss over a list of parameters in state_dict order; returns a dict with
    loss, mse, kld (the positive KL term), mu, logvar, rep, recon"""
    it = iter(params)
    nxt = lambda: (next(it), next(it))
    x = obs
    for _ in range(n):
        w, b = nxt(); x = F.relu(F.conv2d(x, w, b, stride=2))
        for _ in range(3):
            w, b = nxt(); x = F.relu(F.conv2d(x, w, b))
    w, b = nxt(); e = F.conv2d(x, w, b)
    B = obs.shape[0]
    flat = e.reshape(B, -1)
    wm, bm = nxt(); wv, bv = nxt(); wi, bi = nxt()
    mu, logvar = F.linear(flat, wm, bm), F.linear(flat, wv, bv)
    latent = eps * torch.exp(0.5 * logvar) + mu
    h = F.linear(latent, wi, bi).reshape(B, 64, f, f)
    w, b = nxt(); h = F.relu(F.conv2d(h, w, b))
    for _ in range(n):
        w, b = nxt(); h = F.relu(F.conv2d(h, w, b, padding=1))
        for _ in range(3):
            w, b = nxt(); h = F.relu(F.conv2d(h, w, b))
        h = F.pixel_shuffle(h, 2)
    w, b = nxt(); recon = F.conv2d(h, w, b)
    mse = ((obs - recon) ** 2).sum() / B
    kld = torch.mean(-0.5 * torch.sum(1 + logvar - mu ** 2 - logvar.exp(), dim=1), dim=0)
    rep = e.flatten(2).permute(0, 2, 1) if use_cnn_feat else mu
    return dict(loss=mse + kld_weight * kld, mse=mse, kld=kld, mu=mu, logvar=logvar, rep=rep, recon=recon)


def stages(tag):
    S, _, c = CASES[tag]
    return int(round(math.log2(S // c["cnn_feat_size"])))


def moments(a):
    a = np.asarray(a, dtype=np.float64).ravel()
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), a.max(), a.min()])


def sample_idx(n):
    return np.linspace(0, n - 1, min(n, NSAMPLE)).round().astype(np.int64)


@contextlib.contextmanager
def _reference_imports():
    """import ocrs.vaes.vae_module with utils.tools / ocrs.base stubbed (they pull wandb, omegaconf, sb3)"""
    saved = {k: sys.modules.get(k) for k in ("utils", "utils.tools", "ocrs", "ocrs.base", "ocrs.vaes", "ocrs.vaes.vae_module")}
    tools = types.ModuleType("utils.tools")
    tools.Tensor, tools.List = torch.Tensor, list
    tools.np, tools.torch = np, torch
    tools.img_to_slot = lambda x: x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])     # utils/tools.py:29
    tools.for_viz = lambda x: x
    utils = types.ModuleType("utils")
    utils.__path__ = []
    utils.tools = tools
    pkg = types.ModuleType("ocrs")
    pkg.__path__ = [os.path.join(REF, "ocrs")]
    base = types.ModuleType("ocrs.base")
    base.Base = object
    sys.modules.update({"utils": utils, "utils.tools": tools, "ocrs": pkg, "ocrs.base": base})
    sys.path.insert(0, REF)
    try:
        import importlib
        yield importlib.import_module("ocrs.vaes.vae_module")
    finally:
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def main():
    out, inventory = {}, {}
    with _reference_imports() as vm:
        for seed, (tag, (S, B, c)) in enumerate(CASES.items()):
            m = vm.VAE_Module(config(tag), env_config(S)).double()
            load_closed_form(m)
            obs, eps = observations(B, S, seed), noise(B, c["latent_dim"], seed)
            orig = torch.randn_like
            torch.randn_like = lambda t, *a, **k: eps.to(t.dtype)
            try:
                metrics, rep = m.get_loss(obs, with_rep=True)
                mu, logvar = (m._get_mu_logvar(m._enc(obs).reshape(B, -1)))
                latent = eps * torch.exp(0.5 * logvar) + mu
                recon = m._dec(m._in_dec(latent).reshape(B, 64, c["cnn_feat_size"], c["cnn_feat_size"]))
            finally:
                torch.randn_like = orig
            cot = cotangent(tuple(rep.shape), seed)
            (metrics["loss"] + (rep * cot).sum()).backward()
            inventory[tag] = dict(params=[[k, list(v.shape)] for k, v in m.state_dict().items()], rep_dim=m.rep_dim, num_slots=m.num_slots)
            p = f"{tag}/"
            out[p + "loss"] = np.array([metrics["loss"].item(), metrics["mse"].item(), metrics["kld"].item()])
            out[p + "mu"] = mu.detach().numpy()
            r = rep.detach().numpy().ravel()
            out[p + "rep_moments"], out[p + "rep_sample"] = moments(r), r[sample_idx(r.size)]
            rc = recon.detach().numpy().ravel()
            out[p + "recon_moments"], out[p + "recon_sample"] = moments(rc), rc[sample_idx(rc.size)]
            for k, prm in m.named_parameters():
                g = prm.grad.numpy().ravel()
                if g.size <= FULL_MAX:
                    out[p + "grad/" + k] = g.astype(np.float64)
                else:
                    out[p + "gradm/" + k], out[p + "grads/" + k] = moments(g), g[sample_idx(g.size)]
    out["inventory"] = np.array(json.dumps(inventory))
    np.savez_compressed(fixture_path(), **out)
    print(f"wrote {fixture_path()} ({os.path.getsize(fixture_path())} bytes)")


if __name__ == "__main__":
    main()
