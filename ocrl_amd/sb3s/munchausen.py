"""DQN's Munchausen targets (Vieillard, Pietquin and Geist 2020): the scaled, clipped log-policy of the action taken is added to the
reward, and the target network's values at the next observation give way to the soft value of its soft-max policy.  Restated from the
published algorithm; the GPU work is the library's (include/ocrl_hip_munchausen.h, which states every formula): ``munchausen_targets`` is
one ``ocrl_munchausen_targets`` launch in front of the unchanged ``dqn_loss`` / ``qr_loss`` / ``iqn_loss``, which take its results as
``rewards``, ``next_q`` and ``next_quantiles``.  ``DQN(munchausen=True)`` uses it (dqn.py; ``sb3=mdqn``, ``sb3=miqn``)."""
import math

import torch

from .. import _bridge, _lib
from .qhead import coerce

_WHO = "ocrl_amd.sb3s"
MAX_ACTIONS, MAX_SAMPLES = 64, 64            # actions, quantile values per action (include/ocrl_hip_munchausen.h)


def check_munchausen(who, alpha, tau, clip_lo):
    """the kernel's limits on the three numbers, as ValueErrors that name the argument ``who`` gives them"""
    names = ("alpha", "tau", "clip_lo") if who.endswith("munchausen_targets") else ("munchausen_alpha", "munchausen_tau", "munchausen_clip")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"{who}: 0 <= {names[0]} <= 1 (got {alpha})")
    if not (math.isfinite(float(tau)) and float(tau) > 0.0):
        raise ValueError(f"{who}: {names[1]} > 0 and finite (got {tau})")
    if not (math.isfinite(float(clip_lo)) and float(clip_lo) <= 0.0):
        raise ValueError(f"{who}: {names[2]} <= 0 and finite (got {clip_lo})")


def munchausen_targets(cur_q, next_q, actions, rewards, dones, alpha, tau, clip_lo, next_quantiles=None):
    """(rewards_m [B], next_v [B, n], next_m [B, n, N'] or None) of the *target* network's action values ``cur_q`` [B, n] at the
    observations and ``next_q`` [B, n] at the next observations (``next_quantiles`` [B, n, N']: its quantile values there, for the
    quantile heads).  rewards_m = rewards + alpha * clip(tau * log pi(a | cur_q), clip_lo, 0) with pi = softmax(q / tau); every column
    of ``next_v`` holds the row's soft value sum_a pi_a (next_q_a - tau log pi_a), every action's row of ``next_m`` the same mixture of
    the quantile values; both are 0 on finished rows, whose next inputs are not read.  Fresh tensors on the inputs' device; no autograd:
    targets are constants.  No CPU fallback: a CPU tensor raises."""
    who = f"{_WHO}.munchausen_targets"
    if not (cur_q.is_cuda and next_q.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU fallback)")
    if cur_q.dim() != 2 or cur_q.shape != next_q.shape:
        raise ValueError(f"{who}: cur_q and next_q are [batch, n_actions] (got {tuple(cur_q.shape)}, {tuple(next_q.shape)})")
    check_munchausen(who, alpha, tau, clip_lo)
    dev = cur_q.device
    B, A = (int(n) for n in cur_q.shape)
    f32 = torch.float32
    Np = 0
    if next_quantiles is not None:
        if next_quantiles.dim() != 3 or tuple(next_quantiles.shape[:2]) != (B, A):
            raise ValueError(f"{who}: next_quantiles is [batch, n_actions, n'] (got {tuple(next_quantiles.shape)} for a batch of {B} and {A} "
                             "actions)")
        Np = int(next_quantiles.shape[2])
    cur_q, next_q, actions, rewards, dones, next_quantiles = coerce(
        who, dev, f"a batch of {B}, {A} actions and {Np} quantile values", ("cur_q", cur_q, f32, B * A), ("next_q", next_q, f32, B * A),
        ("actions", actions, torch.int64, B), ("rewards", rewards, f32, B), ("dones", dones, torch.uint8, B),
        ("next_quantiles", next_quantiles, f32, B * A * Np))
    rewards_m = torch.empty(B, device=dev, dtype=f32)
    next_v = torch.empty(B, A, device=dev, dtype=f32)
    next_m = torch.empty(B, A, Np, device=dev, dtype=f32) if next_quantiles is not None else None
    _bridge.launch(dev, _lib.lib().ocrl_munchausen_targets, _lib.ptr(cur_q), _lib.ptr(next_q), _lib.ptr(next_quantiles), Np, _lib.ptr(actions),
                   _lib.ptr(rewards), _lib.ptr(dones), B, A, float(alpha), float(tau), float(clip_lo), _lib.ptr(rewards_m), _lib.ptr(next_v),
                   _lib.ptr(next_m))
    return rewards_m, next_v, next_m


__all__ = ["munchausen_targets"]
