"""CPU-only checks of the PPO loop's pieces that need no GPU: the new C symbols and their argument counts, the rollout buffer's order on
CPU tensors, the restated sampler (tests/ppo_ref.py) at the edges of u, and what the PPO constructor refuses."""
import os
import re
import types

import pytest
import torch

from tests import ppo_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ocrl_acnet_act", "ocrl_acnet_act_uniforms", "ocrl_flat_clip_adam_ws_floats", "ocrl_flat_clip_adam_l2")


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_with_the_declared_argument_counts(name):
    from ocrl_amd import _lib
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ocrl_hip.h")).read(), flags=re.S)
    args = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", hdr, re.S).group(1).strip()
    want = 0 if args == "void" else len(args.split(","))
    assert hasattr(L, name)
    assert len(getattr(L, name).argtypes) == want, (name, want)


def _fill(T, E, obs_dtype=torch.float32):
    from ocrl_amd.sb3s import RolloutBuffer
    buf = RolloutBuffer(T, E, (2,), "cpu", 0.99, 0.95, obs_dtype)
    for t in range(T):
        code = torch.tensor([10 * e + t for e in range(E)])
        obs = torch.stack([code, code + 100], dim=1).to(obs_dtype)
        buf.add(obs, code, code.float(), torch.zeros(E), code.float() + 0.5, -code.float())
    return buf


def test_buffer_yields_rows_in_env_major_order():
    T, E = 3, 2
    buf = _fill(T, E)
    batches = list(buf.get(batch_size=4, perm=torch.arange(T * E)))
    assert [b.actions.numel() for b in batches] == [4, 2]                    # the last minibatch is short
    actions = torch.cat([b.actions for b in batches])
    assert actions.tolist() == [10 * e + t for e in range(E) for t in range(T)]          # flat index e * T + t
    obs = torch.cat([b.observations for b in batches])
    assert torch.equal(obs, P.flatten(buf.observations)) and torch.equal(obs[:, 0].long(), actions)
    assert torch.equal(torch.cat([b.old_values for b in batches]), actions.float() + 0.5)
    assert torch.equal(torch.cat([b.old_log_prob for b in batches]), -actions.float())


def test_buffer_yields_every_row_once_under_a_random_permutation():
    T, E = 3, 2
    buf = _fill(T, E)
    gen = torch.Generator().manual_seed(3)
    for perm in (torch.randperm(T * E, generator=gen), None):
        batches = list(buf.get(batch_size=4, perm=perm, generator=gen))
        assert len(batches) == 2 and batches[1].actions.numel() == 2
        assert sorted(torch.cat([b.actions for b in batches]).tolist()) == sorted(10 * e + t for e in range(E) for t in range(T))
    one = list(buf.get())
    assert len(one) == 1 and one[0].actions.numel() == T * E


def test_buffer_keeps_uint8_observations_and_refuses_a_partial_read():
    buf = _fill(3, 2, torch.uint8)
    assert buf.observations.dtype == torch.uint8
    assert all(b.observations.dtype == torch.uint8 for b in buf.get(4, torch.arange(6)))
    from ocrl_amd.sb3s import RolloutBuffer
    part = RolloutBuffer(3, 2, (2,), "cpu")
    part.add(torch.zeros(2, 2), torch.zeros(2), torch.zeros(2), torch.ones(2), torch.zeros(2), torch.zeros(2))
    with pytest.raises(RuntimeError):
        next(part.get(4))


def test_restated_sampler_returns_what_its_midpoints_were_built_for():
    gen = torch.Generator().manual_seed(11)
    for A in (1, 2, 4, 64):
        logits = torch.randn(9, A, generator=gen)
        mid, width = P.intervals(logits)
        assert torch.allclose(width.sum(-1), torch.ones(9, dtype=torch.float64))
        for a in range(A):
            assert torch.equal(P.sample(logits, mid[:, a]), torch.full((9,), a))


def test_restated_sampler_at_the_ends_of_the_unit_interval():
    logits = torch.tensor([[0.0, 1.0, 2.0], [float("-inf"), 0.0, 0.0], [float("-inf"), float("-inf"), 3.0], [5.0, float("-inf"), 0.0]])
    assert P.sample(logits, torch.zeros(4)).tolist() == [0, 1, 2, 0]            # u = 0: the first action of non-zero probability
    top = torch.full((4,), 1 - 2.0 ** -24)
    got = P.sample(logits, top)
    assert (got < 3).all() and got.tolist() == [2, 2, 2, 2]
    assert P.sample(torch.zeros(5, 1), top[:1].expand(5)).tolist() == [0] * 5
    assert P.argmax_lowest(torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0]])).tolist() == [1, 0]


def _env(action_space):
    return types.SimpleNamespace(num_envs=2, observation_space=types.SimpleNamespace(shape=(4,)), action_space=action_space)


def test_ppo_refuses_what_it_does_not_build():
    from ocrl_amd.sb3s import PPO, CustomActorCriticPolicy
    disc = types.SimpleNamespace(n=4)
    with pytest.raises(NotImplementedError, match="clip_range_vf"):
        PPO(CustomActorCriticPolicy, _env(disc), clip_range_vf=0.2)
    with pytest.raises(NotImplementedError, match="schedule"):
        PPO(CustomActorCriticPolicy, _env(disc), learning_rate=lambda progress: 3e-4 * progress)
    with pytest.raises(NotImplementedError, match="schedule"):
        PPO(CustomActorCriticPolicy, _env(disc), clip_range=lambda progress: 0.2)
    box = types.SimpleNamespace(shape=(3,), low=-1.0, high=1.0)
    with pytest.raises(NotImplementedError, match="Discrete action spaces only"):
        PPO(CustomActorCriticPolicy, _env(box))
