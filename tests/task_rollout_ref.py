"""numpy restatement of a task dataset's later frames (include/ocrl_hip_rollout.h: ocrl_task_scenes_rollout_batch): an episode walked
under the uniform random policy.  Nothing of the environment is restated here: the episode and the step are those of
tests/sprite_env_ref.py and tests/oddoneout_ref.py (``Env.step``), imported.  What this adds is the walk's own rules: which draw is which
action, that a step which ends the episode is not committed, and how the drawn step count is read.  Like those modules it draws nothing
itself: it consumes the uniforms handed to it (ocrl_sprite_env_uniforms of the episode, from draw 0 and from draw 2^19)."""
import numpy as np

from tests import oddoneout_ref as O
from tests import sprite_env_ref as R

WALK_DRAW0 = 1 << 19            # draw 2^19 + s is the action of step s; draw 2^19 - 1 the drawn step count


def below(u, m):
    """the integer in [0, m) of one uniform u = bits24 / 2^24: (bits24 * m) >> 24"""
    return (int(np.float32(u) * 16777216.0) * int(m)) >> 24


def actions(u):
    """the actions of uniforms u (draws 2^19, 2^19 + 1, ..): 0 up, 1 left, 2 down, 3 right"""
    return [below(v, 4) for v in u]


def drawn_step(u, max_step):
    """the step count of draw 2^19 - 1 in [0, max_step]"""
    return below(u, max_step + 1)


def walk(d, u_episode, u_actions):
    """the episode of descriptor d made from u_episode (draws 0, 1, ..), walked with the actions of u_actions until a step ends it or
    they run out -> (frames, L): frames[s] = the rows [hi + 1, 5] after s committed steps, s = 0 .. len(frames) - 1; L = the step
    (counted from 1) that ended the episode, None when the actions ran out first.  The ending step is not in frames: L == len(frames)."""
    mod = O if d.task == 1 else R
    env = mod.Env(mod.spec_from_desc(d), lambda k: u_episode)       # the episode after the end is made from the same uniforms and never looked at
    frames = [env.rows.copy()]
    for s, a in enumerate(actions(u_actions)):
        done = env.step(a)[1]
        if done:
            return frames, s + 1
        frames.append(env.rows.copy())
    return frames, None


def scene(frames, L, t, max_steps):
    """(rows, steps_taken) of scene t of a walked episode: the state after min(t, L - 1) steps, t clamped to [0, max_steps]"""
    t = min(max(int(t), 0), int(max_steps))
    if L is None and t >= len(frames):
        raise IndexError(f"the walk needs more than {len(frames) - 1} actions for step {t}")
    taken = t if L is None else min(t, L - 1)
    return frames[taken], taken
