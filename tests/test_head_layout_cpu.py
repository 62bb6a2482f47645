"""The workspace of the three heads that run on the actor-critic head's tile code (ocrl_acnet_*, ocrl_qnet_*, ocrl_c51_*), against a
formula written out here from the headers' documented parameter order.  The three share one layout on the host side
(ocrl_amd/csrc/acnet_host.h): this checks it against something other than itself.  No GPU: *_ws_floats launches nothing."""
import ctypes
import itertools

from ocrl_amd import _lib

BATCHES = (1, 16, 17, 1043)                 # one ragged tile, one full, two, and 66 tiles over the 64 slabs
FEATURES = (10, 64)
HIDDEN = ((), (64,), (64, 32))


def up64(n):
    return (n + 63) & ~63


def chain(K, hidden):
    """(parameter count, output width) of a chain of Linear layers on an input of width K: weight [N, K] and bias [N] per layer"""
    n = 0
    for N in hidden:
        n += N * K + N
        K = N
    return n, K


def ws_floats(B, trunks, n_params, stats):
    """saved layer outputs in trunk order, the slabs of partial gradients, the slabs' scalar rows and (acnet) the advantages' statistics"""
    S = min((B + 15) // 16, 64)
    total = sum(up64(B * N) for hidden in trunks for N in hidden)
    return total + up64(S * n_params) + up64(S * 8) + (up64(8) if stats else 0)


def test_the_q_head_workspace():
    L = _lib.lib()
    for B, F, hidden in itertools.product(BATCHES, FEATURES, HIDDEN):
        A = 5
        n, K = chain(F, hidden)
        n += A * K + A                                                      # the output Linear
        d = _lib.qnet_desc(B, F, A, list(hidden), [1] * len(hidden))
        assert L.ocrl_qnet_ws_floats(ctypes.byref(d)) == ws_floats(B, [hidden], n, False), (B, F, hidden)


def test_the_categorical_head_workspace():
    L = _lib.lib()
    for B, F, hidden, dueling in itertools.product(BATCHES, FEATURES, HIDDEN, (False, True)):
        A, Z = 5, 51
        n, K = chain(F, hidden)
        n += A * Z * K + A * Z                                              # the advantage Linear
        if dueling:
            n += Z * K + Z                                                  # the value Linear reads the chain's output too
        d = _lib.c51_desc(B, F, A, Z, list(hidden), [1] * len(hidden), dueling)
        assert L.ocrl_c51_ws_floats(ctypes.byref(d)) == ws_floats(B, [hidden], n, False), (B, F, hidden, dueling)


def test_the_actor_critic_head_workspace():
    L = _lib.lib()
    for B, F, A, shared, policy, value in itertools.product(BATCHES, FEATURES, (0, 5), HIDDEN, HIDDEN, HIDDEN):
        ns, Kh = chain(F, shared)
        npi, Kp = chain(Kh, policy)
        nvf, Kv = chain(Kh, value)
        n = ns + npi + nvf
        if A:
            n += A * Kp + A + Kv + 1                                        # action_net, then value_net
        trunks = (shared, policy, value)
        d = _lib.acnet_desc(B, F, A, [list(t) for t in trunks], [[2] * len(t) for t in trunks])
        assert L.ocrl_acnet_ws_floats(ctypes.byref(d)) == ws_floats(B, trunks, n, True), (B, F, A, trunks)
