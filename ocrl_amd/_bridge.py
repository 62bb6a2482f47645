"""The rules between torch and the stateless C entry points (include/ocrl_hip.h), held once for every head:

1. GPU only: a CPU input raises RuntimeError (``gpu_input``).
2. Parameters are float32 on the input's device, and of the head's shapes where it knows them (``inputs``).
3. What a backward reads again goes through ``ctx.save_for_backward``, so torch's version check raises when one of them changed in
   place; the workspace is private to the node and stays a ``ctx`` attribute.
4. Every C call runs under ``torch.cuda.device(dev)`` on ``_lib.stream(dev)``, ``dev`` the input's device (``launch``).
5. A zero workspace size is a refused shape: ValueError with the head's description of the call and the library's reason (``workspace``).
6. Cotangents are made contiguous float32, ``None`` stays ``None`` (``cotangent``); the input's gradient is allocated only when
   ``ctx.needs_input_grad[0]``.

``who`` is the head's name in its messages, e.g. "ocrl_amd.poolings.RN"."""
import ctypes

import torch

from . import _lib


def ints(v):
    """a C int array of a sequence"""
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def gpu_input(who, x):
    """rule 1: x contiguous float32"""
    if not x.is_cuda:
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU fallback)")
    return x.contiguous().float()


def inputs(who, x, params, shapes=None):
    """rules 1 and 2: (x contiguous float32, the parameters detached and contiguous), as the kernels read them"""
    if shapes is not None and (len(params) != len(shapes) or any(tuple(p.shape) != tuple(sh) for p, sh in zip(params, shapes))):
        raise ValueError(f"{who}: parameter shapes {[list(p.shape) for p in params]} are not the head's {[list(sh) for sh in shapes]}")
    x = gpu_input(who, x)
    for p in params:
        if p.dtype != torch.float32 or p.device != x.device:
            raise RuntimeError(f"{who}: parameters must be float32 on the input's device {x.device} (got {p.dtype} on {p.device})")
    return x, [p.detach().contiguous() for p in params]


def workspace(who, n, dev, call, keep=True, reason=None):
    """rule 5: n floats on dev (none with keep = False: a call that saves nothing); `call` describes the refused call, `reason` stands in
    for the library's where its size function records none"""
    if n == 0:
        raise ValueError(f"{who}: shape not supported: {call}: " + (reason or _lib.lib().ocrl_last_error().decode()))
    return torch.empty(n if keep else 0, device=dev, dtype=torch.float32)


def launch(dev, fn, *args):
    """rule 4: fn(*args, stream) on dev's current stream, with dev the current device"""
    with torch.cuda.device(dev):
        _lib.check(fn(*args, _lib.stream(dev)))


def cotangent(g):
    return None if g is None else g.contiguous().float()


# NatureCNN's unpadded conv stack as (out channels, kernel, stride): ocrs/naturecnn.py builds 3 or 4 of them, poolings/cnn_linear.py 3
NATURE_CONVS = ((32, 8, 4), (64, 4, 2), (64, 3, 1), (128, 3, 1))


def conv_map_size(size, n_convs=3):
    """the side of the map the first n_convs leave of an input of side `size` (0: it does not fit)"""
    for _, k, st in NATURE_CONVS[:n_convs]:
        size = (size - k) // st + 1 if size >= k else 0
    return size


def conv_shapes(cin, n_convs=3):
    """the (weight, bias) shapes of the first n_convs on cin input channels, in state_dict order"""
    shapes = []
    for cout, k, _ in NATURE_CONVS[:n_convs]:
        shapes += [(cout, cin, k, k), (cout,)]
        cin = cout
    return shapes
