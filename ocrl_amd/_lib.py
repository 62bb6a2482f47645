"""ctypes binding of libocrl_hip.so, derived from include/ocrl_hip.h, include/ocrl_hip_dqn.h, include/ocrl_hip_rollout.h, include/ocrl_hip_replay.h, include/ocrl_hip_c51.h, include/ocrl_hip_noisy.h, include/ocrl_hip_classifier.h, include/ocrl_hip_iodine.h, include/ocrl_hip_qr.h, include/ocrl_hip_iqn.h, include/ocrl_hip_munchausen.h, include/ocrl_hip_fqf.h, include/ocrl_hip_slate_kernels.h and include/ocrl_hip_vit_kernels.h (_abi.py reads them: the struct classes, the constants and every
entry point's argtypes / restype come from the header's own declarations).  Fails loudly when the library is not built."""
import ctypes
import os
from ctypes import c_void_p

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCRL_HIP_LIB") or os.path.join(_HERE, "libocrl_hip.so")      # OCRL_HIP_LIB: development builds
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip.h")
DQN_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_dqn.h")      # the DQN entry points: a second, self-contained header
ROLLOUT_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_rollout.h")      # the task datasets' later frames: a third one
REPLAY_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_replay.h")      # DQN's replay extensions: a fourth one
C51_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_c51.h")      # DQN's categorical head: a fifth one
NOISY_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_noisy.h")      # DQN's noisy linear layers: a sixth one
CLASSIFIER_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_classifier.h")      # the MLP classifier's step: a seventh one
IODINE_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_iodine.h")      # the IODINE / broadcast-decoder kernels one by one: an eighth one
QR_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_qr.h")      # DQN's quantile head: a ninth one
SLATE_KERNELS_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_slate_kernels.h")      # the SLATE token-path and helper kernels one by one: a tenth one
VIT_KERNELS_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_vit_kernels.h")      # the pooling-Transformer and MAE kernels one by one: an eleventh one
IQN_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_iqn.h")      # DQN's implicit quantile head: a twelfth one
MUNCHAUSEN_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_munchausen.h")      # DQN's Munchausen targets: a thirteenth one
FQF_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "ocrl_hip_fqf.h")      # DQN's fully parameterized quantile function: a fourteenth one
_lib = None

if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(HEADER_PATH) as _f:
    ABI = _abi.read(_f.read())
CONSTANTS = ABI.consts                                  # the header's `#define NAME <integer>`s
# the header's structs as ctypes classes: make a GemmDesc / ConvDesc / ConvWgradDesc / AcnetDesc with gemm_desc() / conv_desc() /
# conv_wgrad_desc() / acnet_desc(), a FlatSegment table with flat_segments(); ocrl_amd.envs fills a SpriteEnvDesc from an env config
SlateConfig, IodineConfig, GemmDesc, ConvDesc, ConvWgradDesc, XattnDesc, AcnetDesc, SpriteEnvDesc, ScenesDesc, FlatSegment = (
    ABI.structs["ocrl_" + n] for n in ("slate_config", "iodine_config", "gemm_desc", "conv_desc", "conv_wgrad_desc", "xattn_desc", "acnet_desc",
                                       "sprite_env_desc", "scenes_desc", "flat_segment"))
FLAT_MAX_SEGMENTS = CONSTANTS["OCRL_FLAT_MAX_SEGMENTS"]
if not os.path.exists(DQN_HEADER_PATH):
    raise RuntimeError(f"{DQN_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(DQN_HEADER_PATH) as _f:
    ABI_DQN = _abi.read(_f.read())                      # a table of its own: ABI stays what ocrl_hip.h declares
QnetDesc = ABI_DQN.structs["ocrl_qnet_desc"]
QNET_MAX_LAYERS = len(QnetDesc().dims)
if not os.path.exists(ROLLOUT_HEADER_PATH):
    raise RuntimeError(f"{ROLLOUT_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(ROLLOUT_HEADER_PATH) as _f:
    ABI_ROLLOUT = _abi.read(_f.read())                  # no struct of its own: the descriptor is ocrl_hip.h's SpriteEnvDesc, passed with byref()
if not os.path.exists(REPLAY_HEADER_PATH):
    raise RuntimeError(f"{REPLAY_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(REPLAY_HEADER_PATH) as _f:
    ABI_REPLAY = _abi.read(_f.read())                   # no struct of its own: the TD step's descriptor is ocrl_hip_dqn.h's QnetDesc, passed with byref()
if not os.path.exists(C51_HEADER_PATH):
    raise RuntimeError(f"{C51_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(C51_HEADER_PATH) as _f:
    ABI_C51 = _abi.read(_f.read())                      # a struct of its own: the categorical head's descriptor
C51Desc = ABI_C51.structs["ocrl_c51_desc"]
if not os.path.exists(NOISY_HEADER_PATH):
    raise RuntimeError(f"{NOISY_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(NOISY_HEADER_PATH) as _f:
    ABI_NOISY = _abi.read(_f.read())                    # a struct of its own: the layer table of the noisy layers
NoisyDesc = ABI_NOISY.structs["ocrl_noisy_desc"]
NOISY_MAX_LAYERS = len(NoisyDesc().out)
if not os.path.exists(CLASSIFIER_HEADER_PATH):
    raise RuntimeError(f"{CLASSIFIER_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(CLASSIFIER_HEADER_PATH) as _f:
    ABI_CLASSIFIER = _abi.read(_f.read())               # no struct of its own: the head's descriptor is ocrl_hip_dqn.h's QnetDesc, passed with byref()
if not os.path.exists(IODINE_HEADER_PATH):
    raise RuntimeError(f"{IODINE_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(IODINE_HEADER_PATH) as _f:
    ABI_IODINE = _abi.read(_f.read())                   # no struct: every entry takes plain pointers and integers
if not os.path.exists(QR_HEADER_PATH):
    raise RuntimeError(f"{QR_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(QR_HEADER_PATH) as _f:
    ABI_QR = _abi.read(_f.read())                       # a struct of its own: the quantile head's descriptor
QrDesc = ABI_QR.structs["ocrl_qr_desc"]
if not os.path.exists(SLATE_KERNELS_HEADER_PATH):
    raise RuntimeError(f"{SLATE_KERNELS_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(SLATE_KERNELS_HEADER_PATH) as _f:
    ABI_SLATE_KERNELS = _abi.read(_f.read())            # no struct: every entry takes plain pointers and integers
if not os.path.exists(VIT_KERNELS_HEADER_PATH):
    raise RuntimeError(f"{VIT_KERNELS_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(VIT_KERNELS_HEADER_PATH) as _f:
    ABI_VIT_KERNELS = _abi.read(_f.read())              # no struct: every entry takes plain pointers and integers
if not os.path.exists(IQN_HEADER_PATH):
    raise RuntimeError(f"{IQN_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(IQN_HEADER_PATH) as _f:
    ABI_IQN = _abi.read(_f.read())                      # a struct of its own: the implicit quantile head's descriptor
IqnDesc = ABI_IQN.structs["ocrl_iqn_desc"]
if not os.path.exists(MUNCHAUSEN_HEADER_PATH):
    raise RuntimeError(f"{MUNCHAUSEN_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(MUNCHAUSEN_HEADER_PATH) as _f:
    ABI_MUNCHAUSEN = _abi.read(_f.read())               # no struct: the one entry takes plain pointers and numbers
if not os.path.exists(FQF_HEADER_PATH):
    raise RuntimeError(f"{FQF_HEADER_PATH} is missing: ocrl_amd derives its binding of libocrl_hip.so from the header and runs from the source tree.")
with open(FQF_HEADER_PATH) as _f:
    ABI_FQF = _abi.read(_f.read())                      # a struct of its own: the implicit quantile head's descriptor, restated
FqfDesc = ABI_FQF.structs["ocrl_fqf_desc"]


def flat_segments(segs):
    """the host table ocrl_flat_clip_*_l2_multi read: one (p, g, s0, s1, n) per segment; p, g, s0, s1 are device addresses as integers
    or ptr()'s result, None for a null pointer"""
    addr = lambda a: a.value if isinstance(a, c_void_p) else a
    return (FlatSegment * len(segs))(*[FlatSegment(addr(p), addr(g), addr(s0), addr(s1), int(n)) for p, g, s0, s1, n in segs])


def acnet_desc(B, F, A, dims, acts):
    """AcnetDesc of three trunks: dims / acts = (shared, policy, value) sequences of widths / activation codes (0 none, 1 relu, 2 tanh)"""
    d = AcnetDesc(B=B, F=F, A=A)
    for t in range(3):
        if len(dims[t]) > CONSTANTS["OCRL_ACNET_MAX_LAYERS"]:
            raise ValueError(f"ocrl_amd: at most {CONSTANTS['OCRL_ACNET_MAX_LAYERS']} layers per trunk (got {len(dims[t])})")
        d.n[t] = len(dims[t])
        for l, (w, a) in enumerate(zip(dims[t], acts[t])):
            d.dims[t][l], d.acts[t][l] = int(w), int(a)
    return d


def qnet_desc(B, F, A, dims, acts):
    """QnetDesc of a Q head: dims / acts = the hidden layers' widths / activation codes (0 none, 1 relu, 2 tanh)"""
    if len(dims) > QNET_MAX_LAYERS or len(acts) != len(dims):
        raise ValueError(f"ocrl_amd: at most {QNET_MAX_LAYERS} hidden layers, one activation code each (got {len(dims)}, {len(acts)})")
    d = QnetDesc(B=B, F=F, A=A, n=len(dims))
    for l, (w, a) in enumerate(zip(dims, acts)):
        d.dims[l], d.acts[l] = int(w), int(a)
    return d


def c51_desc(B, F, A, Z, dims, acts, dueling=False):
    """C51Desc of a categorical head: Z atoms per action, dims / acts as qnet_desc takes them, dueling = the value Linear beside the advantages"""
    if len(dims) > len(C51Desc().dims) or len(acts) != len(dims):
        raise ValueError(f"ocrl_amd: at most {len(C51Desc().dims)} hidden layers, one activation code each (got {len(dims)}, {len(acts)})")
    d = C51Desc(B=B, F=F, A=A, Z=Z, n=len(dims), dueling=int(bool(dueling)))
    for l, (w, a) in enumerate(zip(dims, acts)):
        d.dims[l], d.acts[l] = int(w), int(a)
    return d


def qr_desc(B, F, A, N, dims, acts, dueling=False):
    """QrDesc of a quantile head: N quantile values per action, dims / acts as qnet_desc takes them, dueling = the value Linear beside the advantages"""
    if len(dims) > len(QrDesc().dims) or len(acts) != len(dims):
        raise ValueError(f"ocrl_amd: at most {len(QrDesc().dims)} hidden layers, one activation code each (got {len(dims)}, {len(acts)})")
    d = QrDesc(B=B, F=F, A=A, N=N, n=len(dims), dueling=int(bool(dueling)))
    for l, (w, a) in enumerate(zip(dims, acts)):
        d.dims[l], d.acts[l] = int(w), int(a)
    return d


def iqn_desc(B, F, A, N, C, dims, acts):
    """IqnDesc of an implicit quantile head: N sampled fractions per row of the call, C cosines, dims / acts as qnet_desc takes them"""
    if len(dims) > len(IqnDesc().dims) or len(acts) != len(dims):
        raise ValueError(f"ocrl_amd: at most {len(IqnDesc().dims)} hidden layers, one activation code each (got {len(dims)}, {len(acts)})")
    d = IqnDesc(B=B, F=F, A=A, N=N, C=C, n=len(dims))
    for l, (w, a) in enumerate(zip(dims, acts)):
        d.dims[l], d.acts[l] = int(w), int(a)
    return d


def fqf_desc(B, F, A, N, C, dims, acts):
    """FqfDesc of ocrl_fqf_act: the implicit quantile head's descriptor (iqn_desc) with N proposed fractions per row"""
    if len(dims) > len(FqfDesc().dims) or len(acts) != len(dims):
        raise ValueError(f"ocrl_amd: at most {len(FqfDesc().dims)} hidden layers, one activation code each (got {len(dims)}, {len(acts)})")
    d = FqfDesc(B=B, F=F, A=A, N=N, C=C, n=len(dims))
    for l, (w, a) in enumerate(zip(dims, acts)):
        d.dims[l], d.acts[l] = int(w), int(a)
    return d


def noisy_desc(layers):
    """NoisyDesc of a sequence of Linear layers: layers = (in, out) per layer"""
    layers = list(layers)
    if not 1 <= len(layers) <= NOISY_MAX_LAYERS:
        raise ValueError(f"ocrl_amd: 1 .. {NOISY_MAX_LAYERS} noisy layers (got {len(layers)})")
    d = NoisyDesc(n_layers=len(layers))
    for l, (i, o) in enumerate(layers):
        getattr(d, "in")[l], d.out[l] = int(i), int(o)
    return d


def gemm_desc(**kw):
    """GemmDesc with the defaults of GemmArgs (alpha = 1, one batch, no split, the dispatch rule) and the given fields"""
    d = GemmDesc(batch=1, batch_inner=1, splitk=1, alpha=1.0, x_scale=1.0, e_scale=1.0, force_sb=-1)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def conv_desc(**kw):
    """ConvDesc with the given fields; every other field is zero (no bias, no activation, no posmap, no mask, the forward pack, the
    throughput kernel)"""
    d = ConvDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def conv_wgrad_desc(**kw):
    """ConvWgradDesc with the given fields; every other field is zero (no bias gradient, overwrite)"""
    d = ConvWgradDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C ocrl_amd/csrc).  ocrl_amd has no CPU fallback.")
    # PyTorch-ROCm carries its own copy of the HIP runtime; it has to be the one already in the process when this library resolves its
    # libamdhip64 dependency, or the two halves talk to two runtimes (observed: "no ROCm-capable device is detected" from the library
    # when it was loaded before torch)
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for abi in (ABI, ABI_DQN, ABI_ROLLOUT, ABI_REPLAY, ABI_C51, ABI_NOISY, ABI_CLASSIFIER, ABI_IODINE, ABI_QR, ABI_IQN, ABI_MUNCHAUSEN, ABI_FQF, ABI_SLATE_KERNELS, ABI_VIT_KERNELS):
        for name, (restype, argtypes) in abi.functions.items():
            f = getattr(L, name)
            f.argtypes = argtypes
            if restype is not ctypes.c_int:     # ctypes' default
                f.restype = restype
    for name, cls in {**ABI.structs, **ABI_DQN.structs, **ABI_C51.structs, **ABI_NOISY.structs, **ABI_QR.structs, **ABI_IQN.structs, **ABI_FQF.structs}.items():        # every struct whose size the library reports
        if name + "_size" in {**ABI.functions, **ABI_DQN.functions, **ABI_C51.functions, **ABI_NOISY.functions, **ABI_QR.functions, **ABI_IQN.functions, **ABI_FQF.functions} and getattr(L, name + "_size")() != ctypes.sizeof(cls):
            raise RuntimeError(f"libocrl_hip.so: {name} is {getattr(L, name + '_size')()} bytes, this binding's {cls.__name__} {ctypes.sizeof(cls)}")
    if L.ocrl_abi_version() != CONSTANTS["OCRL_ABI_VERSION"]:
        raise RuntimeError(f"libocrl_hip.so ABI version mismatch: the library is {L.ocrl_abi_version()}, include/ocrl_hip.h {CONSTANTS['OCRL_ABI_VERSION']}")
    _lib = L
    return L


def check(rc):
    if rc:
        raise RuntimeError("ocrl_hip: " + lib().ocrl_last_error().decode())


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptrs(ts):
    """array of the device pointers of a list of tensors (a None entry stays a null pointer)"""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def stream(device=None):
    """torch's current stream on `device` (None: the current device), as the library's `void* stream` argument"""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
