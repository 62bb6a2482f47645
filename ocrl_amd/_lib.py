"""ctypes binding of libocrl_hip.so (include/ocrl_hip.h).  Fails loudly when the library is not built."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_longlong, c_size_t, c_uint, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCRL_HIP_LIB") or os.path.join(_HERE, "libocrl_hip.so")      # OCRL_HIP_LIB: development builds
_lib = None


class SlateConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("obs_size", "obs_channels", "vocab_size", "d_model", "cnn_hidden", "num_slots",
                                      "num_iterations", "slot_size", "mlp_hidden", "num_dec_blocks", "num_dec_heads")] + \
               [("dropout", c_float), ("max_batch", c_int), ("use_bcdec", c_int), ("hard", c_int), ("num_slot_heads", c_int)]


class IodineConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("obs_size", "obs_channels", "slot_size", "num_iterations", "num_slots")] + \
               [("sigma", c_float), ("beta", c_float), ("layer_norm", c_int), ("ref_mlp_hidden", c_int), ("max_batch", c_int)]


class GemmDesc(ctypes.Structure):
    """mirror of ocrl_gemm_desc (include/ocrl_hip.h); make one with gemm_desc()"""
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p)] + \
               [(n, c_int) for n in ("M", "N", "K", "lda", "ldb", "ldc", "akc", "bkc", "batch", "batch_inner")] + \
               [(n, c_longlong) for n in ("sA", "sB", "sC", "sAi", "sBi", "sCi")] + \
               [("splitk", c_int), ("alpha", c_float), ("bias", c_void_p), ("relu", c_int),
                ("drop_p", c_float), ("drop_seed", c_ulonglong), ("drop_site", c_uint),
                ("mask", c_void_p), ("ldmask", c_int), ("sMask", c_longlong), ("mask_elu", c_int),
                ("resid", c_void_p), ("ldr", c_int), ("sR", c_longlong),
                ("adrop_p", c_float), ("adrop_site", c_uint), ("adrop_ld", c_int),
                ("bias_out", c_void_p), ("sBias", c_longlong),
                ("a_mode", c_int), ("b_mode", c_int), ("x_lse", c_void_p), ("x_tok", c_void_p), ("x_scale", c_float),
                ("epi_mode", c_int), ("stat", c_void_p), ("hstat", c_void_p), ("hidx", c_void_p), ("e1", c_void_p), ("e2", c_void_p),
                ("e_seed", c_ulonglong), ("e_lse", c_void_p), ("e_rowvec", c_void_p), ("e_scale", c_float),
                ("force_tile", c_int), ("force_sb", c_int)]


class ConvDesc(ctypes.Structure):
    """mirror of ocrl_conv_desc (include/ocrl_hip.h); make one with conv_desc()"""
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("y", c_void_p)] + \
               [(n, c_int) for n in ("B", "H", "W", "cin", "cin_pad", "ks")] + \
               [("bias", c_void_p), ("relu", c_int), ("posmap", c_void_p), ("mask", c_void_p), ("mask_elu", c_int),
                ("transposed", c_int), ("low_latency", c_int)]


class ConvWgradDesc(ctypes.Structure):
    """mirror of ocrl_conv_wgrad_desc (include/ocrl_hip.h); make one with conv_wgrad_desc()"""
    _fields_ = [("x", c_void_p), ("dy", c_void_p), ("dw", c_void_p), ("db", c_void_p)] + \
               [(n, c_int) for n in ("B", "H", "W", "cin", "cin_pad", "ks", "accumulate")]


class XattnDesc(ctypes.Structure):
    """mirror of ocrl_xattn_desc (include/ocrl_hip.h)"""
    _fields_ = [(n, c_void_p) for n in ("x", "resid", "mem", "Wq", "Wk", "Wv", "Wo", "ck", "cv", "Ab", "AbT", "Vo", "VoT", "y", "P", "gd",
                                        "Pd", "dS", "dx", "dAb", "dVo", "dck", "dcv", "dWq", "dWo", "pq", "po", "cs_ws")] + \
               [("cs_ws_floats", c_size_t)] + [(n, c_int) for n in ("B", "T", "K", "d", "h")] + \
               [("p", c_float), ("seed", c_ulonglong), ("site_p", c_uint), ("site_o", c_uint)]


class AcnetDesc(ctypes.Structure):
    """mirror of ocrl_acnet_desc (include/ocrl_hip.h); make one with acnet_desc()"""
    _fields_ = [("B", c_int), ("F", c_int), ("A", c_int), ("n", c_int * 3), ("dims", (c_int * 8) * 3), ("acts", (c_int * 8) * 3)]


class SpriteEnvDesc(ctypes.Structure):
    """mirror of ocrl_sprite_env_desc (include/ocrl_hip.h); ocrl_amd.envs fills it from an env config"""
    _fields_ = [(n, c_int) for n in ("E", "H", "lo", "hi", "mode", "rew_type", "occlusion", "max_steps", "n_colors", "n_shapes", "n_scales")] + \
               [("colors", c_int * 8), ("shapes", c_int * 8), ("scales", c_float * 8), ("target_color", c_int), ("target_shape", c_int),
                ("target_scale", c_float), ("agent_color", c_int), ("agent_shape", c_int)] + \
               [(n, c_float) for n in ("agent_scale", "agent_x", "agent_y", "step_size", "dist_agent", "dist_objs", "dist_wall")] + \
               [("task", c_int), ("obj_comp", c_int), ("unseen_mode", c_int), ("unseen_colors", c_int * 2)]


class ScenesDesc(ctypes.Structure):
    """mirror of ocrl_scenes_desc (include/ocrl_hip.h)"""
    _fields_ = [("H", c_int), ("K", c_int)]


FLAT_MAX_SEGMENTS = 8            # OCRL_FLAT_MAX_SEGMENTS


class FlatSegment(ctypes.Structure):
    """mirror of ocrl_flat_segment (include/ocrl_hip.h); make a table with flat_segments()"""
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("s0", c_void_p), ("s1", c_void_p), ("n", c_longlong)]


def flat_segments(segs):
    """the host table ocrl_flat_clip_*_l2_multi read: one (p, g, s0, s1, n) per segment; p, g, s0, s1 are device addresses as integers
    or ptr()'s result, None for a null pointer"""
    addr = lambda a: a.value if isinstance(a, c_void_p) else a
    return (FlatSegment * len(segs))(*[FlatSegment(addr(p), addr(g), addr(s0), addr(s1), int(n)) for p, g, s0, s1, n in segs])


def acnet_desc(B, F, A, dims, acts):
    """AcnetDesc of three trunks: dims / acts = (shared, policy, value) sequences of widths / activation codes (0 none, 1 relu, 2 tanh)"""
    d = AcnetDesc(B=B, F=F, A=A)
    for t in range(3):
        if len(dims[t]) > 8:
            raise ValueError(f"ocrl_amd: at most 8 layers per trunk (got {len(dims[t])})")
        d.n[t] = len(dims[t])
        for l, (w, a) in enumerate(zip(dims[t], acts[t])):
            d.dims[t][l], d.acts[t][l] = int(w), int(a)
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
    p = c_void_p
    L.ocrl_last_error.restype = c_char_p
    L.ocrl_abi_version.restype = c_int
    L.ocrl_slate_config_size.restype = c_size_t
    if L.ocrl_slate_config_size() != ctypes.sizeof(SlateConfig):
        raise RuntimeError(f"libocrl_hip.so: ocrl_slate_config is {L.ocrl_slate_config_size()} bytes, this binding's SlateConfig {ctypes.sizeof(SlateConfig)}")
    L.ocrl_slate_create.argtypes = [POINTER(SlateConfig), POINTER(p)]
    L.ocrl_slate_destroy.argtypes = [p]
    L.ocrl_slate_destroy.restype = None
    L.ocrl_slate_param_count.argtypes = [p]
    L.ocrl_slate_param_info.argtypes = [p, c_int, c_char_p, c_int, POINTER(c_int * 4), POINTER(c_int), POINTER(c_longlong),
                                        POINTER(c_longlong), POINTER(c_int)]
    L.ocrl_slate_flat_size.argtypes = [p]
    L.ocrl_slate_flat_size.restype = c_longlong
    L.ocrl_slate_group_begin.argtypes = [p, c_int]
    L.ocrl_slate_group_begin.restype = c_longlong
    L.ocrl_slate_workspace_bytes.argtypes = [p]
    L.ocrl_slate_workspace_bytes.restype = c_size_t
    L.ocrl_slate_bind.argtypes = [p, p, p, p, p, p, c_size_t]
    L.ocrl_slate_forward.argtypes = [p, p, c_int, c_float, c_int, c_ulonglong, p, p, p, p]
    L.ocrl_slate_backward.argtypes = [p, p]
    L.ocrl_slate_generate.argtypes = [p, p]
    L.ocrl_slate_encode.argtypes = [p, p, c_int, c_ulonglong, p, p]
    L.ocrl_slate_encode_backward.argtypes = [p, p, p]
    L.ocrl_slate_freeze_weights.argtypes = [p, c_int]
    L.ocrl_slate_clip_adam.argtypes = [p, POINTER(c_float * 3), c_float, c_int, c_float, p]
    L.ocrl_slate_grad_norm.argtypes = [p, p]
    L.ocrl_slate_metrics.argtypes = [p]
    L.ocrl_slate_metrics.restype = p
    L.ocrl_slate_tensor.argtypes = [p, c_char_p, POINTER(p), POINTER(c_longlong)]
    L.ocrl_slate_dropout_mask.argtypes = [p, c_uint, c_longlong, p, p]
    L.ocrl_slate_soft_z.argtypes = [p, p]
    L.ocrl_gemm.argtypes = [p, p, p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, p, c_int, p, c_int, p, c_int,
                            c_int, p, p]
    L.ocrl_gemm_desc_size.restype = c_size_t
    L.ocrl_gemm_ex.argtypes = [POINTER(GemmDesc), p, c_size_t, p]
    L.ocrl_gemm_plan.argtypes = [POINTER(GemmDesc), POINTER(c_int * 6)]
    L.ocrl_conv2d_fwd.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, p, p]
    L.ocrl_conv2d_fwd_lowlat.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, p, p]
    L.ocrl_conv2d_x3_ws_floats.restype = c_size_t
    L.ocrl_conv2d_fwd_x3.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, c_int, p, p]
    L.ocrl_conv2d_bwd_data_x3.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, p, p]
    L.ocrl_conv2d_bwd_weight_x3.argtypes = [p, p, p, c_int, c_int, c_int, c_int, p, c_size_t, p]
    L.ocrl_conv2d_bwd_data.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, p, p]
    L.ocrl_conv2d_wgrad_ws_floats.argtypes = [c_int, c_int, c_int, c_int, c_int]
    L.ocrl_conv2d_wgrad_ws_floats.restype = c_size_t
    L.ocrl_conv2d_bwd_weight.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, c_int, c_int, p, c_size_t, p]
    L.ocrl_conv_desc_size.restype = c_size_t
    L.ocrl_conv_wgrad_desc_size.restype = c_size_t
    for name, cls in (("ocrl_conv_desc", ConvDesc), ("ocrl_conv_wgrad_desc", ConvWgradDesc)):
        n = getattr(L, name + "_size")()
        if n != ctypes.sizeof(cls):
            raise RuntimeError(f"libocrl_hip.so: {name} is {n} bytes, this binding's {cls.__name__} {ctypes.sizeof(cls)}")
    L.ocrl_conv2d_ex.argtypes = [POINTER(ConvDesc), p, c_size_t, p]
    L.ocrl_conv2d_bwd_weight_ex.argtypes = [POINTER(ConvWgradDesc), p, c_size_t, p]
    L.ocrl_conv2d_first_fwd_ws_floats.restype = c_size_t
    L.ocrl_conv2d_first_fwd.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, p, c_size_t, p]
    L.ocrl_conv2d_first_wgrad_ws_floats.argtypes = [c_int, c_int, c_int]
    L.ocrl_conv2d_first_wgrad_ws_floats.restype = c_size_t
    L.ocrl_conv2d_first_bwd_weight.argtypes = [p, p, p, p, c_int, c_int, c_int, c_int, p, c_size_t, p]
    L.ocrl_layernorm_fwd.argtypes = [p, p, p, p, p, p, c_longlong, c_int, p]
    L.ocrl_layernorm_bwd.argtypes = [p, p, p, p, p, p, p, c_longlong, c_int, p, c_size_t, p]
    L.ocrl_sa_input_plan.argtypes = [c_longlong, POINTER(c_int * 3)]
    L.ocrl_sa_input_fwd.argtypes = [p] * 11 + [c_longlong, c_int, p]
    L.ocrl_sa_input_bwd.argtypes = [p] * 16 + [c_longlong, c_int, p, c_size_t, p]
    L.ocrl_attention_fwd.argtypes = [p, p, p, p, p, c_int, c_int, c_int, c_int, c_int, c_float, c_ulonglong, c_uint, p]
    L.ocrl_attention_bwd.argtypes = [p, p, p, p, p, p, p, p, p, p, c_int, c_int, c_int, c_int, c_int, c_float, c_ulonglong, c_uint, p]
    L.ocrl_attention_bwd_ds_floats.argtypes = [c_int, c_int, c_int]
    L.ocrl_attention_bwd_ds_floats.restype = c_size_t
    L.ocrl_attention_bwd_ws.argtypes = L.ocrl_attention_bwd.argtypes[:-1] + [p, c_size_t, p]
    L.ocrl_xattn_desc_size.restype = c_size_t
    if L.ocrl_xattn_desc_size() != ctypes.sizeof(XattnDesc):
        raise RuntimeError(f"libocrl_hip.so: ocrl_xattn_desc is {L.ocrl_xattn_desc_size()} bytes, this binding's XattnDesc {ctypes.sizeof(XattnDesc)}")
    L.ocrl_xattn_plan.argtypes = [c_int, c_int, c_int, POINTER(c_int * 5)]
    L.ocrl_xattn_fwd.argtypes = [POINTER(XattnDesc), p]
    L.ocrl_xattn_bwd.argtypes = [POINTER(XattnDesc), p]
    L.ocrl_cross_attn_fwd.argtypes = [p, p, p, p, p, c_int, c_int, c_int, c_int, c_int, c_float, c_ulonglong, c_uint, p]
    L.ocrl_cross_attn_bwd_ws_floats.argtypes = [c_int] * 5
    L.ocrl_cross_attn_bwd_ws_floats.restype = c_size_t
    L.ocrl_cross_attn_bwd.argtypes = [p] * 8 + [c_int] * 5 + [c_float, c_ulonglong, c_uint, p, c_size_t, p]
    L.ocrl_obs_u8_to_f32.argtypes = [p, p, c_int, c_int, c_int, c_int, p]
    L.ocrl_prof_enable.argtypes = [c_uint]
    L.ocrl_prof_collect.argtypes = [POINTER(ctypes.c_double * 8), POINTER(c_longlong * 8), c_int]
    L.ocrl_iodine_create.argtypes = [POINTER(IodineConfig), POINTER(p)]
    L.ocrl_iodine_destroy.argtypes = [p]
    L.ocrl_iodine_destroy.restype = None
    L.ocrl_iodine_param_count.argtypes = [p]
    L.ocrl_iodine_param_info.argtypes = [p, c_int, c_char_p, c_int, POINTER(c_int * 4), POINTER(c_int), POINTER(c_longlong), POINTER(c_longlong)]
    L.ocrl_iodine_flat_size.argtypes = [p]
    L.ocrl_iodine_flat_size.restype = c_longlong
    L.ocrl_iodine_workspace_bytes.argtypes = [p]
    L.ocrl_iodine_workspace_bytes.restype = c_size_t
    L.ocrl_iodine_bind.argtypes = [p, p, p, p, p, p, c_size_t]
    L.ocrl_iodine_forward.argtypes = [p, p, c_int, c_ulonglong, p, p]
    L.ocrl_iodine_backward.argtypes = [p, p]
    L.ocrl_iodine_clip_adam.argtypes = [p, c_float, c_float, c_int, c_float, p]
    L.ocrl_iodine_grad_norm.argtypes = [p, p]
    L.ocrl_iodine_metrics.argtypes = [p]
    L.ocrl_iodine_metrics.restype = p
    L.ocrl_iodine_tensor.argtypes = [p, c_char_p, POINTER(p), POINTER(c_longlong)]
    L.ocrl_slot_attention_ws_floats.argtypes = [c_int, c_int, c_int, c_int, c_int]
    L.ocrl_slot_attention_ws_floats.restype = c_size_t
    L.ocrl_slot_attention_fwd.argtypes = [p, p, POINTER(p), p, p, c_int, c_int, c_int, c_int, c_int, c_int, p, c_size_t, p]
    L.ocrl_slot_attention_bwd.argtypes = [p, p, p, p, POINTER(p), c_int, c_int, c_int, c_int, c_int, c_int, p, c_size_t, p]
    L.ocrl_slot_attention_mh_ws_floats.argtypes = [c_int] * 7
    L.ocrl_slot_attention_mh_ws_floats.restype = c_size_t
    L.ocrl_slot_attention_mh_fwd.argtypes = [p, p, POINTER(p), p, p] + [c_int] * 7 + [p, c_size_t, p]
    L.ocrl_slot_attention_mh_bwd.argtypes = [p, p, p, p, POINTER(p)] + [c_int] * 7 + [p, c_size_t, p]
    L.ocrl_slot_attention_plan.argtypes = [c_int, c_int, c_int, c_int, POINTER(c_int * 6)]
    L.ocrl_pool_transformer_ws_floats.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int]
    L.ocrl_pool_transformer_ws_floats.restype = c_size_t
    L.ocrl_pool_transformer_fwd.argtypes = [p, POINTER(p), p, p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_ulonglong, p, c_size_t, p]
    L.ocrl_pool_transformer_bwd.argtypes = [p, p, POINTER(p), p, POINTER(p), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_ulonglong, p,
                                            c_size_t, p]
    L.ocrl_pool_transformer_dropout_mask.argtypes = [c_int, c_int, c_longlong, c_float, c_ulonglong, p, p]
    L.ocrl_pool_transformer_long_ws_floats.argtypes = [c_int] * 7
    L.ocrl_pool_transformer_long_ws_floats.restype = c_size_t
    L.ocrl_pool_transformer_long_fwd.argtypes = L.ocrl_pool_transformer_fwd.argtypes
    L.ocrl_pool_transformer_long_bwd.argtypes = L.ocrl_pool_transformer_bwd.argtypes
    L.ocrl_pool_rn_ws_floats.argtypes = [c_int, c_int, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int)]
    L.ocrl_pool_rn_ws_floats.restype = c_size_t
    L.ocrl_pool_rn_fwd.argtypes = [p, POINTER(p), p, c_int, c_int, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int), p, c_size_t, p]
    L.ocrl_pool_rn_bwd.argtypes = [p, p, POINTER(p), p, POINTER(p), c_int, c_int, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int), p, c_size_t, p]
    L.ocrl_naturecnn_ws_floats.argtypes = [c_int] * 8
    L.ocrl_naturecnn_ws_floats.restype = c_size_t
    L.ocrl_naturecnn_fwd.argtypes = [p, POINTER(p), p] + [c_int] * 9 + [p, c_size_t, p]
    L.ocrl_naturecnn_bwd.argtypes = [p, p, POINTER(p), POINTER(p)] + [c_int] * 8 + [p, c_size_t, p]
    L.ocrl_pool_cnn_ws_floats.argtypes = [c_int] * 5
    L.ocrl_pool_cnn_ws_floats.restype = c_size_t
    L.ocrl_pool_cnn_fwd.argtypes = [p, POINTER(p), p] + [c_int] * 6 + [p, c_size_t, p]
    L.ocrl_pool_cnn_bwd.argtypes = [p, p, POINTER(p), p, POINTER(p)] + [c_int] * 5 + [p, c_size_t, p]
    L.ocrl_vae_ws_floats.argtypes = [c_int] * 7
    L.ocrl_vae_ws_floats.restype = c_size_t
    L.ocrl_vae_fwd.argtypes = [p, POINTER(p), p, p, p, p] + [c_int] * 6 + [c_float, c_int, p, c_size_t, p]
    L.ocrl_vae_bwd.argtypes = [p, p, POINTER(p), p, p, POINTER(p)] + [c_int] * 6 + [c_float, c_int, p, c_size_t, p]
    L.ocrl_mae_ws_floats.argtypes = [c_int] * 11
    L.ocrl_mae_ws_floats.restype = c_size_t
    L.ocrl_mae_fwd.argtypes = [p, POINTER(p), p, p, p, p, p, p] + [c_int] * 11 + [p, c_size_t, p]
    L.ocrl_mae_bwd.argtypes = [p, POINTER(p), p, p, POINTER(p)] + [c_int] * 11 + [p, c_size_t, p]
    L.ocrl_mae_rank.argtypes = [p, p, p, p, c_int, c_int, c_int, p]
    L.ocrl_probe_ws_floats.argtypes = [c_int] * 7 + [POINTER(c_int), c_int]
    L.ocrl_probe_ws_floats.restype = c_size_t
    L.ocrl_probe_fwd.argtypes = [p, POINTER(p), p, p, p, p, p] + [c_int] * 8 + [POINTER(c_int), c_float, c_int, POINTER(c_int), POINTER(c_int),
                                 POINTER(c_int), p, c_size_t, p]
    L.ocrl_probe_bwd.argtypes = [p, p, POINTER(p), POINTER(p)] + [c_int] * 7 + [POINTER(c_int), c_float, c_int, p, c_size_t, p]
    L.ocrl_probe_match_ws_floats.argtypes = [c_int, c_int]
    L.ocrl_probe_match_ws_floats.restype = c_size_t
    L.ocrl_probe_match.argtypes = [p, c_int, c_longlong, p, p, p, p, p, p] + [c_int] * 6 + [POINTER(c_int)] * 3 + [p, c_size_t, p]
    L.ocrl_ari_counts.argtypes = [p, c_longlong, c_longlong, c_longlong, c_int, p, c_longlong, c_longlong, c_longlong, c_int, c_int, c_int, c_longlong, p, p, p]
    L.ocrl_acnet_desc_size.restype = c_size_t
    if L.ocrl_acnet_desc_size() != ctypes.sizeof(AcnetDesc):
        raise RuntimeError(f"libocrl_hip.so: ocrl_acnet_desc is {L.ocrl_acnet_desc_size()} bytes, this binding's AcnetDesc {ctypes.sizeof(AcnetDesc)}")
    L.ocrl_acnet_ws_floats.argtypes = [POINTER(AcnetDesc)]
    L.ocrl_acnet_ws_floats.restype = c_size_t
    L.ocrl_acnet_fwd.argtypes = [POINTER(AcnetDesc), p, POINTER(p), p, p, p, p, c_int, p, c_size_t, p]
    L.ocrl_acnet_bwd.argtypes = [POINTER(AcnetDesc), p, POINTER(p), p, p, p, p, p, POINTER(p), p, c_size_t, p]
    L.ocrl_acnet_ppo_fwd_bwd.argtypes = [POINTER(AcnetDesc), p, POINTER(p), p, p, p, p, c_float, c_float, c_float, c_int, p, p, POINTER(p), p, c_size_t, p]
    L.ocrl_acnet_a2c_fwd_bwd.argtypes = [POINTER(AcnetDesc), p, POINTER(p), p, p, p, c_float, c_float, c_int, p, p, POINTER(p), p, c_size_t, p]
    L.ocrl_acnet_act.argtypes = [POINTER(AcnetDesc), p, POINTER(p), c_ulonglong, c_ulonglong, p, c_int, p, p, p, p, p]
    L.ocrl_acnet_act_uniforms.argtypes = [c_ulonglong, c_ulonglong, c_longlong, p, p]
    L.ocrl_flat_clip_adam_ws_floats.argtypes = []
    L.ocrl_flat_clip_adam_ws_floats.restype = c_size_t
    L.ocrl_flat_clip_adam_l2.argtypes = [p, p, p, p, c_longlong, c_float, c_float, c_float, c_float, c_float, c_int, p, p, c_size_t, p]
    L.ocrl_flat_clip_rmsprop_ws_floats.argtypes = []
    L.ocrl_flat_clip_rmsprop_ws_floats.restype = c_size_t
    L.ocrl_flat_clip_rmsprop_l2.argtypes = [p, p, p, c_longlong, c_float, c_float, c_float, c_float, p, p, c_size_t, p]
    L.ocrl_flat_clip_multi_ws_floats.argtypes = []
    L.ocrl_flat_clip_multi_ws_floats.restype = c_size_t
    L.ocrl_flat_clip_adam_l2_multi.argtypes = [POINTER(FlatSegment), c_int, c_float, c_float, c_float, c_float, c_float, c_int, p, p, c_size_t, p]
    L.ocrl_flat_clip_rmsprop_l2_multi.argtypes = [POINTER(FlatSegment), c_int, c_float, c_float, c_float, c_float, p, p, c_size_t, p]
    L.ocrl_gae.argtypes = [p, p, p, p, p, p, p, c_int, c_int, c_float, c_float, p]
    L.ocrl_sprite_env_desc_size.restype = c_size_t
    if L.ocrl_sprite_env_desc_size() != ctypes.sizeof(SpriteEnvDesc):
        raise RuntimeError(f"libocrl_hip.so: ocrl_sprite_env_desc is {L.ocrl_sprite_env_desc_size()} bytes, this binding's SpriteEnvDesc "
                           f"{ctypes.sizeof(SpriteEnvDesc)}")
    L.ocrl_sprite_env_state_floats.argtypes = [POINTER(SpriteEnvDesc)]
    L.ocrl_sprite_env_state_floats.restype = c_size_t
    L.ocrl_sprite_env_reset.argtypes = [POINTER(SpriteEnvDesc), p, c_ulonglong, p, c_longlong, p]
    L.ocrl_sprite_env_step.argtypes = [POINTER(SpriteEnvDesc), p, c_ulonglong, p, p, p, p, p, p, p]
    L.ocrl_sprite_render.argtypes = [p, c_int, c_int, c_int, c_int, p, p]
    L.ocrl_sprite_state_obs.argtypes = [p, c_int, c_int, p, p]
    L.ocrl_gt_mlp_ws_floats.argtypes = [c_int, c_int, c_int, POINTER(c_int)]
    L.ocrl_gt_mlp_ws_floats.restype = c_size_t
    L.ocrl_gt_mlp_fwd.argtypes = [p, POINTER(p), p, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), p, c_size_t, p]
    L.ocrl_gt_mlp_bwd.argtypes = [p, p, POINTER(p), p, POINTER(p), c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), p, c_size_t, p]
    L.ocrl_sprite_env_uniforms.argtypes = [c_ulonglong, c_longlong, c_int, c_longlong, c_int, c_int, p, p]
    L.ocrl_scenes_batch.argtypes = [POINTER(ScenesDesc), c_ulonglong, p, c_int, p, p, p, p, p]
    L.ocrl_scenes_uniforms.argtypes = [c_ulonglong, c_longlong, c_int, c_int, p, p]
    L.ocrl_task_scenes_batch.argtypes = [POINTER(SpriteEnvDesc), c_ulonglong, p, c_int, p, p, p, p, p, p]
    L.ocrl_comm_unique_id.argtypes = [p, c_size_t]
    L.ocrl_comm_init.argtypes = [POINTER(p), c_int, c_int, p]
    L.ocrl_comm_allreduce.argtypes = [p, p, c_longlong, p]
    L.ocrl_comm_world.argtypes = [p]
    L.ocrl_comm_destroy.argtypes = [p]
    L.ocrl_comm_destroy.restype = None
    if L.ocrl_abi_version() != 5:
        raise RuntimeError("libocrl_hip.so ABI version mismatch")
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
