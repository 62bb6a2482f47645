"""SlateEngine / IodineEngine — own the C handle, the flat parameter / gradient / Adam buffers (torch-allocated,
adopted by the library) and the workspace.  Host-side plumbing only; all arithmetic is in HIP."""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib

SITE_ZPOS = 1
SITE_BLK_BASE = 16


def _aligned_empty(nbytes, device):
    """uint8 tensor whose data_ptr is 256-byte aligned"""
    raw = torch.empty(nbytes + 512, dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + nbytes]


def param_table(L, prefix, h, with_group):
    """The parameter table a handle publishes, in the reference module's parameters() order: one
    SimpleNamespace(name, shape, offset, numel, group) per tensor.  `with_group`: ocrl_<prefix>_param_info has the `group`
    out-parameter (a model with one optimiser group has none, and every entry gets group 0)."""
    count, info = getattr(L, f"ocrl_{prefix}_param_count"), getattr(L, f"ocrl_{prefix}_param_info")
    name = ctypes.create_string_buffer(256)
    shape = (ctypes.c_int * 4)()
    nd, off, ne, grp = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
    tail = (ctypes.byref(grp),) if with_group else ()
    out = []
    for i in range(count(h)):
        _lib.check(info(h, i, name, 256, ctypes.byref(shape), ctypes.byref(nd), ctypes.byref(off), ctypes.byref(ne), *tail))
        out.append(SimpleNamespace(name=name.value.decode(), shape=tuple(shape[k] for k in range(nd.value)), offset=off.value,
                                   numel=ne.value, group=grp.value))
    return out


class Engine:
    """What the stateful handles (include/ocrl_hip.h: ocrl_slate_*, ocrl_iodine_*) have in common: the handle, its parameter
    table, the flat parameter / gradient / Adam buffers and the workspace it adopts, and views into them.  A subclass names its
    `prefix`, builds its config struct and adds its own calls."""
    prefix = None           # ocrl_<prefix>_* is this engine's part of the ABI
    has_groups = False      # the parameter table carries optimiser groups

    @staticmethod
    def config(dims, max_batch):
        """the model's config struct (_lib.*Config) for `dims`"""
        raise NotImplementedError

    def _fn(self, name):
        return getattr(self.L, f"ocrl_{self.prefix}_{name}")

    @classmethod
    def _create(cls, L, dims, max_batch):
        c, h = cls.config(dims, max_batch), ctypes.c_void_p()
        _lib.check(getattr(L, f"ocrl_{cls.prefix}_create")(ctypes.byref(c), ctypes.byref(h)))
        return h

    @classmethod
    def param_spec(cls, dims):
        """the parameter table for `dims`, read from a one-image handle (creating one needs no GPU)"""
        L = _lib.lib()
        h = cls._create(L, dims, 1)
        try:
            return param_table(L, cls.prefix, h, cls.has_groups)
        finally:
            getattr(L, f"ocrl_{cls.prefix}_destroy")(h)

    def __init__(self, dims, max_batch, device="cuda:0", with_optimizer=True):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"ocrl_amd runs on an AMD GPU only (device={device!r}); there is no CPU path")
        if not torch.cuda.is_available():
            raise RuntimeError("ocrl_amd: no GPU visible to PyTorch-ROCm")
        self.L = _lib.lib()
        self.device = dev
        self.dims = dims
        self.max_batch = int(max_batch)
        self.h = h = self._create(self.L, dims, self.max_batch)
        self.params = param_table(self.L, self.prefix, h, self.has_groups)
        self.flat_size = self._fn("flat_size")(h)
        with torch.cuda.device(dev):
            mk = lambda: _aligned_empty(self.flat_size * 4, dev).view(torch.float32).zero_()
            self.flat_p, self.flat_g = mk(), mk()
            self.flat_m, self.flat_v = (mk(), mk()) if with_optimizer else (None, None)
            self.ws_bytes = self._fn("workspace_bytes")(h)
            self.ws = _aligned_empty(self.ws_bytes, dev)
            _lib.check(self._fn("bind")(h, _lib.ptr(self.flat_p), _lib.ptr(self.flat_g), _lib.ptr(self.flat_m), _lib.ptr(self.flat_v),
                                        _lib.ptr(self.ws), self.ws_bytes))
        self.metrics = self._view(self._fn("metrics")(h), 8, torch.float32)
        self.adam_step = 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._fn("destroy")(self.h)
                self.h = None
        except Exception:
            pass

    # ---- views
    def _view(self, p, count, dtype):
        off = int(p) - self.ws.data_ptr()
        assert 0 <= off and off + count * 4 <= self.ws.numel(), "pointer outside the workspace"
        return self.ws[off:off + count * 4].view(dtype)

    def view(self, flat, p):
        return flat[p.offset:p.offset + p.numel].view(p.shape)

    def param(self, name):
        p = next(q for q in self.params if q.name == name)
        return self.view(self.flat_p, p)

    def grad(self, name):
        p = next(q for q in self.params if q.name == name)
        return self.view(self.flat_g, p)

    def tensor(self, name, shape, dtype=torch.float32):
        p, n = ctypes.c_void_p(), ctypes.c_longlong()
        _lib.check(self._fn("tensor")(self.h, name.encode(), ctypes.byref(p), ctypes.byref(n)))
        cnt = 1
        for s in shape:
            cnt *= s
        assert cnt <= n.value, (name, shape, n.value)
        return self._view(p.value, cnt, dtype).view(shape)

    @property
    def stream(self):
        return _lib.stream(self.device)

    # ---- step pieces every model has (forward and clip_adam differ in their arguments)
    def backward(self):
        _lib.check(self._fn("backward")(self.h, self.stream))

    def grad_norm(self):
        _lib.check(self._fn("grad_norm")(self.h, self.stream))
        return self.metrics[3]


class SlateEngine(Engine):
    """dims: namespace with obs_size, obs_channels, vocab_size, d_model, cnn_hidden, num_slots,
    num_iterations, slot_size, mlp_hidden, num_dec_blocks, num_dec_heads, dropout."""
    prefix = "slate"
    has_groups = True

    @staticmethod
    def config(dims, max_batch):
        return _lib.SlateConfig(dims.obs_size, dims.obs_channels, dims.vocab_size, dims.d_model, dims.cnn_hidden, dims.num_slots,
                                dims.num_iterations, dims.slot_size, dims.mlp_hidden, dims.num_dec_blocks, dims.num_dec_heads,
                                float(dims.dropout), max_batch, int(bool(getattr(dims, "use_bcdec", False))),
                                int(bool(getattr(dims, "hard", False))), int(getattr(dims, "num_slot_heads", 1)))

    def __init__(self, dims, max_batch, device="cuda:0", with_optimizer=True):
        super().__init__(dims, max_batch, device, with_optimizer)
        self.group_begin = [self.L.ocrl_slate_group_begin(self.h, g) for g in range(4)]

    def tensor(self, name, shape, dtype=torch.float32):
        if name == "z":      # the soft sample is not a by-product of the step (fused soft-max heads): written on request
            _lib.check(self.L.ocrl_slate_soft_z(self.h, self.stream))
        return super().tensor(name, shape, dtype)

    # ---- step pieces
    def forward(self, obs, tau, train, seed, noise=None):
        """obs [B,3,S,S] fp32 contiguous on device.  noise: dict(z=[B,T,V], z_hard=[B,T,V], slots=[B,K,D]) or None."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
        nz = nzh = ns = None
        if noise is not None:
            nz, nzh, ns = noise.get("z"), noise.get("z_hard"), noise.get("slots")
            for t in (nz, nzh, ns):
                assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
        self._keep = (obs, nz, nzh, ns)      # keep inputs alive until the stream has consumed them
        _lib.check(self.L.ocrl_slate_forward(self.h, _lib.ptr(obs), obs.shape[0], float(tau), int(bool(train)), int(seed),
                                             _lib.ptr(nz), _lib.ptr(nzh), _lib.ptr(ns), self.stream))
        return self.metrics

    def generate(self):
        _lib.check(self.L.ocrl_slate_generate(self.h, self.stream))

    def encode(self, obs, seed, slot_noise=None):
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
        self._keep = (obs, slot_noise)
        self.encode_generation = getattr(self, "encode_generation", 0) + 1      # which encode() the saved activations belong to
        _lib.check(self.L.ocrl_slate_encode(self.h, _lib.ptr(obs), obs.shape[0], int(seed), _lib.ptr(slot_noise), self.stream))

    def freeze_weights(self, on=True):
        """the parameters will not change: encode() keeps its derived weight images between calls"""
        _lib.check(self.L.ocrl_slate_freeze_weights(self.h, int(bool(on))))

    def encode_backward(self, dslots):
        """d loss / d slots of the last encode() -> flat_g (encoder tensors; zeros elsewhere)"""
        assert dslots.is_cuda and dslots.dtype == torch.float32 and dslots.is_contiguous()
        _lib.check(self.L.ocrl_slate_encode_backward(self.h, _lib.ptr(dslots), self.stream))

    def clip_adam(self, lrs, clip, grad_scale=1.0):
        self.adam_step += 1
        arr = (ctypes.c_float * 3)(*[float(x) for x in lrs])
        _lib.check(self.L.ocrl_slate_clip_adam(self.h, ctypes.byref(arr), float(clip if clip is not None else 0.0), self.adam_step,
                                               float(grad_scale), self.stream))

    def dropout_mask(self, site, shape):
        n = 1
        for s in shape:
            n *= s
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.check(self.L.ocrl_slate_dropout_mask(self.h, int(site), n, _lib.ptr(out), self.stream))
        return out.view(shape)


class IodineEngine(Engine):
    """dims: namespace with obs_size, obs_channels, slot_size, num_iterations, num_slots, sigma, beta, layer_norm, ref_mlp_hidden."""
    prefix = "iodine"

    @staticmethod
    def config(dims, max_batch):
        return _lib.IodineConfig(dims.obs_size, dims.obs_channels, dims.slot_size, dims.num_iterations, dims.num_slots, float(dims.sigma),
                                 float(dims.beta), int(bool(dims.layer_norm)), dims.ref_mlp_hidden, max_batch)

    def forward(self, obs, seed, noise=None):
        """obs [B,3,S,S] fp32 contiguous on device; noise: optional [I,B,K,L] N(0,1) draws."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
        assert noise is None or (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous())
        self._keep = (obs, noise)
        _lib.check(self.L.ocrl_iodine_forward(self.h, _lib.ptr(obs), obs.shape[0], int(seed), _lib.ptr(noise), self.stream))
        return self.metrics

    def clip_adam(self, lr, clip, grad_scale=1.0):
        self.adam_step += 1
        _lib.check(self.L.ocrl_iodine_clip_adam(self.h, float(lr), float(clip if clip is not None else 0.0), self.adam_step, float(grad_scale),
                                                self.stream))
