"""CNN_Transformer pooling (poolings/cnn_transformer/cnn_transformer.py, cnn_transformer_module.py:12-40): the three NatureCNN
convolutions over ``slot_to_img(rep)``, their ``[B, 64, oh, ow]`` map as ``[B, oh ow, 64]`` tokens, then the pooling transformer
(poolings/common/transformer.py:9-33).  The convolutions are ``ocrl_pool_cnn_fwd/_bwd`` with ``rep_dim == 0`` (the last layer writes
the token layout directly); the transformer is the ``_Transformer`` container and ``_PoolFn`` of poolings/transformer.py: 16 tokens (a
64 x 64 map) take its short path, a 128 x 128 map's 144 tokens the long one.  ``pos_emb`` "ape" and "lpe" both build the fixed sin/cos
table with ``max_len = ocr_num_slots + 1``, of which the first ``oh ow + 1`` rows are used."""
from torch import nn

from .base import Base
from .cnn_linear import _NatureCNN, run_pool_cnn
from .transformer import _PoolFn, _PositionalEncoding, _Transformer, Transformer_Module


class CNN_Transformer_Module(nn.Module):
    def __init__(self, ocr_rep_dim: int, ocr_num_slots: int, config, num_stacked_obss: int = 1) -> None:
        super().__init__()
        self.rep_dim = d_model = config.d_model
        self._cnn = _NatureCNN(ocr_rep_dim, None, use_cnn_feat=True)
        if config.pos_emb in ("ape", "lpe"):                 # both map to the fixed table (cnn_transformer_module.py:24-27)
            pos = _PositionalEncoding(ocr_num_slots + 1, d_model)
        elif config.pos_emb == "None":
            pos = None
        else:
            raise ValueError(f"unknown pos_emb {config.pos_emb!r}")
        self._trans = _Transformer(64, d_model, config.nhead, config.num_layers, pos)
        layer = self._trans._trans.layers[0]
        self._geom = (d_model, config.nhead, layer.linear1.out_features, config.num_layers)
        self._drop_p = float(layer.dropout.p)
        self._calls = 0
        self.seed = 0

    _param_list = Transformer_Module._param_list             # the transformer's parameters in ocrl_pool_transformer_* order

    def forward(self, state):
        tokens = run_pool_cnn(state, self._cnn)
        pos = None if self._trans._pos is None else self._trans._pos.pe[: tokens.shape[1] + 1, 0].contiguous()
        p = self._drop_p if self.training else 0.0
        self._calls += 1
        seed = (int(self.seed) << 32) + self._calls           # a fresh dropout pattern per call, reproducible from `seed`
        return _PoolFn.apply(tokens, pos, self._geom, p, seed, *self._param_list())


class CNN_Transformer(Base):
    def __init__(self, ocr, config, num_stacked_obss: int = 1) -> None:
        self._module = CNN_Transformer_Module(ocr.rep_dim, ocr.num_slots, config, num_stacked_obss)
        super().__init__(ocr, config)
