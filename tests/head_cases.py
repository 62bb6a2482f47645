"""One small instance of every stateless head, for the checks that hold for all of them (tests/test_gpu_head_contract.py,
tests/test_head_contract_cpu.py): ``CASES[name]()`` returns ``(module, call, x)`` -- the nn.Module that owns the head's parameters (on the
CPU, built at a fixed seed), ``call(x)`` that runs the head's forward on ``x`` and returns the tensor to backpropagate from, and a CPU
input.  ``REFUSED[name]()`` is the same for a shape the library refuses."""
import types

import torch

from tests.golden import make_golden_probe as GP

ns = types.SimpleNamespace


def _seeded(make):
    torch.manual_seed(11)
    return make()


def _gen():
    return torch.Generator().manual_seed(12)


def rn(K=5):
    from ocrl_amd import poolings
    m = _seeded(lambda: poolings.RN_Module(67, 5, 1, ns(g_dims=[64, 64], f_dims=[64, 32])))
    return m, m, torch.randn(4, K, 67, generator=_gen())


def transformer(use_mlp1=False, K=6, nhead=4, num_layers=1):
    from ocrl_amd import poolings
    cfg = ns(d_model=64, nhead=nhead, num_layers=num_layers, pos_emb="ape", use_mlp1=use_mlp1)
    m = _seeded(lambda: poolings.Transformer_Module(64, K, cfg))
    return m, m, torch.randn(4, K, 64, generator=_gen())


def mlp():
    from ocrl_amd import poolings
    m = _seeded(lambda: poolings.MLP_Module(64, 6, ns(dims=[64, 32], acts=["relu", "relu"])))
    return m, m, torch.randn(4, 6, 64, generator=_gen())


def cnn_linear(rep_dim=32):
    from ocrl_amd import poolings
    m = _seeded(lambda: poolings.CNN_Linear_Module(3, 4096, ns(rep_dim=rep_dim)))
    return m, m, torch.rand(2, 4096, 3, generator=_gen())


def naturecnn(rep_dim=32):
    from ocrl_amd import ocrs
    m = _seeded(lambda: ocrs.NatureCNN_Module(ns(rep_dim=rep_dim, use_cnn_feat=False, cnn_feat_size=4), ns(obs_size=64, obs_channels=3)))
    return m, m, torch.rand(2, 3, 64, 64, generator=_gen())


def vae(latent_dim=32, loss=True):
    from ocrl_amd import ocrs
    cfg = ns(name="VAE", latent_dim=latent_dim, use_cnn_feat=False, cnn_feat_size=4, learning=ns(lr=1e-4, kld_weight=1e-4))
    m = _seeded(lambda: ocrs.VAE_Module(cfg, ns(obs_size=16, obs_channels=3)))
    eps = torch.randn(2, latent_dim, generator=_gen())
    return m, (lambda x: m.loss_terms(x, eps.to(x.device))[0]) if loss else m, torch.rand(2, 3, 16, 16, generator=_gen())


def _acnet_cfg(width=64):
    return ns(ortho_init=False, shared_net=ns(dims=[64, width], acts=["relu", "relu"]), policy_net=ns(dims=[64], acts=["tanh"]),
              value_net=ns(dims=[64], acts=["tanh"]))


def custom_network(width=64):
    from ocrl_amd.sb3s import CustomNetwork
    m = _seeded(lambda: CustomNetwork(24, _acnet_cfg(width)))
    return m, lambda x: torch.cat(m(x), 1), torch.randn(4, 24, generator=_gen())


def _policy(width):
    from ocrl_amd.sb3s import CustomActorCriticPolicy
    return _seeded(lambda: CustomActorCriticPolicy(None, ns(n=4), config=ns(sb3_acnet=_acnet_cfg(width)), features_extractor=ns(features_dim=24)))


def logits_values(width=64):
    pol = _policy(width)

    def call(x):
        logits, values = pol.logits_values(x)
        return logits.sum() + values.sum()
    return pol, call, torch.randn(4, 24, generator=_gen())


def ppo_loss(width=64):
    from ocrl_amd.sb3s import ppo_loss as loss
    pol, g = _policy(width), _gen()
    x = torch.randn(4, 24, generator=g)
    actions, old, adv, ret = torch.randint(0, 4, (4,), generator=g), -torch.rand(4, generator=g), torch.randn(4, generator=g), torch.randn(4, generator=g)
    return pol, lambda x: loss(pol, x, actions, old, adv, ret, 0.2, 0.5, 0.01)[0], x


def probe(K=6):
    from ocrl_amd.utils.property_predictor import PropertyPredictor
    x = torch.randn(4, K, 192, generator=_gen())
    pp = _seeded(lambda: PropertyPredictor(GP.StandInEncoder("SLATE", x), GP.probe_config("slate_mlp3"), GP.dataset_config()))
    y = GP.targets(4, 5, 0, torch.float32)

    def call(x):
        pp._encoder._x = x                                    # the stand-in encoder returns what it holds
        return pp.get_loss({"obss": None, "objs": y.to(x.device)})["loss"]
    return pp._module, call, x


CASES = {"RN": rn, "Transformer": transformer, "Transformer_mlp1": lambda: transformer(use_mlp1=True), "MLP": mlp, "CNN_Linear": cnn_linear,
         "NatureCNN": naturecnn, "VAE": vae, "VAE_encode": lambda: vae(loss=False), "CustomNetwork": custom_network, "logits_values": logits_values,
         "ppo_loss": ppo_loss, "probe": probe}

REFUSED = {"RN_one_slot": lambda: rn(K=1), "Transformer_nine_layers": lambda: transformer(num_layers=9),
           "Transformer_long_head_size_8": lambda: transformer(K=40, nhead=8), "CNN_Linear_rep_6": lambda: cnn_linear(6),
           "NatureCNN_rep_6": lambda: naturecnn(6), "VAE_latent_6": lambda: vae(6), "CustomNetwork_width_6": lambda: custom_network(6),
           "logits_values_width_6": lambda: logits_values(6), "ppo_loss_width_6": lambda: ppo_loss(6), "probe_13_slots": lambda: probe(13)}
