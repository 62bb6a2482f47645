"""GPU checks of the NatureCNN encoder's inputs: observation channel counts other than 3 against the fp64 restatement (the first layer's
K = 64 cin walks other tails of the four-wave K split), what must raise before any launch on the device (another obs_size, fp16 or
misplaced parameters), and torch's in-place check on what the backward reads again."""
import types

import pytest
import torch

from tests.test_gpu_naturecnn import ref64

pytestmark = pytest.mark.gpu


def _nature(cin, S=64, **over):
    c = dict(rep_dim=512, use_cnn_feat=False, cnn_feat_size=4)
    c.update(over)
    from ocrl_amd import ocrs
    return ocrs.NatureCNN_Module(types.SimpleNamespace(**c), types.SimpleNamespace(obs_size=S, obs_channels=cin)).cuda()


def _grid(m, cin, B, S, seed):
    """weights +-1/4 on a quarter of the entries, biases in {-1/8, 0, 1/8}, observations in {0, 1/2, 1}: the fp32 forward is exact
    (tests/test_gpu_naturecnn.py::grid_params), so fp32 and fp64 ReLU masks agree"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.copy_(torch.randint(-1, 2, p.shape, generator=g).float() * (torch.rand(p.shape, generator=g) < 0.25).float() * 0.25)
            else:
                p.copy_(torch.randint(-1, 2, p.shape, generator=g).float() * 0.125)
    return torch.randint(0, 3, (B, cin, S, S), generator=g).float() * 0.5


@pytest.mark.parametrize("cin,use_feat", [(1, False), (4, False), (5, True), (7, False)])
@pytest.mark.parametrize("B", [3, 32])
def test_channel_counts_against_fp64(cin, use_feat, B):
    m = _nature(cin, use_cnn_feat=use_feat)
    obs = _grid(m, cin, B, 64, 40 + cin + B)
    params = m._param_list()
    out = m(obs.cuda())
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(B))
    (out * cot.cuda()).sum().backward()
    want, leaves = ref64(obs, params, 3, use_feat)
    (want * cot.double()).sum().backward()
    assert out.shape == want.shape
    assert (out.detach().cpu().double() - want.detach()).abs().max() <= 1e-5 * want.abs().max()
    for p, leaf in zip(params, leaves):
        scale = leaf.grad.abs().max().item()
        assert scale > 0 and (p.grad.cpu().double() - leaf.grad).abs().max().item() <= 5e-5 * scale


def test_other_obs_size_raises_on_the_gpu():
    m = _nature(3)
    with pytest.raises(ValueError, match="flatten"):
        m(torch.zeros(2, 3, 84, 84, device="cuda"))
    with pytest.raises(ValueError, match="flatten"):
        m(torch.zeros(2, 3, 48, 48, device="cuda"))
    assert m(torch.zeros(2, 3, 64, 64, device="cuda")).shape == (2, 512)


def test_fp16_or_misplaced_parameters_raise():
    m = _nature(3).half()
    with pytest.raises(RuntimeError, match="float32"):
        m(torch.zeros(2, 3, 64, 64, device="cuda"))
    m = _nature(3).cpu()
    with pytest.raises(RuntimeError, match="float32"):
        m(torch.zeros(2, 3, 64, 64, device="cuda"))


def test_weight_changed_in_place_before_backward_raises():
    m = _nature(3)
    obs = torch.rand(4, 3, 64, 64, device="cuda")
    out = m(obs)
    with torch.no_grad():
        m._cnn[2].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
