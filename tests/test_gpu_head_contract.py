"""GPU checks of what every stateless head does the same way (ocrl_amd/_bridge.py), over tests/head_cases.py: parameters that are not
float32 on the input's device raise before any launch, an in-place write on a weight between forward and backward raises, a head on
cuda:1 computes bit for bit what it computes on cuda:0 while cuda:0 stays the current device, a refused shape is a ValueError, and
the actor-critic backward takes strided cotangents."""
import pytest
import torch

from tests.head_cases import CASES, REFUSED

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_fp16_or_misplaced_parameters_raise(name):
    module, call, x = CASES[name]()
    module.cuda().half()
    with pytest.raises(RuntimeError, match="float32"):
        call(x.cuda())
    module, call, x = CASES[name]()                           # the parameters stay on the CPU
    with pytest.raises(RuntimeError, match="float32"):
        call(x.cuda())


@pytest.mark.parametrize("name", ["RN", "Transformer", "CustomNetwork", "logits_values", "probe"])
def test_weight_changed_in_place_before_backward_raises(name):
    module, call, x = CASES[name]()
    module.cuda()
    out = call(x.cuda())
    with torch.no_grad():
        next(module.parameters()).mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


@pytest.mark.parametrize("name", ["CustomNetwork", "logits_values"])
def test_non_contiguous_cotangents_give_the_contiguous_gradients(name):
    """strided cotangents with distinct values per output are converted to copies; the copies must live until the launch"""
    module, _, x = CASES[name]()
    module.cuda()
    x = x.cuda().requires_grad_(True)
    leaves = [x] + list(module.parameters())
    outs = module(x) if name == "CustomNetwork" else module.logits_values(x)
    g = torch.Generator().manual_seed(3)
    wide = [torch.randn(*o.shape[:-1], 2 * o.shape[-1], generator=g).cuda() for o in outs]
    strided = [w[..., ::2] for w in wide]
    assert not any(c.is_contiguous() for c in strided) and not torch.equal(strided[0].flatten()[:4], strided[1].flatten()[:4])
    got = torch.autograd.grad(outs, leaves, strided, retain_graph=True, allow_unused=True)
    want = torch.autograd.grad(outs, leaves, [c.contiguous() for c in strided], allow_unused=True)
    assert any(w is not None and w.abs().max() > 0 for w in want)
    for a, b in zip(got, want):
        assert (a is None and b is None) or torch.equal(a, b)


def _run(name, dev):
    module, call, x = CASES[name]()
    module.to(dev)
    x = x.to(dev).requires_grad_(name not in ("NatureCNN", "VAE", "VAE_encode"))        # these refuse an observation gradient
    out = call(x)
    out.sum().backward()
    return [out.detach().cpu()] + [None if t.grad is None else t.grad.cpu() for t in [x] + list(module.parameters())]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
@pytest.mark.parametrize("name", list(CASES))
def test_head_on_a_device_that_is_not_the_current_one(name):
    torch.cuda.set_device(0)
    want = _run(name, "cuda:0")
    got = _run(name, "cuda:1")
    assert torch.cuda.current_device() == 0
    assert len(got) == len(want) and any(g is not None for g in want[2:])
    for a, b in zip(got, want):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_shape_is_a_value_error(name):
    module, call, x = REFUSED[name]()
    module.cuda()
    with pytest.raises(ValueError, match="shape not supported"):
        call(x.cuda())
