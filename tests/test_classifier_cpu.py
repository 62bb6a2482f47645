"""What the MLP classifier promises without a GPU: the seventh header (include/ocrl_hip_classifier.h) parses, binds and is exported while
the six older tables stay as they were; every rejection its entry point makes before a launch; the restatement of tests/classifier_ref.py
against torch's own cross-entropy on the GPU tests' cases, its fp32 evaluation inside the GPU tests' bounds, and its hand-worked
out-of-range example; the train_classifier config; the module's parameters and the constructor's refusals."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from tests import classifier_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
FAKE = 0x10000                  # a 16-byte aligned address that is never read: every call below is rejected before any launch
WHO = "ocrl_clf_ce_fwd_bwd"
# the bounds of tests/test_gpu_classifier.py (those of tests/test_gpu_dqn.py for the same tile arithmetic)
LOSS_BOUND, LOGIT_BOUND, GRAD_BOUND, GRAD_FLOOR = 1e-4, 1e-5, 3e-4, 1e-3
CASES = [(s, l) for l in R.LAYOUTS for s in R.SHAPES]


def last_error():
    return _lib.lib().ocrl_last_error().decode()


# ---- header and binding
def test_header_parses_and_the_library_exports_what_it_declares():
    text = open(os.path.join(ROOT, "include", "ocrl_hip_classifier.h")).read()
    abi = _abi.read(text)
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == {WHO: 11} and abi.consts == {} and abi.structs == {}
    assert set(_lib.ABI_CLASSIFIER.functions) == {WHO}
    L = _lib.lib()
    f = getattr(L, WHO)                                                                   # the symbol is exported
    assert len(f.argtypes) == 11 and f.argtypes[0] is ctypes.c_void_p and f.argtypes[9] is ctypes.c_size_t
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_CLASSIFIER_H$", text, re.M) and "#include <stddef.h>" in text
    assert '"ocrl_hip' not in text and text.count("#include") == 1                        # self-contained
    # the six older tables are what they were
    assert len(_lib.ABI.functions) == 146 and _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and L.ocrl_abi_version() == 5
    assert len(_lib.ABI_DQN.functions) == 9 and len(_lib.ABI_ROLLOUT.functions) == 1 and len(_lib.ABI_REPLAY.functions) == 8
    assert len(_lib.ABI_C51.functions) == 6 and len(_lib.ABI_NOISY.functions) == 5
    older = [set(a.functions) for a in (_lib.ABI, _lib.ABI_DQN, _lib.ABI_ROLLOUT, _lib.ABI_REPLAY, _lib.ABI_C51, _lib.ABI_NOISY)]
    assert not any(WHO in s for s in older)


def test_the_makefile_names_the_new_parts():
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    for part in ("classifier.hip", "classifier_unit.o", "classifier.h", "ocrl_hip_classifier.h"):
        assert part in makefile, part
    assert re.search(r"^(?:\S+ )*classifier\.o(?: \S+)*: acnet_tile\.h$", makefile, re.M)


# ---- rejections before any launch
def call(d="good", x=FAKE, w="good", labels=FAKE, scalars=FAKE, logits=None, dx=None, dw="good", ws=FAKE, n=1 << 40):
    L = _lib.lib()
    good = _lib.qnet_desc(5, 8, 4, [8, 8], [1, 1])
    six = (ctypes.c_void_p * 6)(*[FAKE] * 6)
    ref = ctypes.byref(good) if isinstance(d, str) else None if d is None else ctypes.byref(d)
    v = lambda a: None if a is None else ctypes.c_void_p(a)
    return L.ocrl_clf_ce_fwd_bwd(ref, v(x), six if isinstance(w, str) else w, v(labels), v(scalars), v(logits), v(dx), six if isinstance(dw, str) else dw,
                                 v(ws), n, None)


def test_arguments_are_checked_before_any_launch():
    L = _lib.lib()
    good = _lib.qnet_desc(5, 8, 4, [8, 8], [1, 1])
    need = L.ocrl_qnet_ws_floats(ctypes.byref(good))
    assert need > 0
    hole = (ctypes.c_void_p * 6)(FAKE, FAKE, None, FAKE, FAKE, FAKE)
    for kw, msg in ((dict(d=None), f"{WHO}: null descriptor"),
                    (dict(x=None), f"{WHO}: null argument"),
                    (dict(w=None), f"{WHO}: null argument"),
                    (dict(labels=None), f"{WHO}: null argument"),
                    (dict(scalars=None), f"{WHO}: null argument"),
                    (dict(ws=None), f"{WHO}: null argument"),
                    (dict(w=hole), f"{WHO}: parameter pointer 2 of 6 is null"),
                    (dict(dw=hole), f"{WHO}: parameter pointer 2 of 6 is null"),
                    (dict(dw=None, dx=FAKE), f"{WHO}: dfeatures without dw"),
                    (dict(n=need - 1), f"{WHO}: workspace too small ({need - 1} < {need} floats)"),
                    (dict(dw=None, n=need - 1), f"{WHO}: workspace too small"),
                    (dict(n=0), "workspace too small")):
        assert call(**kw) != 0 and msg in last_error(), (msg, last_error())


@pytest.mark.parametrize("kw, reason", [(dict(A=65), "1 <= n_actions <= 64"), (dict(A=0), "1 <= n_actions <= 64"), (dict(dims=[6]), "multiples of 4"),
                                        (dict(dims=[260]), "multiples of 4"), (dict(n=9), "at most 8 hidden layers"), (dict(B=0), "batch >= 1"),
                                        (dict(F=0), "feature_dim >= 1"), (dict(acts=[3]), "activation 0")])
def test_what_qnet_ws_floats_rejects_is_rejected(kw, reason):
    kw = dict(dict(B=5, F=8, A=4, dims=[8], acts=[1], n=1), **kw)
    d = _lib.qnet_desc(kw["B"], kw["F"], kw["A"], kw["dims"], kw["acts"])
    d.n = kw["n"]
    assert _lib.lib().ocrl_qnet_ws_floats(ctypes.byref(d)) == 0 and reason in last_error()
    assert call(d=d) != 0 and reason in last_error() and last_error().startswith(WHO)
    assert call(d=d, dw=None) != 0 and reason in last_error()


# ---- the restatement
def rel(got, want, floor=0.0):
    return (got.double() - want.double()).abs().max().item() / max(want.abs().max().item(), floor, 1e-30)


@pytest.mark.parametrize("shape, lname", CASES, ids=lambda v: str(v))
def test_the_restatement_is_torchs_cross_entropy_and_fp32_stays_inside_the_bounds(shape, lname):
    B, F, A = shape
    x, ps, labels = R.case(B, F, A, lname)
    acts = R.LAYOUTS[lname][1]
    assert x.shape == (B, F) and int(labels.min()) >= 0 and int(labels.max()) < A
    scal, z, dx, dw = R.ce_step(x, ps, acts, labels)
    # fp64: torch's own loss and argmax, and their gradients
    xs = x.double().requires_grad_(True)
    pd = [p.double().requires_grad_(True) for p in ps]
    zt = R.q_forward(xs, pd, acts)
    loss = torch.nn.functional.cross_entropy(zt, labels)
    grads = torch.autograd.grad(loss, [xs] + pd)
    assert abs(scal[0].item() - loss.item()) <= 1e-12 * max(loss.item(), 1.0) and scal[2].item() == B
    assert scal[1].item() == pytest.approx((zt.argmax(dim=1) == labels).double().mean().item(), abs=1e-15)
    for g, w in zip([dx] + dw, grads):
        assert rel(g, w) <= 1e-11
    # fp32: torch's own evaluation of the same case, against the bounds the kernel is held to
    s32, z32, dx32, dw32 = R.ce_step(x, ps, acts, labels, torch.float32)
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    e_loss = abs(s32[0].item() - scal[0].item()) / scal[0].item()
    e_z = rel(z32, z)
    e_g = max(rel(g, w, GRAD_FLOOR * gmax) for g, w in zip([dx32] + dw32, [dx] + dw))
    assert e_loss <= LOSS_BOUND and e_z <= LOGIT_BOUND and e_g <= GRAD_BOUND, (e_loss, e_z, e_g)
    assert max(e_loss, e_z, e_g) <= 1e-5                                                  # in fact near 4e-7: the bounds leave room


def test_hand_worked_out_of_range_example():
    """the docstring of tests/classifier_ref.py: a plain row, a tie whose lowest index is the label, a label outside [0, A)"""
    z = torch.tensor([[0.0, math.log(3.0)], [5.0, 5.0], [1.0, 0.0]], dtype=torch.float64, requires_grad=True)
    labels = torch.tensor([1, 0, 7])
    scal = R.ce_rule(z, labels)
    assert scal[0].item() == pytest.approx((math.log(4) - math.log(3) + math.log(2)) / 3, abs=1e-15)
    assert scal[1].item() == pytest.approx(2 / 3, abs=1e-15) and scal[2].item() == 2.0
    scal[0].backward()
    want = torch.tensor([[0.25, -0.25], [-0.5, 0.5], [0.0, 0.0]], dtype=torch.float64) / 3
    assert torch.allclose(z.grad, want, atol=1e-15) and (z.grad[2] == 0).all()
    assert R.ce_rule(z.detach(), torch.tensor([1, 1, -1]))[1].item() == pytest.approx(1 / 3, abs=1e-15)      # the tie's higher index is no hit
    assert R.lowest_argmax(torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [0.0, 1.0, 5.0]])).tolist() == [1, 0, 2]


# ---- config and module
def test_train_classifier_config_resolves_to_the_references_values():
    c = compose(CFG, "train_classifier", ["ocr=slate", "pooling=transformer", "dataset=target-N4C4S3S1"])
    assert c.batch_size == 128 and c.classifier.to_dict() == {"d_model": 64, "learning": {"lr": 0.0001}}
    assert c.ocr.name == "SLATE" and c.pooling.name == "Transformer" and c.dataset.name == "TargetN4C4S3S1" and c.dataset.num_labels == 4
    assert c.run_dir == "./outputs/train_classifier/SLATE-Transformer-TargetN4C4S3S1" and c.wandb.project == "ocrl-classification"
    assert (c.max_steps, c.log_interval, c.eval_interval) == (None, 10, 1000) and "hydra" not in c
    for missing in (["pooling=transformer", "dataset=target-N4C4S3S1"], ["ocr=slate", "dataset=target-N4C4S3S1"], ["ocr=slate", "pooling=transformer"]):
        with pytest.raises(ValueError, match="You must specify"):
            compose(CFG, "train_classifier", missing)
    assert "reference ships" in __import__("train_classifier").__doc__


def _cfg(d_model=64, lr=1e-4):
    return types.SimpleNamespace(d_model=d_model, learning=types.SimpleNamespace(lr=lr))


def _dataset(num_labels=4, rng=(4, 4)):
    return types.SimpleNamespace(num_labels=num_labels, num_objects_range=list(rng))


def test_module_parameters_and_refusals():
    from ocrl_amd.ocrs.flat_module import FlatParamModule
    from ocrl_amd.utils.classifier import Classifier
    torch.manual_seed(2)
    clf = Classifier(R.StubPooling(128), _cfg(), _dataset())
    sd = clf._module.state_dict()
    assert list(sd) == ["0.weight", "0.bias", "2.weight", "2.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(64, 128), (64,), (4, 64), (4,)]
    assert isinstance(clf._opt, torch.optim.Adam) and clf._opt.param_groups[0]["lr"] == 1e-4
    assert set(clf.save()) == {"classifier_module_state_dict", "classifier_opt_state_dict"}
    assert [tuple(p.shape) for p in clf._params()] == [tuple(v.shape) for v in sd.values()]
    with pytest.raises(RuntimeError, match="must live on the GPU"):                        # no CPU fallback
        clf.get_loss({"obss": torch.zeros(3, 128), "labels": torch.zeros(3, 1, dtype=torch.int64)})
    with pytest.raises(RuntimeError, match="labels"):
        clf.get_loss({"obss": torch.zeros(3, 128)})
    # a task dataset names its objects under `task`
    c = compose(CFG, "train_classifier", ["ocr=slate", "pooling=transformer", "dataset=target-N4C4S3S1"])
    assert list(Classifier(R.StubPooling(128), c.classifier, c.dataset)._module.state_dict()) == list(sd)
    c.dataset.task.num_objects_range = [4, 6]
    with pytest.raises(ValueError, match=r"dataset\.num_labels = 4 must cover the 6 objects"):
        Classifier(R.StubPooling(128), c.classifier, c.dataset)
    # each refusal names its key
    with pytest.raises(ValueError, match=r"dataset\.num_labels = 3"):
        Classifier(R.StubPooling(128), _cfg(), _dataset(3))
    with pytest.raises(ValueError, match=r"dataset\.num_labels = 65"):
        Classifier(R.StubPooling(128), _cfg(), _dataset(65))
    assert Classifier(R.StubPooling(8), _cfg(4), _dataset(64))._module[2].out_features == 64
    for bad in (0, 2, 6, 66, 260):
        with pytest.raises(ValueError, match=rf"classifier\.d_model .* \(got {bad}\)"):
            Classifier(R.StubPooling(128), _cfg(bad), _dataset())
    assert Classifier(R.StubPooling(128), _cfg(256), _dataset())._module[0].out_features == 256

    class Flat(FlatParamModule):
        backend = "SLATE"

    aux = R.StubPooling(128)
    aux._learn_aux_loss, aux._ocr = True, types.SimpleNamespace(_module=Flat())
    with pytest.raises(NotImplementedError, match=r"pooling\.learn_aux_loss=True .* SLATE"):
        Classifier(aux, _cfg(), _dataset())
    aux._ocr = types.SimpleNamespace(_module=torch.nn.Linear(2, 2))                      # an autograd-trained encoder is taken
    assert Classifier(aux, _cfg(), _dataset())._learn_aux_loss
