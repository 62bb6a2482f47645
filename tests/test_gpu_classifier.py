"""GPU checks of the MLP classifier: ``ocrl_clf_ce_fwd_bwd`` (include/ocrl_hip_classifier.h) through the C ABI, ``Classifier.update``, the
routing of its gradient into a SLATE encoder, and train_classifier.py, against the restatement of tests/classifier_ref.py.

Bounds are those tests/test_gpu_dqn.py applies to the same tile arithmetic: the loss 1e-4 relative, the logits 1e-5 of the largest, every
gradient 3e-4 of its tensor's largest entry with a floor of 1e-3 of the largest gradient of the case.  Torch's own fp32 evaluation of the
same cases sits near 4e-7 on all three (tests/test_classifier_cpu.py asserts it stays inside).  The accuracy is exact: the count, over
the returned fp32 logits, of rows whose lowest-index maximum is the label, divided by B.  ``Classifier.update`` is graded on dp / lr,
elementwise, against the fp64 restatement with torch's Adam; the bound is TRAIN_MARGIN x TRAIN_DEV below."""
import ctypes
import functools
import json
import math
import os
import types

import pytest
import torch

from tests import classifier_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
LOSS_BOUND, LOGIT_BOUND, GRAD_BOUND, GRAD_FLOOR = 1e-4, 1e-5, 3e-4, 1e-3
CASES = [(s, l) for l in R.LAYOUTS for s in R.SHAPES]


def _lib():
    from ocrl_amd import _lib as lib
    return lib, lib.lib()


def nanlike(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def err(got, want, floor=0.0):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert torch.isfinite(got).all(), "non-finite entries (an output the kernels did not write?)"
    return (got - want).abs().max().item() / max(want.abs().max().item(), floor, 1e-30)


def run_clf(x, ps, layout, A, labels, want_dx=True, evaluate=False, want_logits=True):
    """one call on buffers pre-filled with NaN: dict(scal [3], logits, dx, dw), every absent output None"""
    lib, L = _lib()
    B, F = x.shape
    d = lib.qnet_desc(B, F, A, *layout)
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    assert n > 0, L.ocrl_last_error().decode()
    xs, pd, lb = x.cuda(), [p.cuda() for p in ps], labels.cuda().long().reshape(-1).contiguous()
    scal, ws = nanlike(3), nanlike(n)
    logits = nanlike(B, A) if want_logits else None
    dw = None if evaluate else [nanlike(*p.shape) for p in ps]
    dx = nanlike(B, F) if want_dx and not evaluate else None
    lib.check(L.ocrl_clf_ce_fwd_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(lb), lib.ptr(scal), lib.ptr(logits), lib.ptr(dx),
                                    None if evaluate else lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(scal=scal, logits=logits, dx=dx, dw=dw)


def run_generic(x, ps, layout, A, labels):
    """the same step without the fused kernel: ocrl_qnet_fwd with save, dz formed by torch autograd from its q, then ocrl_qnet_bwd"""
    lib, L = _lib()
    B, F = x.shape
    d = lib.qnet_desc(B, F, A, *layout)
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    xs, pd, q, ws = x.cuda(), [p.cuda() for p in ps], nanlike(B, A), nanlike(n)
    lib.check(L.ocrl_qnet_fwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(q), 1, lib.ptr(ws), n, lib.stream()))
    z = q.clone().requires_grad_(True)
    scal = R.ce_rule(z, labels.cuda())
    scal[0].backward()
    dq = z.grad.contiguous()
    dw, dx = [nanlike(*p.shape) for p in ps], nanlike(B, F)
    lib.check(L.ocrl_qnet_bwd(ctypes.byref(d), lib.ptr(xs), lib.ptrs(pd), lib.ptr(dq), lib.ptr(dx), lib.ptrs(dw), lib.ptr(ws), n, lib.stream()))
    torch.cuda.synchronize()
    return dict(scal=scal.detach(), logits=q, dx=dx, dw=dw)


@functools.lru_cache(maxsize=None)
def ref(B, F, A, lname):
    x, ps, labels = R.case(B, F, A, lname)
    return R.ce_step(x, ps, R.LAYOUTS[lname][1], labels)


def exact_acc(logits, labels):
    """the count of rows of the fp32 logits whose lowest-index maximum is the label, over B, as fp32 divides"""
    z, lb = logits.cpu(), labels.reshape(-1).cpu()
    hits = (R.lowest_argmax(z) == lb).sum()
    return (hits.float() / torch.tensor(float(z.shape[0]))).item()


def check_against(tag, got, want, bounds=True):
    """the three bounds of the module docstring on one result; returns the worst (loss, logits, gradient) errors"""
    scal, z, dx, dw = want
    e_loss = abs(got["scal"][0].item() - scal[0].item()) / abs(scal[0].item())
    e_z = err(got["logits"], z)
    gmax = max(g.abs().max().item() for g in [dx] + dw)
    e_g = 0.0
    for nme, g, w in zip(["dx"] + [f"dw{i}" for i in range(len(dw))], [got["dx"]] + got["dw"], [dx] + dw):
        e = err(g, w, GRAD_FLOOR * gmax)
        e_g = max(e_g, e)
        if bounds:
            assert e <= GRAD_BOUND, (tag, nme, e)
    if bounds:
        assert math.isfinite(got["scal"][0].item()) and e_loss <= LOSS_BOUND and e_z <= LOGIT_BOUND, (tag, e_loss, e_z)
    return e_loss, e_z, e_g


# ------------------------------------------------------------------------------------------------------------ 1. against fp64, 3. variants
@pytest.mark.parametrize("shape, lname", CASES, ids=lambda v: str(v))
def test_step_against_fp64(shape, lname):
    B, F, A = shape
    layout = R.LAYOUTS[lname]
    x, ps, labels = R.case(B, F, A, lname)
    tag = f"B{B} F{F} A{A} {lname}"
    got = run_clf(x, ps, layout, A, labels)
    e = check_against(tag, got, ref(B, F, A, lname))
    log(f"clf {tag}: loss rel err {e[0]:.2e} (bound {LOSS_BOUND:.0e}), logits {e[1]:.2e} (bound {LOGIT_BOUND:.0e}), worst gradient {e[2]:.2e} "
        f"(bound {GRAD_BOUND:.0e}); acc {got['scal'][1].item():.4f}")
    assert got["scal"][1].item() == exact_acc(got["logits"], labels) and got["scal"][2].item() == B
    # again: the same bits.  Without dfeatures: dw and the scalars bitwise.  Evaluating: the scalars and the logits bitwise
    again, nodx, ev = run_clf(x, ps, layout, A, labels), run_clf(x, ps, layout, A, labels, want_dx=False), run_clf(x, ps, layout, A, labels, evaluate=True)
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bits(again["scal"], got["scal"]) and bits(again["logits"], got["logits"]) and bits(again["dx"], got["dx"])
    assert all(bits(a, b) for a, b in zip(again["dw"], got["dw"]))
    assert nodx["dx"] is None and bits(nodx["scal"], got["scal"]) and all(bits(a, b) for a, b in zip(nodx["dw"], got["dw"]))
    assert ev["dw"] is None and ev["dx"] is None and bits(ev["scal"], got["scal"]) and bits(ev["logits"], got["logits"])
    nolog = run_clf(x, ps, layout, A, labels, evaluate=True, want_logits=False)
    assert nolog["logits"] is None and bits(nolog["scal"], got["scal"])


# ------------------------------------------------------------------------------------------------------------ 2. fused against generic
@pytest.mark.parametrize("shape, lname", CASES, ids=lambda v: str(v))
def test_fused_against_generic(shape, lname):
    B, F, A = shape
    layout = R.LAYOUTS[lname]
    x, ps, labels = R.case(B, F, A, lname)
    tag = f"B{B} F{F} A{A} {lname}"
    got, gen = run_clf(x, ps, layout, A, labels), run_generic(x, ps, layout, A, labels)
    assert torch.equal(got["logits"].view(torch.int32), gen["logits"].view(torch.int32))               # ocrl_qnet_fwd's bits
    e = check_against(tag + " generic", gen, ref(B, F, A, lname))
    # the two paths against each other, under the same bounds
    gmax = max(g.abs().max().item() for g in [gen["dx"]] + gen["dw"])
    e_f = max(err(a, b, GRAD_FLOOR * gmax) for a, b in zip([got["dx"]] + got["dw"], [gen["dx"]] + gen["dw"]))
    e_l = abs(got["scal"][0].item() - gen["scal"][0].item()) / abs(gen["scal"][0].item())
    log(f"clf {tag}: generic path against fp64: loss {e[0]:.2e}, gradient {e[2]:.2e}; fused against generic: loss {e_l:.2e}, gradient {e_f:.2e}")
    # the accuracy is compared as a count: torch on the GPU divides by a Python scalar through its reciprocal, which is not fp32's quotient
    assert e_f <= GRAD_BOUND and e_l <= LOSS_BOUND and round(got["scal"][1].item() * B) == round(gen["scal"][1].item() * B)
    assert got["scal"][1].item() == exact_acc(gen["logits"], labels)


# ------------------------------------------------------------------------------------------------------------ 4. row independence
@pytest.mark.parametrize("lname", list(R.LAYOUTS))
def test_a_row_does_not_depend_on_its_position_or_on_the_batch(lname):
    """rows 0 .. 4 of the B = 17 case alone (B = 5), and at the end of the batch (another tile, another lane): logits bitwise, B * dfeatures
    to 1e-6 relative (1 / B is the one operation that differs)"""
    layout = R.LAYOUTS[lname]
    x, ps, labels = R.case(17, 12, 4, lname)
    perm = torch.cat([torch.arange(5, 17), torch.arange(5)])
    full, head, moved = run_clf(x, ps, layout, 4, labels), run_clf(x[:5], ps, layout, 4, labels[:5]), run_clf(x[perm], ps, layout, 4, labels[perm])
    assert torch.equal(full["logits"][:5], head["logits"]) and torch.equal(moved["logits"][12:], head["logits"])
    assert torch.equal(moved["logits"][:12], full["logits"][5:])
    a, b, c = 17 * full["dx"][:5], 5 * head["dx"], 17 * moved["dx"][12:]
    scale = a.abs().max().item()
    assert scale > 0 and (a - b).abs().max().item() <= 1e-6 * scale and torch.equal(a, c)


# ------------------------------------------------------------------------------------------------------------ 5. stability
def test_large_logits_stay_finite_and_inside_the_bounds():
    """the output Linear of the (17, 12, 4) case times 400: in fp64 |z| reaches 292 and the loss 116, far past where exp(z) overflows"""
    lname, layout = "clf", R.LAYOUTS["clf"]
    x, ps, labels = R.case(17, 12, 4, lname)
    ps = ps[:-2] + [ps[-2] * 400.0, ps[-1] * 400.0]
    want = R.ce_step(x, ps, layout[1], labels)
    assert want[1].abs().max().item() > 88.8 and want[0][0].item() > 10.0                 # exp overflows fp32 past 88.7
    got = run_clf(x, ps, layout, 4, labels)
    e = check_against("B17 F12 A4 clf x400", got, want)
    log(f"clf x400: max |z| {want[1].abs().max().item():.1f}, loss {got['scal'][0].item():.4f} (fp64 {want[0][0].item():.4f}), rel err {e[0]:.2e}, "
        f"logits {e[1]:.2e}, worst gradient {e[2]:.2e}")
    assert all(torch.isfinite(t).all() for t in [got["scal"], got["dx"]] + got["dw"])
    assert got["scal"][1].item() == exact_acc(got["logits"], labels)


def test_an_exact_tie_counts_for_the_lowest_index():
    """classes 1 and 3 with zero weight rows and equal biases above every other logit: z[:, 1] == z[:, 3] bitwise and the maximum"""
    B, F, A, layout = 37, 12, 4, R.LAYOUTS["clf"]
    x, ps, _ = R.case(17, 12, 4, "clf")
    x = torch.randn(B, F, generator=torch.Generator().manual_seed(7))
    ps = [p.clone() for p in ps]
    ps[-2][1], ps[-2][3] = 0.0, 0.0
    ps[-1][1], ps[-1][3] = 50.0, 50.0
    labels = torch.tensor([1, 3] * B)[:B]
    got = run_clf(x, ps, layout, A, labels)
    z = got["logits"].cpu()
    assert torch.equal(z[:, 1], z[:, 3]) and (z[:, 1] == 50.0).all() and (z[:, [0, 2]] < 50.0).all()
    n1 = int((labels == 1).sum())
    assert 0 < n1 < B and got["scal"][1].item() == (torch.tensor(float(n1)) / torch.tensor(float(B))).item() == exact_acc(got["logits"], labels)
    want = R.ce_step(x, ps, layout[1], labels)
    check_against("tie", got, want)
    assert abs(got["scal"][0].item() - math.log(2.0)) < 1e-4                              # p = 1/2 on both: every row's loss is ln 2


# ------------------------------------------------------------------------------------------------------------ 6. labels outside [0, A)
@pytest.mark.parametrize("shape, lname", [((17, 12, 4), "clf"), ((37, 128, 15), "mlp"), ((1040, 8, 4), "none")], ids=lambda v: str(v))
def test_labels_outside_the_range_contribute_nothing(shape, lname):
    B, F, A = shape
    layout = R.LAYOUTS[lname]
    x, ps, labels = R.case(B, F, A, lname)
    labels = labels.clone()
    labels[0], labels[-1] = -3, A + 5
    want = R.ce_step(x, ps, layout[1], labels)
    got = run_clf(x, ps, layout, A, labels)
    assert got["scal"][2].item() == B - 2 == want[0][2].item()
    assert (got["dx"][0] == 0).all() and (got["dx"][-1] == 0).all() and (got["dx"][1:-1] != 0).any()
    check_against(f"B{B} F{F} A{A} {lname} out-of-range", got, want)
    inside = torch.ones(B, dtype=torch.bool)
    inside[0] = inside[-1] = False
    hits = ((R.lowest_argmax(got["logits"].cpu()) == labels) & inside).sum()
    assert got["scal"][1].item() == (hits.float() / torch.tensor(float(B))).item()
    ev = run_clf(x, ps, layout, A, labels, evaluate=True)
    assert torch.equal(ev["scal"].view(torch.int32), got["scal"].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ 7. training
# largest |dp_fp32 / lr - dp_fp64 / lr| of the restatement (tests/classifier_ref.train: torch autograd + torch.optim.Adam) over every
# parameter after the TRAIN_UPDATES updates of test_update_against_the_restatement, measured on a CPU by train_deviation(): 1.08e-5 of
# updates that reach 2.0.  (Adam's first steps are g / (|g| + 1e-8) ~ +-1: the deviation sits on the few entries whose gradient is small
# enough for its rounding to show against eps.)
TRAIN_DEV = 1.1e-5
TRAIN_MARGIN = 4                  # the kernel's sum order differs from torch's: the factor tests/test_gpu_dqn.py allows for the same reason
TRAIN_LR, TRAIN_UPDATES, TRAIN_SHAPE = 1e-3, 2, (37, 128, 4)


def train_inputs():
    """(the classifier's initial parameters, the batches) of test 7 on the CPU: fixed features, one batch per update"""
    from ocrl_amd.utils.classifier import Classifier
    B, F, A = TRAIN_SHAPE
    torch.manual_seed(23)
    clf = Classifier(R.StubPooling(F), types.SimpleNamespace(d_model=64, learning=types.SimpleNamespace(lr=TRAIN_LR)),
                     types.SimpleNamespace(num_labels=A, num_objects_range=[A, A]))
    gen = torch.Generator().manual_seed(29)
    batches = [(torch.randn(B, F, generator=gen), torch.randint(0, A, (B, 1), generator=gen)) for _ in range(TRAIN_UPDATES)]
    return clf, [p.detach().clone() for p in clf._params()], batches


def train_deviation():
    """what TRAIN_DEV records (CPU)"""
    _, ps, batches = train_inputs()
    p32, p64 = R.train(ps, (1,), batches, TRAIN_LR, torch.float32), R.train(ps, (1,), batches, TRAIN_LR, torch.float64)
    return max(((a.double() - p0.double()) - (w - p0.double())).abs().max().item() for a, w, p0 in zip(p32, p64, ps)) / TRAIN_LR


def test_update_against_the_restatement():
    clf, ps, batches = train_inputs()
    clf.to("cuda:0")
    want = R.train(ps, (1,), batches, TRAIN_LR, torch.float64)
    for step, (x, labels) in enumerate(batches):
        m = clf.update({"obss": x.cuda(), "labels": labels.cuda()}, step)
        assert set(m) == {"loss", "ce", "acc", "valid_rows"} and all(v.is_cuda for v in m.values())
        assert m["valid_rows"].item() == TRAIN_SHAPE[0] and torch.equal(m["loss"].detach(), m["ce"])
        assert m["acc"].item() == exact_acc(clf.last_logits, labels)
    bound = TRAIN_MARGIN * TRAIN_DEV
    worst = 0.0
    for i, (g, w, p0) in enumerate(zip(clf._params(), want, ps)):
        worst = max(worst, ((g.detach().cpu().double() - p0.double()) - (w - p0.double())).abs().max().item() / TRAIN_LR)
        assert (g.detach().cpu() != p0).any(), i
    log(f"clf update: worst dp/lr deviation {worst:.2e} (bound {bound:.2e}, {worst / bound:.2f} of it)")
    assert worst <= bound


def test_no_grad_reaches_the_evaluating_form(monkeypatch):
    """validation: under torch.no_grad() get_loss passes a null dw and a null dfeatures (two launches, no backward), with grad enabled
    it passes both lists; the scalars and the logits are the same bits either way"""
    lib, L = _lib()
    clf, _, batches = train_inputs()
    clf.to("cuda:0")
    calls, entry = [], L.ocrl_clf_ce_fwd_bwd

    def spy(*args):
        calls.append((args[6] is not None, args[7] is not None))                          # (dfeatures, dw) given?
        return entry(*args)
    monkeypatch.setattr(L, "ocrl_clf_ce_fwd_bwd", spy)
    batch = {"obss": batches[0][0].cuda(), "labels": batches[0][1].cuda()}
    with torch.no_grad():
        ev = clf.get_loss(batch)
        ev_logits = clf.last_logits
    assert calls == [(False, False)] and not ev["loss"].requires_grad and math.isfinite(ev["loss"].item())
    tr = clf.get_loss(batch)
    assert calls[1:] == [(False, True)] and tr["loss"].requires_grad                       # fixed features: no dfeatures, but dw
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(bits(ev[k], tr[k].detach()) for k in ("loss", "ce", "acc", "valid_rows")) and bits(ev_logits, clf.last_logits)
    tr["loss"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in clf._params())
    attached = dict(batch, obss=batch["obss"].clone().requires_grad_(True))               # a representation that wants its gradient
    clf.get_loss(attached)["loss"].backward()
    assert calls[2:] == [(True, True)] and attached["obss"].grad.abs().max() > 0
    for p in clf._params():                                                               # frozen parameters under grad mode: nothing to take
        p.requires_grad_(False)
    frozen = clf.get_loss(batch)
    assert calls[3:] == [(False, False)] and not frozen["loss"].requires_grad and bits(frozen["loss"], ev["loss"])


# ------------------------------------------------------------------------------------------------------------ 8. encoder routing
TINY = ["ocr.dvae.vocab_size=256", "ocr.slotattr.num_slots=6", "ocr.slotattr.num_iterations=3", "ocr.tfdec.num_dec_blocks=2", "dataset.obs_size=16"]
TASK = ["ocr=slate", "pooling=transformer", "dataset=target-N4C4S3S1", "dataset.with_objs=True", "device=cuda:0"]
ENC = ("_enc.", "_enc_pos.", "_slotattn.")


def build_classifier(*over):
    from ocrl_amd import ocrs, poolings
    from ocrl_amd.utils.classifier import Classifier
    from ocrl_amd.utils.config import compose
    from ocrl_amd.utils.datasets import get_dataloaders
    c = compose(CFG, "train_classifier", TASK + TINY + ["batch_size=4"] + list(over))
    torch.manual_seed(3)
    ocr = ocrs.SLATE(c.ocr, c.dataset)
    pooling = poolings.Transformer(ocr, c.pooling)
    clf = Classifier(pooling, c.classifier, c.dataset)
    clf.to("cuda:0")
    batch = next(iter(get_dataloaders(c.dataset, 4, 0, seed=1, device="cuda:0")[0]))
    return clf, ocr, pooling, {"obss": batch["obss"], "labels": batch["labels"]}


@pytest.mark.parametrize("downstream", [False, True], ids=["detached", "downstream"])
def test_the_gradient_reaches_the_encoder_only_when_asked(downstream):
    clf, ocr, pooling, batch = build_classifier(f"pooling.learn_downstream_loss={downstream}")
    assert batch["obss"].shape == (4, 3, 16, 16) and batch["labels"].shape == (4, 1) and batch["labels"].dtype == torch.int64
    assert int(batch["labels"].min()) >= 0 and int(batch["labels"].max()) < 4
    snap = lambda mod: {k: v.detach().clone() for k, v in mod.named_parameters()}
    enc0, pool0, clf0 = snap(ocr._module), snap(pooling._module), snap(clf._module)
    clf.train()
    m = clf.update(batch, 0)
    assert math.isfinite(m["loss"].item()) and m["valid_rows"].item() == 4
    moved = lambda before, mod: {k: not torch.equal(v.detach(), before[k]) for k, v in mod.named_parameters()}
    assert all(moved(clf0, clf._module).values()) and any(moved(pool0, pooling._module).values())
    enc = moved(enc0, ocr._module)
    if not downstream:
        assert not any(enc.values()), [k for k, v in enc.items() if v]
    else:
        assert any(v for k, v in enc.items() if k.startswith(ENC))
        assert not any(v for k, v in enc.items() if not k.startswith(ENC)), [k for k, v in enc.items() if v and not k.startswith(ENC)]
        assert any(v for k, v in enc.items() if k.startswith("_slotattn.")) and any(v for k, v in enc.items() if k.startswith("_enc."))


# ------------------------------------------------------------------------------------------------------------ 9. the entry point
def test_train_classifier_writes_metrics_and_a_checkpoint_that_reloads(tmp_path):
    import train_classifier
    from ocrl_amd import ocrs, poolings
    from ocrl_amd.utils.classifier import Classifier
    from ocrl_amd.utils.config import compose
    over = TASK + TINY + ["dataset.on_device=True", "batch_size=8", "max_steps=3", "eval_interval=2", "log_interval=1", "dataset.synthetic_val=16",
                          f"run_dir={tmp_path / 'run'}"]
    assert train_classifier.main(over) == 3
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    train = [l for l in lines if "train/ce" in l]
    assert [l["step"] for l in train] == [0, 1, 2] and [l["step"] for l in lines if "val/loss" in l] == [2]
    for l in train:
        assert math.isfinite(l["train/ce"]) and 0 <= l["train/acc"] <= 1 and l["train/valid_rows"] == 8 and l["train/loss"] == l["train/ce"]
    val = [l for l in lines if "val/loss" in l][0]
    assert math.isfinite(val["val/loss"]) and 0 <= val["val/acc"] <= 1
    ck = torch.load(str(tmp_path / "run" / "checkpoints" / "model_latest.pth"), map_location="cpu", weights_only=True)
    assert {"step", "epoch", "best_val_loss", "classifier_module_state_dict", "classifier_opt_state_dict", "pooling_module_state_dict",
            "pooling_opt_state_dict", "ocr_module_state_dict"} <= set(ck) and ck["step"] == 3
    assert list(ck["classifier_module_state_dict"]) == ["0.weight", "0.bias", "2.weight", "2.bias"]
    assert (tmp_path / "run" / "checkpoints" / "model_2.pth").exists() and (tmp_path / "run" / "checkpoints" / "model_best.pth").exists()
    # the checkpoint reloads into a fresh Classifier
    c = compose(CFG, "train_classifier", over)
    torch.manual_seed(77)
    ocr = ocrs.SLATE(c.ocr, c.dataset)
    fresh = Classifier(poolings.Transformer(ocr, c.pooling), c.classifier, c.dataset)
    fresh.to("cuda:0")
    assert not torch.equal(fresh._module[0].weight.detach().cpu(), ck["classifier_module_state_dict"]["0.weight"])
    fresh.load(torch.load(str(tmp_path / "run" / "checkpoints" / "model_latest.pth"), map_location="cuda:0", weights_only=True))
    for k, v in fresh._module.state_dict().items():
        assert torch.equal(v.cpu(), ck["classifier_module_state_dict"][k]), k
    for k, v in fresh._pooling._module.state_dict().items():
        assert torch.equal(v.cpu(), ck["pooling_module_state_dict"][k]), k
    # a dataset without a target has no labels to train on
    with pytest.raises(RuntimeError, match="labels"):
        train_classifier.main(["ocr=slate", "pooling=transformer", "dataset=random-N5C4S4S2", "dataset.on_device=True", "dataset.with_objs=True",
                               "device=cuda:0"] + TINY + ["batch_size=8", "max_steps=3", "eval_interval=2", f"run_dir={tmp_path / 'random'}"])
