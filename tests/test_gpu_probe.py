"""GPU parity of the slot property probe (ocrl_probe_*: probe.hip, probe_unit.cpp; ocrl_amd.utils.property_predictor) against the
fixture recorded from the reference's PropertyPredictor in fp64 (tests/golden/probe.npz) and its restatement (make_golden_probe.py:
ref_probe).  Bars, the project's own (BASELINE): col exactly equal on every image; loss within 1e-5 relative;
head outputs, cost matrices and metrics within 1e-4 relative; every parameter gradient within 5e-5 of its tensor's maximum."""
import json

import numpy as np
import pytest
import torch

from tests.golden import make_golden_probe as G
from tests.gpu_util import log, relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return np.load(G.fixture_path())


def _gain(fx, tag):
    return json.loads(str(fx["inventory"]))[tag]["gain"]


def _predictor(fx, tag):
    from ocrl_amd.utils.property_predictor import PropertyPredictor
    pp = PropertyPredictor(G.StandInEncoder(G.CASES[tag][0], G.rows(tag, torch.float32)), G.probe_config(tag), G.dataset_config())
    G.load_closed_form(pp._module, _gain(fx, tag))
    pp.to("cuda:0")
    return pp


def _batch(tag):
    return {"obss": None, "objs": G.case_targets(tag, torch.float32).cuda()}


def _metric_errors(metrics, want):
    got = G.metric_vector({k: v.detach().cpu() for k, v in metrics.items()})
    return np.abs(got - want) / np.abs(want)


@pytest.mark.parametrize("tag", list(G.CASES))
def test_fixture_case(fx, tag):
    pp = _predictor(fx, tag)
    metrics = pp.get_loss(_batch(tag))
    assert all(v.is_cuda for v in metrics.values()) and list(metrics) == G.METRIC_NAMES
    metrics["loss"].backward()
    torch.cuda.synchronize()
    e_m = _metric_errors(metrics, fx[tag + "/metrics"])
    e_out = relerr(pp.last_output, torch.from_numpy(fx[tag + "/out"]))
    e_cost = relerr(pp.last_cost, torch.from_numpy(fx[tag + "/cost"]))
    # every gradient in full against the fp64 restatement (pinned to the fixture by tests/test_probe_cpu.py)
    ref = [p.detach().double().cpu().requires_grad_() for p in pp._module.parameters()]
    G.ref_probe(G.rows(tag), ref, G.case_targets(tag), G.CASES[tag][2])["loss"].backward()
    e_g = {n: relerr(p.grad, r.grad) for (n, p), r in zip(pp._module.named_parameters(), ref)}
    log(f"probe {tag}: loss rel {e_m[0]:.2e}, metrics rel {e_m[1:].max():.2e}, out {e_out:.2e}, cost {e_cost:.2e}, worst grad {max(e_g.values()):.2e}")
    assert np.array_equal(pp.last_matching.cpu().numpy(), fx[tag + "/col"])
    assert e_m[0] < 1e-5
    assert e_m[1:].max() < 1e-4 and e_out < 1e-4 and e_cost < 1e-4
    ref_g = {n: r.grad for (n, _), r in zip(pp._module.named_parameters(), ref)}
    for n, p in pp._module.named_parameters():
        assert e_g[n] < 5e-5, (n, e_g[n])
        g = p.grad.double().cpu().numpy().ravel()                # and the recorded entries of the reference's own gradient
        key = tag + "/grad/" + n
        want, got = (fx[key], g) if key in fx else (fx[tag + "/grads/" + n], g[G.sample_idx(g.size)])
        assert np.abs(got - want).max() < 5e-5 * ref_g[n].abs().max().item(), n


def test_match_at_the_slot_limit(fx):
    from ocrl_amd.utils.property_predictor import MAX_SLOTS, probe_match
    out, y = G.wide_inputs(_gain(fx, "wide"), torch.float32)
    assert out.shape[1] == MAX_SLOTS
    r = probe_match(out.cuda(), y.cuda(), *G.schema())
    torch.cuda.synchronize()
    assert np.array_equal(r["col"].cpu().numpy(), fx["wide/col"])
    m = r["metrics"].double().cpu().numpy()
    e = np.abs(m - fx["wide/metrics"]) / np.abs(fx["wide/metrics"])
    e_cost = relerr(r["cost"], torch.from_numpy(fx["wide/cost"]))
    o64 = torch.from_numpy(fx["wide/out"]).requires_grad_()
    G.match_loss(o64, G.wide_inputs(_gain(fx, "wide"))[1])["loss"].backward()
    e_g = relerr(r["dout"], o64.grad)
    log(f"probe wide (K 12, N 9): loss rel {e[0]:.2e}, metrics rel {e[1:].max():.2e}, cost {e_cost:.2e}, dout {e_g:.2e}")
    assert e[0] < 1e-5 and e[1:].max() < 1e-4 and e_cost < 1e-4 and e_g < 5e-5
    unmatched = torch.ones(out.shape[:2], dtype=torch.bool)
    unmatched[torch.arange(out.shape[0])[:, None], torch.from_numpy(fx["wide/col"]).long()] = False
    assert (r["dout"].cpu()[unmatched] == 0).all()             # zero rows for unmatched slots
    # the incoming d loss scales the gradient
    r2 = probe_match(out.cuda(), y.cuda(), *G.schema(), dloss=torch.tensor([0.5], device="cuda"))
    assert torch.equal(r2["dout"], r["dout"] * 0.5) and torch.equal(r2["col"], r["col"])


def test_above_the_slot_limit_is_a_host_side_error():
    from ocrl_amd import _lib
    from ocrl_amd.utils.property_predictor import PropertyPredictor, probe_match
    out = torch.zeros(2, 13, 15, device="cuda")
    y = G.targets(2, 5, 0, torch.float32).cuda()
    with pytest.raises(RuntimeError, match="built for 1 .. 12 slots"):
        probe_match(out, y, *G.schema())
    assert b"12" in _lib.lib().ocrl_last_error()
    pp = PropertyPredictor(G.StandInEncoder("SLATE", torch.zeros(2, 13, 192, device="cuda")), G.probe_config("slate_linear"), G.dataset_config())
    pp.to("cuda:0")
    with pytest.raises(ValueError, match="at most 12"):
        pp.get_loss({"obss": None, "objs": y})


def test_two_runs_are_bit_identical(fx):
    res = []
    for _ in range(2):
        pp = _predictor(fx, "slate_mlp3")
        m = pp.get_loss(_batch("slate_mlp3"))
        m["loss"].backward()
        res.append([m[k].detach().clone() for k in G.METRIC_NAMES] + [pp.last_matching, pp.last_cost, pp.last_output] +
                   [p.grad.clone() for p in pp._module.parameters()])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("tag", ["slate_mlp3", "vae_mlp3"])
def test_three_updates_follow_the_fp64_trajectory(fx, tag):
    pp = _predictor(fx, tag)
    ref = [p.detach().double().cpu().requires_grad_() for p in pp._module.parameters()]
    opt = torch.optim.Adam(ref, lr=1e-4)
    batch = _batch(tag)
    for step in range(3):
        got = pp.update(batch, step)["loss"].item()
        r = G.ref_probe(G.rows(tag), ref, G.case_targets(tag), G.CASES[tag][2])
        opt.zero_grad()
        r["loss"].backward()
        opt.step()
        err = abs(got - r["loss"].item()) / abs(r["loss"].item())
        log(f"probe {tag} update {step}: loss {got:.6f} (fp64 {r['loss'].item():.6f}, rel {err:.2e})")
        assert np.array_equal(pp.last_matching.cpu().numpy(), r["col"])
        assert err < 1e-5
    # Adam's normalised step g / (|g| + eps) turns the fp32 rounding of a near-zero gradient into a step of either sign, so after n steps
    # an entry may sit up to 2 n lr from its fp64 twin whatever the kernels' accuracy; that, plus fp32 storage, is all that can be asked
    worst = max((p.detach().double().cpu() - q.detach()).abs().max().item() for p, q in zip(pp._module.parameters(), ref))
    assert worst <= 2 * 3 * 1e-4 + 1e-6


def test_checkpoint_round_trip(fx, tmp_path):
    a = _predictor(fx, "slate_mlp3")
    a.update(_batch("slate_mlp3"), 0)
    torch.save(a.save(), tmp_path / "probe.pth")
    ck = torch.load(tmp_path / "probe.pth", map_location="cuda:0", weights_only=True)
    assert set(ck) == {"property_predictor_module_state_dict", "property_predictor_opt_state_dict"}
    b = _predictor(fx, "slate_mlp3")
    b.load(ck)
    for (k, p), (_, q) in zip(a._module.state_dict().items(), b._module.state_dict().items()):
        assert torch.equal(p, q), k
    la, lb = a.update(_batch("slate_mlp3"), 1)["loss"], b.update(_batch("slate_mlp3"), 1)["loss"]
    assert torch.equal(la, lb)                                  # the Adam moments came along
    for p, q in zip(a._module.parameters(), b._module.parameters()):
        assert torch.equal(p, q)
    # a reference-shaped nn.Sequential takes the state dict as it is
    ref = torch.nn.Sequential(*[type(m)(m.in_features, m.out_features) if isinstance(m, torch.nn.Linear) else torch.nn.LeakyReLU() for m in a._module])
    ref.load_state_dict(ck["property_predictor_module_state_dict"])


def test_end_to_end_over_a_frozen_slate_encoder():
    """PropertyPredictor(SLATE(...)) at the tiny 16 x 16 configuration of smoke(): shapes, finiteness, and a frozen encoder"""
    from oracle import slate_oracle as O
    from ocrl_amd.utils.data import random_sprite_scenes, scenes_to_obs
    from ocrl_amd.utils.property_predictor import PropertyPredictor
    from tests.gpu_util import build_wrapper
    cfg = O.default_cfg(obs_size=16, vocab_size=256, num_slots=6, num_iterations=3, num_dec_blocks=2)
    ocr = build_wrapper(cfg, O.formula_params(cfg))
    pp = PropertyPredictor(ocr, G.probe_config("slate_mlp3"), G.dataset_config())
    pp.to("cuda:0")
    pp.eval()
    img, objs = random_sprite_scenes(4, 16, seed=3, with_objs=True)
    batch = {"obss": scenes_to_obs(img).cuda(), "objs": torch.from_numpy(objs).cuda()}
    eng = ocr._module.engine
    before_p, before_g = eng.flat_p.clone(), eng.flat_g.clone()
    head_before = [p.detach().clone() for p in pp._module.parameters()]
    for step in range(2):
        m = pp.update(batch, step)
    torch.cuda.synchronize()
    assert list(m) == G.METRIC_NAMES and all(v.is_cuda and v.dim() == 0 and torch.isfinite(v) for v in m.values())
    assert pp.last_matching.shape == (4, 5) and pp.last_matching.dtype == torch.int32 and pp.last_output.shape == (4, 6, 15)
    assert all(len(set(r)) == 5 and 0 <= min(r) and max(r) < 6 for r in pp.last_matching.cpu().tolist())
    assert 0.0 <= m["acc_color"].item() <= 1.0 and m["loss"].item() > 0
    assert torch.equal(eng.flat_p, before_p) and torch.equal(eng.flat_g, before_g)      # no encoder parameter or gradient changed
    assert all(not torch.equal(p, q) for p, q in zip(pp._module.parameters(), head_before))
    ck = pp.save()
    assert "ocr_module_state_dict" in ck and "property_predictor_module_state_dict" in ck
