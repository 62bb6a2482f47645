"""property-probe micro-benchmark (development aid): the matching kernel alone, a whole PropertyPredictor.update() over recorded slots
(the encoder excluded), the fp64 restatement on the CPU, and the frozen SLATE encoder's model(obs), at B = 128 with the SLATE shape
(K 6, N 5, D 192, mlp3)."""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrl_amd import ocrs
from ocrl_amd.utils.config import compose
from ocrl_amd.utils.property_predictor import PropertyPredictor, probe_match
from tests.golden import make_golden_probe as G
B, K, N, D = int(os.environ.get("B", "128")), 6, 5, 192
torch.manual_seed(0)
slots = torch.randn(B, K, D, device="cuda")
y = G.targets(B, N, 0, torch.float32).cuda()
cfg = G.probe_config("slate_mlp3")
pp = PropertyPredictor(G.StandInEncoder("SLATE", slots), cfg, G.dataset_config())
pp.to("cuda:0")
batch = {"obss": None, "objs": y}
out = torch.randn(B, K, 15, device="cuda")
def t(f, n=50):
    for _ in range(5): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
step = [0]
def upd(): pp.update(batch, step[0]); step[0] += 1
print(f"probe_match (cost, assignment, loss, metrics, d out; incl. the wrapper's allocations) B{B} K{K} N{N}: {t(lambda: probe_match(out, y, *G.schema())):.3f} ms")
print(f"PropertyPredictor.get_loss (mlp3 head + matching, recorded slots) B{B}: {t(lambda: pp.get_loss(batch)):.3f} ms")
print(f"PropertyPredictor.update (get_loss + backward + Adam, recorded slots) B{B}: {t(upd):.3f} ms")
c = compose(os.path.join(ROOT, "configs"), "train_ocr", ["ocr=slate", "dataset=random-N5C4S4S2"])
enc = ocrs.SLATE(c.ocr, c.dataset)
enc._module._max_batch = B
enc.to("cuda:0"); enc.eval(); enc._module.freeze_weights(True)
obs = torch.rand(B, 3, 64, 64, device="cuda")
def encode():
    with torch.no_grad(): enc(obs)
print(f"frozen SLATE encoder model(obs) B{B} 64x64: {t(encode, 20):.3f} ms")
ps = [p.detach().double().cpu().requires_grad_() for p in pp._module.parameters()]
x64, y64 = slots.double().cpu(), y.double().cpu()
t0 = time.perf_counter()
G.ref_probe(x64, ps, y64, K)["loss"].backward()
print(f"ref_probe fp64 on this machine's CPU (forward + backward, numpy bit-mask assignment) B{B}: {(time.perf_counter() - t0) * 1e3:.1f} ms")
