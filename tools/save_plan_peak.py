"""Peak device memory of one training step of the PEMS08 model (make_model nb_block=4, B = 32: the
model_step workload of bench.py), as torch.cuda.max_memory_allocated over the step after warm-up.
One JSON line; LD_LIBRARY_PATH / DSTAGNN_EXT select the library as in tools/ab_libs.sh
(profiles/save_plan_ab.json)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import dstagnn_drought_amd as D  # noqa: E402
from dstagnn_drought_amd.train import make_adam  # noqa: E402

c = bench.CFG
dev = torch.device("cuda:0")
tmd, pa = bench.synth_graph(c["N"])
torch.manual_seed(1)
net = D.make_model(dev, 1, 4, 1, c["K"], c["C"], c["C"], 1, tmd, pa, tmd, c["T"], c["T"], c["N"], c["d_model"],
                   c["d_k"], c["d_k"], c["n_heads"])
D.set_direct_grads(net).train()
opt = make_adam(net.parameters(), 1e-4)
crit = torch.nn.SmoothL1Loss().to(dev)
gen = torch.Generator(device=dev).manual_seed(5)
xm = torch.randn(c["B"], c["N"], 1, c["T"], device=dev, generator=gen)
ym = torch.randn(c["B"], c["N"], c["T"], device=dev, generator=gen)


def step():
    opt.zero_grad(set_to_none=True)
    loss = crit(net(xm), ym)
    loss.backward()
    opt.step()
    return loss


for _ in range(3):
    step()
torch.cuda.synchronize()
base = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
loss = step()
torch.cuda.synchronize()
print(json.dumps({"peak_bytes": torch.cuda.max_memory_allocated(), "resident_before_step_bytes": base,
                  "loss": float(loss), "lib": os.environ.get("LD_LIBRARY_PATH", "-")}))
