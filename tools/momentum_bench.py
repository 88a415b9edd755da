#!/usr/bin/env python
"""The full training step with SGD momentum on the MI355X, one JSON line per run.

Times the fused plan's step (forward, backward, optimizer) under ``DistributedDataParallel(
overlap_optimizer=True)`` at world size 1 -- the trainers' plan -- for two optimizers:

* ``momentum``: ``SGD(lr, momentum=0.9)``;
* ``nesterov_wd``: ``SGD(lr, momentum=0.9, weight_decay=1e-4, nesterov=True)``;

and, with ``--plain``, ``SGD(lr)`` beside them.  Each set runs in a child process of its own under
``--time-limit`` seconds (a set that runs out is reported as such and the others still run); per set
the line holds ms per step over ``--repeats`` timed windows of ``--steps`` steps (HIP events, warm-up
excluded) and the peak memory allocated.  Only the public API is used, so the same file measures a
tree from before the momentum fast paths existed.  Needs a GPU: a timing has no CPU fallback.

    python tools/momentum_bench.py --image-size 3000 --batch-size 5
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETS = {
    "plain": {},
    "momentum": {"momentum": 0.9},
    "nesterov_wd": {"momentum": 0.9, "weight_decay": 1e-4, "nesterov": True},
}


def _child(a):
    import torch

    import torch_distributed_sandbox_amd as tds
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.ops import functional as TF
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    if not torch.cuda.is_available():
        raise SystemExit("momentum_bench: needs a GPU (a timing has no CPU fallback)")
    tds._ext.ops()
    dev = torch.device("cuda", 0)
    H, B = a.image_size, a.batch_size
    torch.manual_seed(0)
    model = ConvNet(image_shape=(H, H), device=dev, mode="fused")
    ddp = DistributedDataParallel(model, device_ids=[0], overlap_optimizer=True)
    opt = ddp.attach_optimizer(SGD(model.parameters(), a.lr, **SETS[a.child]))
    crit = CrossEntropyLoss()
    src = torch.randint(0, 256, (B, 28, 28), dtype=torch.uint8, device=dev)
    x = TF.upsample_bilinear_u8(src, H, H, levels=True)
    y = torch.randint(0, 10, (B,), device=dev)

    def step():
        loss = crit(ddp(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        step()
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            loss = step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.steps)
    ddp.wait_pending_updates()
    torch.cuda.synchronize()
    print(json.dumps({"ms_per_step": ms, "peak_mem_gb": torch.cuda.max_memory_allocated(dev) / 1e9,
                      "fc_grad_is_none": model.fc.weight.grad is None, "final_loss": float(loss.item()),
                      "device": torch.cuda.get_device_name(dev)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image-size", type=int, default=3000)
    ap.add_argument("--batch-size", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain", action="store_true", help="also time SGD(lr)")
    ap.add_argument("--time-limit", type=float, default=180.0, help="seconds per optimizer set (its own process)")
    ap.add_argument("--child", default=None, choices=list(SETS), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        return _child(a)
    rec = {"metric": "momentum_bench", "image_size": a.image_size, "batch_size": a.batch_size, "lr": a.lr,
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    base = [sys.executable, os.path.abspath(__file__)] + [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in
                                                           ("image_size", "batch_size", "lr", "steps", "warmup", "repeats")]
    for name in (["plain"] if a.plain else []) + ["momentum", "nesterov_wd"]:
        try:
            p = subprocess.run(base + ["--child", name], capture_output=True, text=True, timeout=a.time_limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            rec[name] = {"error": f"no result within {a.time_limit:.0f} s"}
            break  # (a hung step: nothing more is started on the GPU)
        if p.returncode != 0:
            rec[name] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-500:]}
            break
        rec[name] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
