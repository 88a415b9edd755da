#!/usr/bin/env python
"""The training step with and without the input gradient on the MI355X, one JSON line.

Three arms on an fp32 batch, alternating in one process (HIP events around ``--steps`` steps, warm-up
excluded, ``--repeats`` windows per arm, interleaved):

* ``fused_dx``: the fused plan's step with ``x.requires_grad`` (csrc/kernels/l1_dgrad.hip);
* ``fused``: the same step without it (the step as it was);
* ``layers_dx``: ``mode="layers"`` with ``x.requires_grad``, the only source of ``x.grad`` before;

and ``dgrad_ms``: ``ops.fused_l1_input_grad`` alone (its two launches) on the tensors of a real step,
with the bytes it moves.  Needs a GPU: a timing has no CPU fallback.

    python tools/input_grad_bench.py --image-size 3000 --batch-size 5
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image-size", type=int, default=3000)
    ap.add_argument("--batch-size", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args(argv)

    import torch

    import torch_distributed_sandbox_amd as tds
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss

    if not torch.cuda.is_available():
        raise SystemExit("input_grad_bench: needs a GPU (a timing has no CPU fallback)")
    ops = tds._ext.ops()
    dev = torch.device("cuda", 0)
    H, B = a.image_size, a.batch_size
    torch.manual_seed(0)
    crit = CrossEntropyLoss()
    x0 = torch.rand(B, 1, H, H, device=dev)
    y = torch.randint(0, 10, (B,), device=dev)

    def arm(mode, needs_grad):
        model = ConvNet(image_shape=(H, H), device=dev, mode=mode)
        opt = SGD(model.parameters(), a.lr)

        def step():
            x = x0.detach().requires_grad_(needs_grad)
            loss = crit(model(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            assert (x.grad is not None) == needs_grad
        return step

    arms = {"fused_dx": arm("fused", True), "fused": arm("fused", False), "layers_dx": arm("layers", True)}

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for fn in arms.values():
        for _ in range(a.warmup):
            fn()
    rec = {"metric": "input_grad_bench", "image_size": H, "batch_size": B, "steps": a.steps, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(dev), "ms_per_step": {k: [] for k in arms}}
    for _ in range(a.repeats):
        for k, fn in arms.items():
            rec["ms_per_step"][k].append(timed(fn, a.steps))

    # the new op alone, on a real forward's tensors and a random pooled gradient
    P = H // 2
    c1, bn1 = ConvNet(image_shape=(H, H), device=dev, mode="fused").layer1[:2]
    rm, rv, nbt = torch.zeros(16, device=dev), torch.ones(16, device=dev), torch.zeros((), dtype=torch.long, device=dev)
    p1, idx1, stats, gram, _ = ops.fused_l1_forward(x0, c1.weight, c1.bias, bn1.weight, bn1.bias, rm, rv, nbt, 0.1, 1e-5)
    dp1h = torch.randn(B, P, (P + 3) // 4, 16, 4, device=dev).half()
    dec = torch.tensor([2.0 ** -9], dtype=torch.float32, device=dev).view(torch.int32)
    bsum = torch.empty(16 * 27, dtype=torch.float64, device=dev)
    ops.fused_l1_backward(dp1h, dec, x0, p1, idx1, c1.weight, c1.bias, bn1.weight, stats, gram, 1.0, None, None, None,
                          None, bsum)
    run = lambda: ops.fused_l1_input_grad(dp1h, dec, x0, idx1, c1.weight, c1.bias, bn1.weight, stats, bsum)
    run()
    rec["dgrad_ms"] = [timed(run, a.steps) for _ in range(a.repeats)]
    rec["dgrad_bytes"] = {"x": x0.numel() * 4, "dp1h": dp1h.numel() * 2, "idx1": idx1.numel(), "dx": x0.numel() * 4}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
