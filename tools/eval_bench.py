#!/usr/bin/env python
"""Inference-plan measurements on the MI355X, one JSON line per run.

Per shape (``--image-size``, ``--batch-size``), with HIP events and the warm-up excluded:

* ``fused``: ms per batch and peak memory of the eval-mode ``no_grad`` forward under ``mode="auto"``
  (the inference plan, models/convnet_fused.py ``forward_inference``);
* ``layers``: the same for ``mode="layers"`` (the exact-fp32 generic path: what every eval forward ran
  before the inference plan existed);
* ``conv2``: the isolated inference conv2 launch (``ops.fused_conv2_forward_inference``) beside the
  training launch (``ops.fused_conv2_forward_bn``) on the same p1, packed weights and gamma2.

Every figure is a list over ``--repeats`` timed windows (each ``--iters`` calls), the two arms of a
comparison alternating inside a repeat.  Needs a GPU: there is no CPU fallback for a timing.

    python tools/eval_bench.py --image-size 3000 --batch-size 5
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time(fn, iters, warmup):
    """ms per call of fn over ``iters`` calls between two HIP events, after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _peak(fn, dev):
    """Peak bytes allocated above the level before the call (after a warming call)."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image-size", type=int, default=3000)
    ap.add_argument("--batch-size", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--input", default="levels", choices=["levels", "fp32"])
    ap.add_argument("--skip-layers", action="store_true", help="leave out the mode='layers' arm (sizes it cannot hold)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a GPU (a timing has no CPU fallback)")

    import torch_distributed_sandbox_amd as tds
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import functional as TF

    ops = tds._ext.ops()
    dev = torch.device("cuda", 0)
    H, B = a.image_size, a.batch_size
    torch.manual_seed(0)
    model = ConvNet(image_shape=(H, H), device=dev, mode="auto").eval()
    src = torch.randint(0, 256, (B, 28, 28), dtype=torch.uint8, device=dev)
    x = TF.upsample_bilinear_u8(src, H, H, levels=a.input == "levels")

    def forward():
        with torch.no_grad():
            return model(x)

    rec = {"metric": "eval_bench", "image_size": H, "batch_size": B, "input": a.input, "iters": a.iters,
           "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(dev)}
    fused_ms, layers_ms = [], []
    for _ in range(a.repeats):  # the arms alternate
        model.mode = "auto"
        fused_ms.append(_time(forward, a.iters, a.warmup))
        if not a.skip_layers:
            model.mode = "layers"
            layers_ms.append(_time(forward, max(2, a.iters // 4), 1))
    model.mode = "auto"
    rec["fused"] = {"ms_per_batch": fused_ms, "peak_mem_bytes": _peak(forward, dev)}
    if not a.skip_layers:
        model.mode = "layers"
        rec["layers"] = {"ms_per_batch": layers_ms, "peak_mem_bytes": _peak(forward, dev)}
        model.mode = "auto"
        rec["fused_vs_layers_time_ratio"] = min(layers_ms) / min(fused_ms)
        rec["fused_vs_layers_peak_ratio"] = rec["layers"]["peak_mem_bytes"] / max(1, rec["fused"]["peak_mem_bytes"])

    # the two conv2 forward launches on the same p1 (the inference plan's own p1 of this batch)
    conv1, bn1 = model.layer1[0], model.layer1[1]
    conv2, bn2 = model.layer2[0], model.layer2[1]
    P = H // 2
    mag = torch.empty(ops.mag_numel(B, P), dtype=torch.int32, device=dev)
    wp, _ = ops.conv2_pack(conv2.weight.detach(), mag, None, False)
    aff1, _ = ops.inference_constants(x, conv1.weight, conv1.bias, bn1.weight, bn1.bias, bn1.running_mean,
                                      bn1.running_var, float(bn1.eps), bn2.weight, bn2.bias, bn2.running_mean,
                                      bn2.running_var, float(bn2.eps), mag)
    p1 = ops.fused_l1_forward_inference(x, conv1.weight, conv1.bias, aff1)
    rm, rv = bn2.running_mean.clone(), bn2.running_var.clone()  # (the training launch updates its statistics)
    nbt = bn2.num_batches_tracked.clone()

    def conv2_inf():
        return ops.fused_conv2_forward_inference(p1, wp, bn2.weight, mag)

    def conv2_train():
        return ops.fused_conv2_forward_bn(p1, wp, conv2.bias, bn2.weight, bn2.bias, rm, rv, nbt, float(bn2.momentum),
                                          float(bn2.eps), mag)

    inf_ms, train_ms = [], []
    for _ in range(a.repeats):
        inf_ms.append(_time(conv2_inf, a.iters, a.warmup))
        train_ms.append(_time(conv2_train, a.iters, a.warmup))
    same = torch.equal(conv2_inf().view(torch.int16), conv2_train()[1].view(torch.int16))
    rec["conv2"] = {"inference_ms": inf_ms, "training_ms": train_ms, "ya_bit_identical": bool(same),
                    "inference_vs_training": min(inf_ms) / min(train_ms)}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
