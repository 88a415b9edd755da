#!/usr/bin/env python
"""Inference-plan measurements on the MI355X, one JSON line per run.

Per shape (``--image-size``, ``--batch-size``), with HIP events and the warm-up excluded:

* ``fused``: ms per batch and peak memory of the eval-mode ``no_grad`` forward under ``mode="auto"``
  (the inference plan, models/convnet_fused.py ``forward_inference``);
* ``layers``: the same for ``mode="layers"`` (the exact-fp32 generic path: what every eval forward ran
  before the inference plan existed);
* ``conv2``: the isolated inference conv2 launch (``ops.fused_conv2_forward_inference``) beside the
  training launch (``ops.fused_conv2_forward_bn``) on the same p1, packed weights and gamma2.

With ``--precision fp8`` the FP8 (E4M3) conv2 of ``ConvNet(inference_precision="fp8")`` is measured beside
the TF32-class one: ``fused_fp8`` (the whole eval forward, its windows alternating with ``fused``'s) and
``conv2.fp8_ms`` (``ops.fused_conv2_forward_inference_fp8`` on the same p1, alternating with the other two).

With ``--fc-precision fp16 fp8`` the inference head on a packed fc weight (``ConvNet(inference_fc_precision=...)``,
csrc/kernels/head_inf.hip) is measured beside the default: ``fused_fc_<kind>`` (the whole eval forward with the
pack cached, alternating with ``fused``; its peak memory includes the pack) and ``head`` (the head launch alone:
``ops.fused_head_forward_inference`` per kind beside the training head on the fp32 weight, on the same ya, and
the one-time ``ops.fc_pack_inference``).  ``--num-classes`` sets the fc width.

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
    ap.add_argument("--precision", default="tf32", choices=["tf32", "fp8"],
                    help="fp8: also measure the FP8 conv2 (forward and isolated launch) beside the TF32-class one")
    ap.add_argument("--fc-precision", nargs="*", default=[], choices=["fp16", "fp8"],
                    help="also measure the inference head on a packed fc weight of these kinds beside the fp32 head")
    ap.add_argument("--num-classes", type=int, default=10)
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
    model = ConvNet(num_classes=a.num_classes, image_shape=(H, H), device=dev, mode="auto").eval()
    # (the fp32 head takes 11 .. 64 classes with at most 16 images: above that only the packed kinds are measured)
    fp32_head = a.num_classes <= 10 or B <= 16
    if not fp32_head and not a.fc_precision:
        raise SystemExit("eval_bench: more than 10 classes with more than 16 images needs --fc-precision")
    if not fp32_head:
        a.skip_layers = True
        if a.precision == "fp8":
            raise SystemExit("eval_bench: --precision fp8 is measured beside the fp32 head (<= 16 images above 10 classes)")
    src = torch.randint(0, 256, (B, 28, 28), dtype=torch.uint8, device=dev)
    x = TF.upsample_bilinear_u8(src, H, H, levels=a.input == "levels")

    def forward():
        with torch.no_grad():
            return model(x)

    rec = {"metric": "eval_bench", "image_size": H, "batch_size": B, "input": a.input, "iters": a.iters,
           "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(dev)}
    fp8 = a.precision == "fp8"
    fused_ms, layers_ms, fp8_ms = [], [], []
    fc_ms = {k: [] for k in a.fc_precision}
    for _ in range(a.repeats):  # the arms alternate
        model.mode = "auto"
        if fp32_head:
            fused_ms.append(_time(forward, a.iters, a.warmup))
        for k in a.fc_precision:
            model.inference_fc_precision = k
            fc_ms[k].append(_time(forward, a.iters, a.warmup))
            model.inference_fc_precision = "fp32"
        if fp8:
            model.inference_precision = "fp8"
            fp8_ms.append(_time(forward, a.iters, a.warmup))
            model.inference_precision = "tf32"
        if not a.skip_layers:
            model.mode = "layers"
            layers_ms.append(_time(forward, max(2, a.iters // 4), 1))
    model.mode = "auto"
    if fp32_head:
        rec["fused"] = {"ms_per_batch": fused_ms, "peak_mem_bytes": _peak(forward, dev)}
    for k in a.fc_precision:
        model.inference_fc_precision, model._fc_pack = k, None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        forward()  # packs
        torch.cuda.synchronize()
        pack_bytes = torch.cuda.memory_allocated(dev) - base
        rec["fused_fc_" + k] = {"ms_per_batch": fc_ms[k], "pack_bytes": pack_bytes,
                                "peak_mem_bytes": pack_bytes + _peak(forward, dev)}
        if fp32_head:
            rec["fused_fc_" + k]["vs_fp32_forward"] = min(fc_ms[k]) / min(fused_ms)
        model.inference_fc_precision, model._fc_pack = "fp32", None
    if fp8:
        model.inference_precision = "fp8"
        rec["fused_fp8"] = {"ms_per_batch": fp8_ms, "peak_mem_bytes": _peak(forward, dev)}
        model.inference_precision = "tf32"
        rec["fp8_vs_tf32_forward"] = min(fp8_ms) / min(fused_ms)
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

    if a.fc_precision:  # the head launch alone, on the inference plan's own ya of this batch
        fc = model.fc
        _, aff2 = ops.inference_constants(x, conv1.weight, conv1.bias, bn1.weight, bn1.bias, bn1.running_mean,
                                          bn1.running_var, float(bn1.eps), bn2.weight, bn2.bias, bn2.running_mean,
                                          bn2.running_var, float(bn2.eps), mag)
        ya = ops.fused_conv2_forward_inference(p1, wp, bn2.weight, mag)

        def head_fp32():
            if a.num_classes > 10:
                return ops.fused_head_wide_forward_aff(ya, aff2, conv2.bias, mag, fc.weight, fc.bias, P)[0]
            return ops.fused_head_forward_aff(ya, aff2, conv2.bias, mag, fc.weight, fc.bias, P, None)

        packs = {k: ops.fc_pack_inference(fc.weight.detach(), P, k) for k in a.fc_precision}
        heads = {k: (lambda k=k: ops.fused_head_forward_inference(ya, aff2, conv2.bias, mag, packs[k][0], packs[k][1],
                                                                  fc.bias, P, a.num_classes, k))
                 for k in a.fc_precision}
        head = {"fp32_ms": [], **{k + "_ms": [] for k in a.fc_precision}, **{k + "_pack_ms": [] for k in a.fc_precision}}
        for _ in range(a.repeats):
            if fp32_head:
                head["fp32_ms"].append(_time(head_fp32, a.iters, a.warmup))
            for k in a.fc_precision:
                head[k + "_ms"].append(_time(heads[k], a.iters, a.warmup))
                head[k + "_pack_ms"].append(_time(lambda k=k: ops.fc_pack_inference(fc.weight.detach(), P, k), 2, 1))
        if fp32_head:
            want = head_fp32().double()
            for k in a.fc_precision:
                head[k + "_vs_fp32"] = min(head[k + "_ms"]) / min(head["fp32_ms"])
                head[k + "_rel_l2_vs_fp32_head"] = ((heads[k]().double() - want).norm() / want.norm()).item()
        rec["head"] = head
        del packs

    if fp8:  # (a timing: mag keeps the TF32-class pack's store factor for the other two launches; p1's FP8 scale is in it)
        wp8, wexp = ops.conv2_pack_fp8(conv2.weight.detach(), None)

    def conv2_fp8():
        return ops.fused_conv2_forward_inference_fp8(p1, wp8, wexp, bn2.weight, mag)

    inf_ms, train_ms, c8_ms = [], [], []
    for _ in range(a.repeats):
        inf_ms.append(_time(conv2_inf, a.iters, a.warmup))
        train_ms.append(_time(conv2_train, a.iters, a.warmup))
        if fp8:
            c8_ms.append(_time(conv2_fp8, a.iters, a.warmup))
    same = torch.equal(conv2_inf().view(torch.int16), conv2_train()[1].view(torch.int16))
    rec["conv2"] = {"inference_ms": inf_ms, "training_ms": train_ms, "ya_bit_identical": bool(same),
                    "inference_vs_training": min(inf_ms) / min(train_ms)}
    if fp8:
        rec["conv2"]["fp8_ms"] = c8_ms
        rec["conv2"]["fp8_vs_inference"] = min(c8_ms) / min(inf_ms)
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
