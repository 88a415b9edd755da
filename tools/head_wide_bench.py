"""Wide fused head (11 .. 64 classes, csrc/kernels/head_wide.hip): the kernels alone and the training step.

Per class count: the head forward and backward alone (device events around ``--iters`` calls after a
warm-up) with the bytes they must move per second -- forward: the fc weight and ya read once; backward:
the weight and ya read, the weight (update-only step) and g2m written -- then the whole training step
at ``--image-size``, batch ``--batch-size``, on the fused plan against ``mode="layers"`` (what a model
of more than ten classes ran before the wide head), alternating ``--repeats`` times in one process.
``--ten`` adds the ten-class head's forward on the same box (the yardstick of the stream rate).
``--update`` adds the pooled exchange's fc step alone (``ops.head_update_pooled``, mode 0: the weight
read and written, every rank's ya read) from one and from two ranks' inputs, the second rank's ya a copy
of the first's.  Prints one JSON line.

    python tools/head_wide_bench.py --classes 26 62
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, iters, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _head_alone(ops, dev, H, B, NC, iters):
    """(forward ms, backward ms, forward bytes, backward bytes) of the head ops on random ya / weight."""
    import torch

    P, Q = H // 2, H // 4
    K = 32 * Q * Q
    plane = ((Q + 3) // 4) * ((Q + 7) // 8) * 32
    ya = torch.randn(B, 32, plane, device=dev).half()
    wfc = torch.randn(NC, K, device=dev) * 0.01
    bfc, b2 = torch.zeros(NC, device=dev), torch.zeros(32, device=dev)
    aff2 = torch.cat([torch.ones(32, device=dev), torch.zeros(32, device=dev)])
    stats2 = torch.cat([torch.zeros(32, device=dev), torch.ones(32, device=dev)])
    dl = torch.randn(B, NC, device=dev) * 1e-3
    fwd_bytes = 4 * NC * K + 2 * B * 32 * plane
    bwd_bytes = 2 * 4 * NC * K + 2 * B * 32 * plane + 2 * B * K
    if NC <= 10:
        t_f = _timed(lambda: ops.fused_head_forward_aff(ya, aff2, b2, None, wfc, bfc, P, None), iters)
        t_b = _timed(lambda: ops.fused_head_backward(dl, ya, stats2, aff2, b2, None, wfc, P, None, 1.0, True, 1e-6,
                                                     keep_dw=False), iters)
    else:
        wmax = ops.fused_head_wide_forward_aff(ya, aff2, b2, None, wfc, bfc, P)[1]
        t_f = _timed(lambda: ops.fused_head_wide_forward_aff(ya, aff2, b2, None, wfc, bfc, P), iters)
        t_b = _timed(lambda: ops.fused_head_wide_backward(dl, ya, stats2, aff2, b2, None, wfc, wmax, P, None, 1.0, 1e-6,
                                                          keep_dw=False), iters)
    return t_f, t_b, fwd_bytes, bwd_bytes


def _update_alone(ops, dev, H, B, NC, W, iters):
    """(ms, bytes) of the pooled exchange's update-only fc step from W ranks' pooled inputs."""
    import torch

    P, Q = H // 2, H // 4
    K = 32 * Q * Q
    plane = ((Q + 3) // 4) * ((Q + 7) // 8) * 32
    ya_all = torch.randn(1, B, 32, plane, device=dev).half().repeat(W, 1, 1, 1)
    wfc = torch.randn(NC, K, device=dev) * 0.01
    aff2 = torch.cat([torch.ones(32, device=dev), torch.zeros(32, device=dev)])
    rec_all = ops.head_pooled_record(aff2, torch.zeros(32, device=dev), None).repeat(W, 1)
    dl = torch.randn(W * B, NC, device=dev) * 1e-3
    t = _timed(lambda: ops.head_update_pooled(dl, ya_all, rec_all, wfc, None, P, 1.0 / W, 1e-6, 0), iters)
    return t, 2 * 4 * NC * K + 2 * W * B * K


def _stepper(dev, H, B, NC, mode, lr):
    import torch

    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.ops import functional as TF

    torch.manual_seed(0)
    model = ConvNet(num_classes=NC, image_shape=(H, H), device=dev, mode=mode)
    opt = SGD(model.parameters(), lr)
    crit = CrossEntropyLoss()
    src = torch.randint(0, 256, (B, 28, 28), dtype=torch.uint8, device=dev)
    x = TF.upsample_bilinear_u8(src, H, H, levels=True)
    y = torch.randint(0, NC, (B,), device=dev)

    def step():
        loss = crit(model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()

    return step


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image-size", type=int, default=3000)
    ap.add_argument("--batch-size", type=int, default=5)
    ap.add_argument("--classes", type=int, nargs="+", default=[26, 62])
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--iters", type=int, default=20, help="calls per timing of the head alone")
    ap.add_argument("--steps", type=int, default=5, help="training steps per timing")
    ap.add_argument("--repeats", type=int, default=3, help="alternations fused / layers")
    ap.add_argument("--ten", action="store_true", help="also time the ten-class head alone")
    ap.add_argument("--no-step", action="store_true", help="the head alone only")
    ap.add_argument("--update", action="store_true", help="also time the pooled exchange's fc step (W = 1, 2)")
    a = ap.parse_args(argv)
    import torch

    import torch_distributed_sandbox_amd as tds

    if not torch.cuda.is_available():
        raise SystemExit("head_wide_bench: needs a GPU (a timing has no CPU fallback)")
    ops = tds._ext.ops()
    dev = torch.device("cuda", 0)
    H, B = a.image_size, a.batch_size
    rec = {"metric": "head_wide_bench", "image_size": H, "batch_size": B, "device": torch.cuda.get_device_name(dev),
           "classes": {}}
    for NC in ([10] if a.ten else []) + list(a.classes):
        t_f, t_b, by_f, by_b = _head_alone(ops, dev, H, B, NC, a.iters)
        r = {"head_fwd_ms": t_f, "head_fwd_tb_per_s": by_f / t_f / 1e9, "head_bwd_update_only_ms": t_b,
             "head_bwd_tb_per_s": by_b / t_b / 1e9}
        if a.update:
            for W in (1, 2):
                t_u, by_u = _update_alone(ops, dev, H, B, NC, W, a.iters)
                r[f"update_pooled_w{W}_ms"], r[f"update_pooled_w{W}_tb_per_s"] = t_u, by_u / t_u / 1e9
        torch.cuda.empty_cache()
        if NC > 10 and not a.no_step:
            fused, layers = [], []
            for _ in range(a.repeats):  # (fresh models each round: the two plans never hold memory together)
                for mode, out in (("fused", fused), ("layers", layers)):
                    step = _stepper(dev, H, B, NC, mode, a.lr)
                    out.append(_timed(step, a.steps, warmup=2))
                    del step
                    torch.cuda.empty_cache()
            r["step_fused_ms"], r["step_layers_ms"] = fused, layers
        rec["classes"][str(NC)] = r
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
