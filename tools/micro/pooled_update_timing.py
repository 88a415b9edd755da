"""Time the pooled activation exchange's fc step (ops.head_update_pooled, mode 0) at the bench shape
for 1, 2 and 4 source ranks' gathered pooled inputs on one GPU (the W = 2 / 4 update of the default
exchange, parallel/factored.py "pooled"), with the bytes it moves and the rate.

--shard W also times, in the same run, the pooled sharded exchange's owner step
(ops.head_update_pooled_shard, mode 0): W source ranks' planes of rank 0's channels
(factored.plane_shards) past that shard of the weight, beside the full sweep over the same W ranks'
whole ya -- ms and effective GB/s for both.

  python tools/micro/pooled_update_timing.py [--ranks 1,2,4] [--iters 10] [--shard 8]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import torch_distributed_sandbox_amd as tds  # noqa: E402
from torch_distributed_sandbox_amd.parallel.factored import plane_shards  # noqa: E402


def _time(fn, iters):
    """Median over 5 windows of ``iters`` calls each, ms per call (device events)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / iters)
    return sorted(t)[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shard", type=int, default=0, metavar="W",
                    help="also time rank 0's shard update of a W-rank pooled sharded exchange (1 <= W <= 32)")
    a = ap.parse_args()
    if a.shard and not 1 <= a.shard <= 32:
        ap.error("--shard takes 1 <= W <= 32")
    ops = tds._ext.ops()
    dev = torch.device("cuda", 0)
    B, P, NC = 5, 1500, 10
    Q = P // 2
    pb = ((Q + 3) // 4 * 4) * ((Q + 7) // 8 * 8)
    w = torch.randn(NC, 32 * Q * Q, device=dev) * 0.01
    b2 = torch.zeros(32, device=dev)
    aff2 = torch.cat([torch.ones(32, device=dev), torch.zeros(32, device=dev)])
    rec = ops.head_pooled_record(aff2, b2, None)

    def full(nr):
        ya_all = torch.randn(nr, B, 32, pb, device=dev).half()
        rec_all = rec.expand(nr, 128).contiguous()
        dl = torch.randn(nr * B, NC, device=dev) * 1e-3
        ms = _time(lambda: ops.head_update_pooled(dl, ya_all, rec_all, w, None, P, 1.0 / nr, 1e-6, 0), a.iters)
        gb = (2 * w.numel() * 4 + ya_all.numel() * 2) / 1e9
        return ms, gb

    for nr in [int(v) for v in a.ranks.split(",")]:
        ms, gb = full(nr)
        print(f"ranks {nr}: {ms:.4f} ms  {gb:.2f} GB  {gb / ms:.2f} TB/s", flush=True)
    if a.shard:
        W = a.shard
        c0, c1 = plane_shards(W)[0]
        nc = c1 - c0
        ya_sh = torch.randn(W, B, nc, pb, device=dev).half()
        rec_all = rec.expand(W, 128).contiguous()
        dl = torch.randn(W * B, NC, device=dev) * 1e-3
        ms_s = _time(lambda: ops.head_update_pooled_shard(dl, ya_sh, rec_all, w, None, P, c0, c1, 1.0 / W, 1e-6, 0),
                     a.iters)
        # the shard's weight columns read and written once, every rank's planes of its channels read once
        gb_s = (2 * NC * nc * Q * Q * 4 + ya_sh.numel() * 2) / 1e9
        del ya_sh
        ms_f, gb_f = full(W)
        print(f"shard W={W} channels [{c0}, {c1}): {ms_s:.4f} ms  {gb_s * 1e3:.1f} MB  {gb_s / ms_s * 1e3:.1f} GB/s",
              flush=True)
        print(f"full sweep, {W} ranks:          {ms_f:.4f} ms  {gb_f * 1e3:.1f} MB  {gb_f / ms_f * 1e3:.1f} GB/s",
              flush=True)
        print(f"shard / full bandwidth: {(gb_s / ms_s) / (gb_f / ms_f):.2f}", flush=True)


if __name__ == "__main__":
    main()
