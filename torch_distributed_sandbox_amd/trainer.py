"""Training loops behind ``mnist_onegpu.py`` and ``mnist_distributed.py``.

Reference loops: mnist_onegpu.py:34-84 (single GPU) and
mnist_distributed.py:48-109 (DDP); SURVEY.md §3.3-§3.4.  Kept: seed 0 before
model construction, ConvNet topology, bs=5, SGD(lr=1e-4), CE loss,
``zero_grad -> backward -> step`` order, the log lines (every 100 steps on
local GPU 0, rank-local loss) and ``Training complete in: ...``.  Added:
images/sec, peak memory, ``--max-steps``, synthetic on-device data, optional
global-average loss (the reference's commented-out ``all_reduce(AVG)``,
mnist_distributed.py:102), checkpoint/resume, fault injection, and a held-out
evaluation after the last epoch (``--eval-size``, :func:`evaluate`; the
reference never evaluates its model).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import time
from datetime import datetime

import torch

from . import _ext
from .data import DeviceUpsampleLoader, SyntheticMNIST
from .models import ConvNet, convnet_fused
from .ops import CrossEntropyLoss, SGD
from .ops import functional as TF
from .parallel import DistributedDataParallel, DistributedSampler
from .parallel import distributed as tdist
from .parallel.factored import EXCHANGE_SOURCES
from .utils import checkpoint, fault
from .utils.timing import StepTimer


def add_common_args(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    p.add_argument("--epochs", default=2, type=int, metavar="N", help="number of total epochs to run")
    p.add_argument("--image-size", default=3000, type=int, help="square image edge (reference: 3000)")
    p.add_argument("--batch-size", default=5, type=int, help="per-GPU batch size (reference: 5)")
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--momentum", default=0.0, type=float, help="SGD momentum (0: plain SGD, the reference)")
    p.add_argument("--weight-decay", default=0.0, type=float, help="SGD weight decay")
    p.add_argument("--dampening", default=0.0, type=float, help="SGD dampening of the momentum")
    p.add_argument("--nesterov", action="store_true", help="Nesterov momentum (needs --momentum > 0, no dampening)")
    p.add_argument("--max-steps", default=0, type=int, help="stop after this many steps per epoch (0 = full epoch)")
    p.add_argument("--dataset-size", default=60000, type=int, help="synthetic MNIST size (reference: 60000)")
    p.add_argument("--log-interval", default=100, type=int)
    p.add_argument("--mode", default="auto", choices=["auto", "fused", "layers"], help="ConvNet execution plan")
    p.add_argument("--input", default="levels", choices=["levels", "fp32"],
                   help="batches as the resized images' uint8 levels (ToTensor's 1/255 folded into conv1) or as "
                        "the materialised fp32 ToTensor image")
    p.add_argument("--device", default="auto", choices=["auto", "cuda", "cpu"])
    p.add_argument("--checkpoint", default="", help="save a checkpoint here at the end (rank 0)")
    p.add_argument("--resume", default="", help="resume from this checkpoint")
    p.add_argument("--json", action="store_true", help="print a JSON summary line at the end")
    p.add_argument("--grad-exchange", default="auto", choices=["auto", "allreduce", "activations", "sharded", "chunked"],
                   help="DDP gradient path of the big fc layer (parallel/factored.py)")
    p.add_argument("--exchange-source", default="pooled", choices=list(EXCHANGE_SOURCES),
                   help="what the fc exchange sends: the fused head's pooled input (activation path), the fc input "
                        "rows, or the pooled input on the sharded path too (parallel/factored.py)")
    p.add_argument("--phase-times", action="store_true",
                   help="time forward / backward / optimizer per step with HIP events (utils/timing.StepTimer; "
                        "adds them to the summary; roctx ranges with TDS_ROCTX=1)")
    p.add_argument("--overlap-optimizer", action=argparse.BooleanOptionalAction, default=True,
                   help="finish the fc bucket (collective + SGD) on a side stream under the next forward")
    p.add_argument("--bucket-mb", default=None, type=float, help="DDP bucket cap (MB, default 25 like torch)")
    p.add_argument("--reserve-cus", default=None, type=int,
                   help="rccl-native: CUs split off for the collectives (multiple of 32; default 32 at world > 1)")
    p.add_argument("--eval-size", default=0, type=int, metavar="N",
                   help="evaluate on N held-out samples (SyntheticMNIST split='test') after the last epoch "
                        "(0 = no evaluation)")
    p.add_argument("--eval-batch-size", default=None, type=int,
                   help="per-GPU batch size of the evaluation (default: --batch-size)")
    return p


def resolve_backend(args) -> str:
    """--backend, or the tuned default (parallel.distributed.default_backend): rccl-native on
    the GPU -- the stack bench.py measures -- and gloo on the CPU."""
    b = getattr(args, "backend", None)
    if b in (None, "auto"):
        on_gpu = args.device != "cpu" and torch.cuda.is_available()
        return tdist.default_backend(on_gpu)
    return tdist._normalise_backend(b)


def _device(args, gpu: int) -> torch.device:
    want = args.device
    if want == "auto":
        want = "cuda" if torch.cuda.is_available() else "cpu"
    if want == "cuda":
        torch.cuda.set_device(gpu)
        _ext.ops()  # fail loudly if the native extension is missing on a GPU box
        return torch.device("cuda", gpu)
    return torch.device("cpu")


def _real_samples(loader):
    """How many of the samples ``loader`` yields on this rank are real: a DistributedSampler pads
    the index list by wrapping to a multiple of the world size, and rank r takes positions r, r + W,
    ... of it, so its positions >= n -- the tail of what it yields -- repeat early samples.  None:
    no padding (no sampler, or drop_last)."""
    s = getattr(loader, "sampler", None)
    if s is None or not hasattr(s, "num_replicas") or getattr(s, "drop_last", False):
        return None
    return max(0, math.ceil((s.n - s.rank) / s.num_replicas))


def evaluate(model, loader, device, group=None) -> dict:
    """Loss and accuracy of ``model`` over ``loader`` in eval mode under ``no_grad``:
    ``{"eval_loss": mean cross-entropy per sample, "eval_accuracy": correct / samples,
    "eval_samples", "eval_images_per_sec"}``, the same dict on every rank.

    A DDP wrapper is unwrapped after its deferred updates landed; at world size > 1 rank 0's BN
    buffers (the authoritative running statistics) are broadcast first.  Under an initialised
    process group every rank evaluates its shard (a ``DistributedSampler(shuffle=False)`` over the
    test split; the padded tail is dropped, so every sample counts once) and the sums are added with
    one all-reduce.  On the GPU the per-batch metrics are one small launch into a device accumulator
    (``ops.eval_metrics``) read once at the end -- no host synchronisation per batch; eval-mode
    ``no_grad`` GPU forwards run the fused inference plan unless the model's mode is ``layers``."""
    device = torch.device(device)
    world = tdist.get_world_size(group) if tdist.is_initialized() else 1
    module = model
    if isinstance(model, DistributedDataParallel):
        model.wait_pending_updates()
        module = model.module
        if model.world_size > 1:
            model._broadcast_buffers_now()  # rank 0's running statistics (the wrapper's C6 broadcast), once
    on_gpu = device.type == "cuda"
    limit = _real_samples(loader)
    was_training = module.training
    module.eval()
    try:
        with torch.no_grad():
            if on_gpu:
                acc = torch.zeros(3, dtype=torch.int64, device=device)  # [fp64 loss sum bits, correct, samples]
                torch.cuda.synchronize(device)
            else:
                sums = torch.zeros(3, dtype=torch.float64)
            t0 = time.perf_counter()
            seen = 0
            for images, labels in loader:
                if limit is not None:
                    if seen >= limit:
                        break
                    if seen + images.shape[0] > limit:
                        images, labels = images[: limit - seen], labels[: limit - seen]
                seen += images.shape[0]
                logits = module(images)
                if on_gpu:
                    _ext.ops().eval_metrics(logits.float().contiguous(), labels.contiguous(), acc)
                else:
                    sums[0] += torch.nn.functional.cross_entropy(logits.double(), labels, reduction="sum")
                    sums[1] += (logits.argmax(dim=1) == labels).sum()
                    sums[2] += labels.numel()
            if on_gpu:
                torch.cuda.synchronize(device)  # the evaluation's one wait for the device
                sums = torch.cat([acc[:1].view(torch.float64), acc[1:].to(torch.float64)])
            dt = time.perf_counter() - t0
            # this rank's wall time rides along, so every rank reports the same rate (the ranks' mean time)
            sums = torch.cat([sums, torch.tensor([dt], dtype=torch.float64, device=sums.device)])
            if world > 1:
                tdist.all_reduce(sums, tdist.ReduceOp.SUM, group=group)
            loss_sum, correct, count, dt = sums.tolist()
            dt /= world
    finally:
        module.train(was_training)
    count = int(count)
    return {"eval_loss": loss_sum / count if count else float("nan"),
            "eval_accuracy": correct / count if count else float("nan"),
            "eval_samples": count,
            "eval_images_per_sec": count / dt if dt > 0 else float("nan")}


def train(gpu: int, args, distributed: bool = False) -> dict:
    rank = 0
    world = 1
    if distributed:
        rank = args.nr * args.gpus + gpu
        world = args.world_size
        backend = resolve_backend(args)
        dev_backend = tdist.is_device_backend(backend)
        # the same stack bench.py measures: rccl-native + C++ reducer + the compute/comm CU split
        tdist.init_process_group(backend=backend, world_size=world, rank=rank,
                                 device_id=gpu if dev_backend else None,
                                 comm_cus=getattr(args, "reserve_cus", None) if backend == "rccl-native" else None)
    device = _device(args, gpu)
    torch.manual_seed(0)
    H = W = args.image_size
    model = ConvNet(image_shape=(H, W), device=device, mode=args.mode)
    batch_size = args.batch_size
    criterion = CrossEntropyLoss()
    opt_args = {"momentum": float(getattr(args, "momentum", 0.0)), "weight_decay": float(getattr(args, "weight_decay", 0.0)),
                "dampening": float(getattr(args, "dampening", 0.0)), "nesterov": bool(getattr(args, "nesterov", False))}
    optimizer = SGD(model.parameters(), args.lr, **opt_args)
    if distributed or device.type == "cuda":
        # the tuned plan bench.py measures, also for the single-GPU script: at world size 1 the
        # wrapper owns the flat parameter / gradient buffers (one SGD sweep over the small
        # parameters), fuses the fc weight's SGD step into the head backward kernel
        # (ops/fused_update.py) and finishes the rest under the next forward (overlap_optimizer)
        # -- the reference's mnist_onegpu.py has no wrapper and steps all 180 M parameters in a
        # separate pass
        model = DistributedDataParallel(model, device_ids=[gpu] if device.type == "cuda" else None,
                                        bucket_cap_mb=getattr(args, "bucket_mb", None),
                                        grad_exchange=getattr(args, "grad_exchange", "auto"),
                                        exchange_source=getattr(args, "exchange_source", "pooled"),
                                        overlap_optimizer=getattr(args, "overlap_optimizer", True))
        model.attach_optimizer(optimizer)
    start_epoch = 0
    if args.resume:
        _, start_epoch, _ = checkpoint.load(args.resume, model, optimizer, map_location=device)
    dataset = SyntheticMNIST(size=args.dataset_size)
    levels = getattr(args, "input", "levels") == "levels"
    fused_plan = getattr(args, "mode", "auto") != "layers"
    moments = levels and fused_plan  # the fused plan reads them
    if distributed:
        sampler = DistributedSampler(len(dataset), num_replicas=world, rank=rank)
        loader = DeviceUpsampleLoader(dataset, batch_size, (H, W), device, sampler=sampler, levels=levels,
                                      moments=moments)
    else:
        loader = DeviceUpsampleLoader(dataset, batch_size, (H, W), device, shuffle=True, levels=levels,
                                      moments=moments)

    start = datetime.now()
    total_step = len(loader)
    if args.max_steps:
        total_step = min(total_step, args.max_steps)
    steps_done = 0
    t_first = None
    loss = None
    timer = StepTimer(enabled=getattr(args, "phase_times", False) and device.type == "cuda")
    for epoch in range(start_epoch, args.epochs):
        loader.set_epoch(epoch)
        for i, (images, labels) in enumerate(loader):
            if args.max_steps and i >= args.max_steps:
                break
            fault.maybe_inject(rank, steps_done)
            with timer.phase("forward"):
                if fused_plan and images.is_cuda:
                    # (fused plan: the loss and dlogits formed by the head forward with the logits)
                    convnet_fused.attach_labels(images, labels)
                outputs = model(images)
                loss = criterion(outputs, labels)
            optimizer.zero_grad()
            with timer.phase("backward"):
                TF.backward(loss)
            with timer.phase("optimizer"):
                optimizer.step()
            if distributed:
                # the reference builds a group every step (mnist_distributed.py:99-100); cached here
                tdist.new_group(ranks=list(range(args.gpus)) if args.nodes == 1 else None)
            steps_done += 1
            if steps_done == 1 and device.type == "cuda":
                torch.cuda.synchronize()
                t_first = time.perf_counter()
            if (i + 1) % args.log_interval == 0:
                shown = loss.detach()
                if distributed and getattr(args, "avg_loss", False):
                    # collective: every rank joins, rank 0 prints
                    shown = shown.clone()
                    tdist.all_reduce(shown, tdist.ReduceOp.AVG)
                if gpu != 0:
                    pass
                elif distributed:
                    print("Rank [{}], Epoch [{}/{}], Step [{}/{}], Loss: {:.4f}".format(
                        rank, epoch + 1, args.epochs, i + 1, total_step, shown.item()), flush=True)
                else:
                    print("Epoch [{}/{}], Step [{}/{}], Loss: {:.4f}".format(
                        epoch + 1, args.epochs, i + 1, total_step, shown.item()), flush=True)
    if hasattr(model, "wait_pending_updates"):
        model.wait_pending_updates()  # the last step's deferred fc update (ops/param_fence.py)
    if device.type == "cuda":
        torch.cuda.synchronize()
    t_end = time.perf_counter()
    summary = {"rank": rank, "world_size": world, "steps": steps_done, "batch_size": batch_size,
               "image_size": H, "final_loss": float(loss.item()) if loss is not None else None,
               "lr": float(args.lr), **opt_args,
               "plan": (f"DDP wrapper ({getattr(model, 'reducer_kind', '?')} reducer, fc grad "
                        f"{model.fc_grad_path()}, overlap_optimizer={model.overlap_optimizer})"
                        if isinstance(model, DistributedDataParallel) else "plain module"),
               "store": tdist.store_kind() if distributed else None}
    if t_first is not None and steps_done > 1:
        dt = t_end - t_first
        summary["images_per_sec_per_rank"] = (steps_done - 1) * batch_size / dt
        summary["images_per_sec_global"] = summary["images_per_sec_per_rank"] * world
        summary["ms_per_step"] = 1e3 * dt / (steps_done - 1)
    if device.type == "cuda":
        summary["peak_mem_gb"] = torch.cuda.max_memory_allocated(device) / 1e9
    if getattr(args, "phase_times", False):
        summary["phases"] = timer.summary()
    took = datetime.now() - start
    ev = None
    if getattr(args, "eval_size", 0) > 0:
        test = SyntheticMNIST(size=args.eval_size, split="test")
        tsampler = DistributedSampler(len(test), num_replicas=world, rank=rank, shuffle=False) if distributed else None
        tloader = DeviceUpsampleLoader(test, getattr(args, "eval_batch_size", None) or batch_size, (H, W), device,
                                       sampler=tsampler, levels=levels)
        ev = evaluate(model, tloader, device)
        summary.update(ev)
    if gpu == 0:
        print("Training complete in: " + str(took), flush=True)
        if ev is not None:
            print("Test Accuracy: {:.2f} %, Test Loss: {:.4f} ({} images)".format(
                100.0 * ev["eval_accuracy"], ev["eval_loss"], ev["eval_samples"]), flush=True)
        if args.json:
            print(json.dumps(summary), flush=True)
    if args.checkpoint:
        checkpoint.save(args.checkpoint, model, optimizer, step=steps_done, epoch=args.epochs, rank=rank)
    if distributed:
        tdist.barrier()
        tdist.destroy_process_group()
    return summary
