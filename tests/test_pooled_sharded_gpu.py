"""The sharded fc exchange from the fused head's pooled input (parallel/factored.py
``source="pooled-sharded"``): every rank sends owner s its ya planes of s's channels (fp16, no
encode, no counts), the owner forms those fc columns from all ranks' planes
(ops.head_update_pooled_shard) and the shards are all-gathered.

Multi-rank (without DDP's overlapped optimizer: under it the sharded path stays on the rows at
world > 1, factored._pooled_sharded_ok): gloo ranks share cuda:0 as in test_multirank_gpu.py; each
step is checked against the fp64 average of the ranks' reference gradients, and -- the owner sums ranks and images in the order
the full pooled sweep does -- bit for bit against the pooled activation exchange on the same data.
World 1 (rccl-native, forced): the whole GPU path against the plain fused plan."""
import copy
import os

import pytest
import torch
import torch.nn as nn

from _tf32ref import rel as _rel
from _tf32ref import tf32_convs
from test_model_gpu import RefConvNet, near_tie_windows

pytestmark = pytest.mark.gpu

B, STEPS, LR = 2, 2, 0.05
LABEL = "sharded-exchange(pooled)"
CONFIGS = (("sharded", "pooled-sharded"), ("activations", "pooled"))


def _data(world, H):
    g = torch.Generator().manual_seed(21)
    xs = torch.rand(STEPS, world, B, 1, H, H, generator=g)
    ys = torch.randint(0, 10, (STEPS, world, B), generator=g)
    return xs, ys


def _worker(rank, world, port, H, out):
    """Both configurations on the same data, one after the other in one process group."""
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    xs, ys = _data(world, H)
    recs = {}
    for mode, source in CONFIGS:
        torch.manual_seed(0)
        m = ConvNet(image_shape=(H, H), device=dev, mode="fused")
        ddp = DistributedDataParallel(m, grad_exchange=mode, overlap_optimizer=False, exchange_source=source)
        opt = ddp.attach_optimizer(SGD(m.parameters(), LR))
        crit = CrossEntropyLoss()
        rec = {"p0": {n: p.detach().cpu().clone() for n, p in m.named_parameters()},
               "b0": {n: b.detach().cpu().clone() for n, b in m.named_buffers()}, "steps": []}
        for s in range(STEPS):
            loss = crit(ddp(xs[s, rank].to(dev)), ys[s, rank].to(dev))
            opt.zero_grad()
            loss.backward()
            bufs = {n: b.detach().cpu().clone() for n, b in m.named_buffers()}
            opt.step()
            ddp.wait_pending_updates()
            torch.cuda.synchronize()
            grads = {n: None if p.grad is None else p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
            params = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
            rec["steps"].append({"loss": float(loss.item()), "grads": grads, "bufs": bufs, "params": params})
        rec["fc_grad"] = ddp.fc_grad_path()
        rec["zs_steps"] = ddp.exchanges[0].zs_stats["steps"]
        recs[source] = rec
        del ddp, opt, m
    torch.save(recs, os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _ref_step(H, params, bufs, x, y, tf32=False):
    """fp64 reference step of one rank's batch; ``tf32``: with TF32-operand convolutions, the
    reference's precision class (tests/_tf32ref.py)."""
    from torch_distributed_sandbox_amd.models import fc_in_features

    ref = RefConvNet(fc_in_features((H, H))).double()
    sd = {k: v.double() if v.is_floating_point() else v for k, v in {**params, **bufs}.items()}
    ref.load_state_dict(sd)
    if tf32:
        tf32_convs(ref)
    pool_in = []
    for pool in (ref.layer1[3], ref.layer2[3]):
        pool.register_forward_hook(lambda mod, inp, o: pool_in.append(inp[0].detach()))
    loss = nn.functional.cross_entropy(ref(x.double()), y)
    loss.backward()
    ties = sum(near_tie_windows(a) for a in pool_in)
    return ({n: p.grad for n, p in ref.named_parameters()}, dict(ref.named_buffers()), float(loss.detach()), ties)


def _check_fp64_average(recs, world, H):
    """The bounds of test_multirank_gpu.py's _check_two_ranks, for ``world`` ranks at edge H."""
    xs, ys = _data(world, H)
    params, bufs0 = recs[0]["p0"], recs[0]["b0"]
    for s in range(STEPS):
        avg, avg_t, ties = None, None, 0
        for r in range(world):
            g, rb, rl, t = _ref_step(H, params, bufs0, xs[s, r], ys[s, r])
            gt, tbuf, tl, _ = _ref_step(H, params, bufs0, xs[s, r], ys[s, r], tf32=True)
            ties += t
            avg = g if avg is None else {n: avg[n] + g[n] for n in avg}
            avg_t = gt if avg_t is None else {n: avg_t[n] + gt[n] for n in avg_t}
            assert abs(recs[r]["steps"][s]["loss"] - rl) < max(1e-4 * max(1.0, abs(rl)), 1.5 * abs(tl - rl)), (s, r)
            for n, b in recs[r]["steps"][s]["bufs"].items():  # rank-0 buffers + this rank's batch
                if b.is_floating_point():
                    et = (tbuf[n] - rb[n]).abs().max().item()
                    assert (b.double() - rb[n]).abs().max().item() < max(1e-4, 1.5 * et), (s, r, n)
                else:
                    assert int(b) == int(rb[n]), (s, r, n)
        avg = {n: v / world for n, v in avg.items()}
        avg_t = {n: v / world for n, v in avg_t.items()}
        for n in avg:
            g0 = recs[0]["steps"][s]["grads"][n]
            p1 = recs[0]["steps"][s]["params"][n]
            assert g0 is not None, (s, n)
            for r in range(1, world):  # every rank holds the same averaged gradient
                assert torch.equal(recs[r]["steps"][s]["grads"][n], g0), (s, n, r)
            ref_g = avg[n]
            if n.endswith("0.bias"):  # conv bias before BN: analytically zero, both sides noise
                wg = avg[n.replace("bias", "weight")].abs().max().item()
                assert (g0.double() - ref_g).abs().max().item() <= 1e-3 * wg + 1e-5, (s, n)
                continue
            rel = ((g0.double() - ref_g).norm() / ref_g.norm().clamp_min(1e-30)).item()
            flip_reach = n.startswith("layer1.") or n.startswith("layer2.0.")
            tol = max(2e-2 if ties and flip_reach else 2e-3, 1.5 * _rel(avg_t[n], ref_g))
            assert rel <= tol, (s, n, rel, tol, ties)
            for r in range(1, world):  # post-step parameters: identical on every rank
                assert torch.equal(recs[r]["steps"][s]["params"][n], p1), (s, n, r)
            assert torch.allclose(p1, params[n] - LR * g0, rtol=1e-6, atol=1e-7), (s, n)
        params = recs[0]["steps"][s]["params"]
        bufs0 = recs[0]["steps"][s]["bufs"]


@pytest.mark.parametrize("world,H", [(2, 256), (3, 260)])
def test_pooled_sharded_ranks(gpu, tmp_path, world, H):
    """W = 2 (16 channels each) and W = 3 at H = 260 (Q = 65: a partial 8-column block; uneven
    shards of 11 / 10 / 11 channels, factored.plane_shards)."""
    from torch_distributed_sandbox_amd.parallel import launch

    launch.spawn(_worker, args=(world, launch.find_free_port(), H, str(tmp_path)), nprocs=world, timeout=240)
    both = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    recs = [b["pooled-sharded"] for b in both]
    twin = both[0]["pooled"]
    assert all(r["fc_grad"] == LABEL and r["zs_steps"] == 0 for r in recs)
    assert twin["fc_grad"] == "activation-exchange(pooled)"
    _check_fp64_average(recs, world, H)
    # the pooled activation exchange on the same data: the same sums in the same order
    for s in range(STEPS):
        a, t = recs[0]["steps"][s], twin["steps"][s]
        for n in ("fc.weight", "fc.bias"):
            assert torch.equal(a["params"][n], t["params"][n]), (s, n, _where(a["params"][n], t["params"][n]))
            assert torch.equal(a["grads"][n], t["grads"][n]), (s, n, _where(a["grads"][n], t["grads"][n]))


def _where(a, b):
    """What differs between two tensors that should be equal (for the assertion message): how many
    elements, the largest difference, and the first and last differing flat positions."""
    d = (a != b).flatten().nonzero().flatten()
    return {"differ": int(d.numel()), "of": a.numel(), "max": float((a.double() - b.double()).abs().max()),
            "first": int(d[0]) if d.numel() else None, "last": int(d[-1]) if d.numel() else None}


def test_not_offered_under_overlapped_optimizer_at_world_gt_1(gpu):
    """DDP's overlapped optimizer hands the exchange its side stream; at world > 1 the sharded path
    then stays on the rows (the activation path keeps the pooled input), at world 1 it does not."""
    from torch_distributed_sandbox_amd.parallel import factored

    w = torch.nn.Parameter(torch.zeros(10, 32 * 16 * 16, device=gpu))
    for world, side, want in ((2, False, True), (2, True, False), (1, True, True)):
        ex = factored.ActivationExchange(w, None, None, world, "sharded", lambda on: None, lambda: None, None,
                                         source="pooled-sharded")
        ex.side_stream = torch.cuda.Stream(device=gpu) if side else None
        ex.arm(True)
        assert ex.pooled_capable() and ex.planned(2) == "sharded"
        assert ex.pooled(2) is want, (world, side)
        ex.detach()
    ex = factored.ActivationExchange(w, None, None, 2, "activations", lambda on: None, lambda: None, None,
                                     source="pooled-sharded")
    ex.side_stream = torch.cuda.Stream(device=gpu)
    ex.arm(True)
    assert ex.pooled(2)
    ex.detach()


# ---------------------------------------------------------------- world 1, forced (rccl-native)
@pytest.fixture(scope="module")
def pg(gpu):
    from torch_distributed_sandbox_amd.parallel import distributed as dist
    from torch_distributed_sandbox_amd.parallel import launch

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = launch.find_free_port()
    dist.init_process_group("rccl-native", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


H1 = 256  # fc: 10 x 131072 (exchange candidate)


def _ddp(m, **kw):
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    return DistributedDataParallel(m, grad_exchange="sharded", exchange_source="pooled-sharded", **kw)


def test_forced_world1_matches_plain_fused(pg, gpu):
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss

    torch.manual_seed(0)
    m = ConvNet(image_shape=(H1, H1), device=gpu, mode="fused")
    ref = copy.deepcopy(m)
    ddp = _ddp(m)
    assert len(ddp.exchanges) == 1 and ddp.exchanges[0].pooled_capable()
    opt = ddp.attach_optimizer(SGD(m.parameters(), 0.01))
    x = torch.rand(3, 1, H1, H1, device=gpu)
    y = torch.tensor([1, 2, 3], device=gpu)
    for step in range(2):
        loss = CrossEntropyLoss()(ddp(x), y)
        opt.zero_grad()
        loss.backward()
        ref.zero_grad()
        CrossEntropyLoss()(ref(x), y).backward()
        for (n, p), q in zip(m.named_parameters(), ref.parameters()):
            if n.endswith("0.bias"):
                continue
            rel = ((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30)).item()
            assert rel < 1e-5, (step, n, rel)
        assert m.fc.weight.grad.data_ptr() == ddp.grad_view(m.fc.weight).data_ptr()
        opt.step()
        with torch.no_grad():
            for p, q in zip(m.parameters(), ref.parameters()):
                q.copy_(p)
    ex = ddp.exchanges[0]
    assert ex.steps_exchanged == 2 and ddp.fc_grad_path() == LABEL
    assert ex.zs_stats["steps"] == 0  # nothing encoded, nothing counted


def test_forced_world1_no_sync_accumulates(pg, gpu):
    """A no_sync() step, then a synced one: the exchanged dW shard is added (the kernel's += mode)
    to the gradient accumulated locally, as the plain model accumulates the two backwards."""
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    torch.manual_seed(0)
    m = ConvNet(image_shape=(H1, H1), device=gpu, mode="fused")
    ref = copy.deepcopy(m)
    ddp = _ddp(m)
    x = torch.rand(3, 1, H1, H1, device=gpu)
    y = torch.tensor([1, 2, 3], device=gpu)
    crit = CrossEntropyLoss()
    ddp.zero_grad()
    ref.zero_grad()
    with ddp.no_sync():
        crit(ddp(x), y).backward()
    crit(ddp(x * 0.5), y).backward()
    crit(ref(x), y).backward()
    crit(ref(x * 0.5), y).backward()
    assert ddp.exchanges[0].steps_exchanged == 1 and ddp.fc_grad_path() == LABEL
    # (fp32 sums of a few terms on both sides, in another order: the bound of the two-step test)
    for p, q in ((m.fc.weight, ref.fc.weight), (m.fc.bias, ref.fc.bias)):
        rel = ((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30)).item()
        assert rel < 1e-5, rel


def test_forced_world1_overlap_matches_sequential(pg, gpu):
    """The update-only step (the owner updates its weight shard in place on the side stream, .grad
    stays None) against the sequential step of the same exchange."""
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss

    torch.manual_seed(0)
    m1 = ConvNet(image_shape=(H1, H1), device=gpu, mode="fused")
    m2 = copy.deepcopy(m1)
    d1 = _ddp(m1, overlap_optimizer=True, fuse_update_in_backward=True)
    d2 = _ddp(m2)
    assert d1.overlap_optimizer and len(d1._deferred) == 1
    o1 = d1.attach_optimizer(SGD(m1.parameters(), 1e-4))
    o2 = d2.attach_optimizer(SGD(m2.parameters(), 1e-4))
    crit = CrossEntropyLoss()
    g = torch.Generator(device=gpu).manual_seed(5)
    for step in range(4):
        x = torch.rand(3, 1, H1, H1, device=gpu, generator=g)
        y = torch.randint(0, 10, (3,), device=gpu, generator=g)
        for d, o in ((d1, o1), (d2, o2)):
            loss = crit(d(x), y)
            o.zero_grad()
            loss.backward()
            o.step()
        assert m1.fc.weight.grad is None and m2.fc.weight.grad is not None
        assert d1.fc_grad_path() == LABEL and d2.fc_grad_path() == LABEL
    d1.wait_pending_updates()
    torch.cuda.synchronize()
    assert d1.exchanges[0].zs_stats["steps"] == 0
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-9), n  # (p - lr*g in another kernel: fma contraction)


def test_preflight_lists_the_real_collectives(pg, gpu):
    from torch_distributed_sandbox_amd.models import ConvNet

    m = ConvNet(image_shape=(H1, H1), device=gpu, mode="fused")
    ddp = _ddp(m)
    seen = []

    def timed(name, nbytes, kind, issue):
        w = issue()
        if w is not None:
            w.wait()
        seen.append((name, nbytes, kind))

    rows, Q, NC = 3, H1 // 4, 10
    plane = ((Q + 3) // 4 * 4) * ((Q + 7) // 8 * 8)
    assert ddp.exchanges[0].preflight(rows, timed) == "sharded"
    torch.cuda.synchronize()
    # world 1: rank 0 owns all 32 channels.  The receive buffer of a step is W * B * nc * plane * 2 B
    assert seen == [
        ("head record all-gather", 128 * 4, "all_gather"),
        ("pooled input (ya) channel-shard exchange (per peer)", rows * 32 * plane * 2, "sendrecv"),
        ("dY all-gather", rows * NC * 4, "all_gather"),
        ("updated W shard exchange (per peer)", NC * 32 * Q * Q * 4, "sendrecv"),
    ]
