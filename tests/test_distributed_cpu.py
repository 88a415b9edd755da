"""Multi-process CPU tests (gloo, world_size 2-4) of the process-group API, DDP,
sampler, launcher fail-fast and fault injection."""
import copy
import os

import pytest
import torch

from torch_distributed_sandbox_amd.parallel import launch


def _init(rank, world, port, backend="gloo"):
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group(backend, rank=rank, world_size=world)
    return dist


# ---------------------------------------------------------------- collectives
def _w_collectives(rank, world, port, backend="gloo"):
    dist = _init(rank, world, port, backend)
    t = torch.tensor(rank + 1, dtype=torch.int32)
    g = dist.new_group(list(range(world)))
    assert g is dist.new_group(list(range(world)))  # cached, no per-step re-init
    dist.all_reduce(t, dist.ReduceOp.SUM, group=g)
    assert t.item() == world * (world + 1) // 2
    f = torch.full((5,), float(rank))
    dist.all_reduce(f, dist.ReduceOp.AVG)
    assert torch.allclose(f, torch.full((5,), (world - 1) / 2))
    m = torch.tensor([float(rank)])
    dist.all_reduce(m, dist.ReduceOp.MAX)
    assert m.item() == world - 1
    w = dist.all_reduce(torch.ones(3), dist.ReduceOp.AVG, async_op=True)
    w.wait()
    b = torch.tensor([rank * 10.0])
    dist.broadcast(b, src=world - 1)
    assert b.item() == (world - 1) * 10.0
    out = [torch.zeros(2) for _ in range(world)]
    dist.all_gather(out, torch.full((2,), float(rank)))
    assert [o[0].item() for o in out] == list(range(world))
    if world > 2:
        sub = dist.new_group([0, 1])
        if rank in (0, 1):
            s = torch.tensor([1.0])
            dist.all_reduce(s, group=sub)
            assert s.item() == 2.0
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "host"])
@pytest.mark.parametrize("world", [2, 3])
def test_collectives(world, backend):
    launch.spawn(_w_collectives, args=(world, launch.find_free_port(), backend), nprocs=world, timeout=180)


# ---------------------------------------------------------------- lifetime
@pytest.mark.parametrize("reducer", ["native", "python"])
def test_ddp_wrapper_and_model_are_collected(reducer):
    """Deleting the wrapper, the model and the optimizer after a training step frees them: the
    hooks, gradient sinks and fused-update providers attached to the parameters hold the wrapper
    weakly (parallel/ddp.py ``_weak_call``).  Round 6 found the cycle through the parameters' C++
    hooks keeping every earlier model's flat buffers alive (tools/oom_demo.py: 0.72 GB per
    ConvNet at 3000^2 on the GPU)."""
    import gc
    import weakref

    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    H = 64
    torch.manual_seed(0)
    m = ConvNet(image_shape=(H, H))
    ddp = DistributedDataParallel(m, reducer=reducer, overlap_optimizer=True)
    opt = ddp.attach_optimizer(SGD(m.parameters(), 0.05))
    x, y = torch.rand(2, 1, H, H), torch.randint(0, 10, (2,))
    opt.zero_grad()
    CrossEntropyLoss()(ddp(x), y).backward()
    opt.step()
    refs = [weakref.ref(o) for o in (m, ddp, ddp.flat_param, m.fc.weight)]
    del m, ddp, opt
    gc.collect()
    assert [r() is None for r in refs] == [True] * 4


# ---------------------------------------------------------------- lazy gradient slots
@pytest.mark.parametrize("reducer", ["native", "python"])
def test_big_layer_grad_slot_allocated_on_first_use(reducer):
    """The big fc layer's weight slot is the flat gradient layout's tail and gets storage only
    when a gradient is written there (parallel/ddp.py ``_lazy_from``; at world size 1 on the GPU
    the fused update never writes one, tests/test_fullscale_plan_gpu.py).  A plain backward grows
    the buffer once: every .grad is a view of the grown buffer, gradients and the flat SGD sweep
    match torch."""
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    H = 256  # fc 10 x 131072: an exchange candidate (>= 2^20 elements)
    torch.manual_seed(0)
    m = ConvNet(image_shape=(H, H))
    ref = copy.deepcopy(m)
    ddp = DistributedDataParallel(m, reducer=reducer)
    assert ddp.reducer_kind == reducer
    w = m.fc.weight
    o, n = ddp._slots[id(w)]
    assert o == ddp._lazy_from and o + n == ddp._total
    assert ddp.flat_grad.numel() == ddp._lazy_from
    assert ddp.grad_storage_bytes() < w.numel() * 4 // 10
    assert ddp.bucket_layout()[0][2] == [(10,), (10, 32 * (H // 4) ** 2)]  # ready order kept
    for p, q in zip(m.parameters(), ref.parameters()):
        assert torch.equal(p, q)
        assert p.data.untyped_storage().data_ptr() == ddp.flat_param.untyped_storage().data_ptr()
    opt = ddp.attach_optimizer(SGD(m.parameters(), 0.05))
    ropt = torch.optim.SGD(ref.parameters(), 0.05)
    crit = CrossEntropyLoss()
    g = torch.Generator().manual_seed(3)
    ptr = None
    for step in range(2):
        x = torch.rand(2, 1, H, H, generator=g)
        y = torch.randint(0, 10, (2,), generator=g)
        opt.zero_grad()
        crit(ddp(x), y).backward()
        fg = ddp.flat_grad
        assert fg.numel() == ddp._total
        ptr = fg.data_ptr() if ptr is None else ptr
        assert fg.data_ptr() == ptr  # grown once, in the first backward
        for p in m.parameters():
            assert p.grad.untyped_storage().data_ptr() == fg.untyped_storage().data_ptr()
        ropt.zero_grad()
        crit(ref(x), y).backward()
        for (nm, p), q in zip(m.named_parameters(), ref.parameters()):
            assert torch.allclose(p.grad, q.grad, rtol=1e-4, atol=1e-7), nm
        opt.step()
        ropt.step()
        for (nm, p), q in zip(m.named_parameters(), ref.parameters()):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), nm


# ---------------------------------------------------------------- DDP equivalence
def _w_ddp(rank, world, port, H, B, backend="gloo"):
    dist = _init(rank, world, port, backend)
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    base = ConvNet(image_shape=(H, H))
    ref = copy.deepcopy(base)  # rank-0 init (all ranks seeded 0)
    torch.manual_seed(100 + rank)
    model = ConvNet(image_shape=(H, H))  # different init per rank -> must be overwritten by rank 0
    model.load_state_dict(base.state_dict()) if rank == 0 else None
    ddp = DistributedDataParallel(model)
    # this package's host ring backend drives the C++ reducer; torch's gloo the Python hooks
    assert ddp.reducer_kind == ("native" if backend == "host" else "python")
    assert [b[2][0] for b in ddp.bucket_layout()][0] == (10,)  # fc.bias first (gradient-ready order)
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p.data, q.data), "rank-0 broadcast at construction failed"
    opt = ddp.attach_optimizer(SGD(model.parameters(), 0.05))
    ropt = torch.optim.SGD(ref.parameters(), 0.05)
    crit = CrossEntropyLoss()
    g = torch.Generator().manual_seed(7)
    for step in range(3):
        xs = torch.rand(world, B, 1, H, H, generator=g)
        ys = torch.randint(0, 10, (world, B), generator=g)
        loss = crit(ddp(xs[rank]), ys[rank])
        opt.zero_grad()
        loss.backward()
        # reference: average of per-rank gradients (per-rank BN stats), one process
        ropt.zero_grad()
        grads = None
        for r in range(world):
            rr = copy.deepcopy(ref)
            rl = torch.nn.functional.cross_entropy(rr(xs[r]), ys[r])
            rl.backward()
            gg = [p.grad.clone() for p in rr.parameters()]
            grads = gg if grads is None else [a + b for a, b in zip(grads, gg)]
            if r == 0:
                ref_buffers = [b.clone() for b in rr.buffers()]
        for p, gsum in zip(ref.parameters(), grads):
            p.grad = gsum / world
        for (n, p), q in zip(model.named_parameters(), ref.parameters()):
            assert torch.allclose(p.grad, q.grad, rtol=1e-4, atol=1e-6), (step, n)
        opt.step()
        ropt.step()
        with torch.no_grad():
            for b, rb in zip(ref.buffers(), ref_buffers):
                b.copy_(rb)  # buffers follow rank 0 (broadcast_buffers=True)
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-6)
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "host"])
def test_ddp_matches_single_process_average(backend):
    launch.spawn(_w_ddp, args=(2, launch.find_free_port(), 32, 2, backend), nprocs=2, timeout=300)


def _w_no_sync(rank, world, port, backend="gloo"):
    dist = _init(rank, world, port, backend)
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    lin = torch.nn.Linear(4, 3)
    ddp = DistributedDataParallel(lin)
    x = torch.full((2, 4), float(rank + 1))
    with ddp.no_sync():
        ddp(x).sum().backward()
    local = lin.weight.grad.clone()
    ddp(x).sum().backward()  # accumulates + syncs
    t = local * 2
    dist.all_reduce(t, dist.ReduceOp.AVG)
    assert torch.allclose(lin.weight.grad, t), (lin.weight.grad, t)
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "host"])
def test_ddp_no_sync_accumulation(backend):
    launch.spawn(_w_no_sync, args=(2, launch.find_free_port(), backend), nprocs=2, timeout=120)


def _w_unused(rank, world, port, find_unused):
    dist = _init(rank, world, port, "host")
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)

    class Two(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(4, 3)
            self.b = torch.nn.Linear(4, 3)  # never used in forward

        def forward(self, x):
            return self.a(x)

    m = Two()
    ddp = DistributedDataParallel(m, find_unused_parameters=find_unused, bucket_cap_mb=1e-5)
    assert ddp.reducer_kind == "native"
    x = torch.full((2, 4), float(rank + 1))
    if find_unused:
        ddp(x).sum().backward()
        assert torch.equal(m.b.weight.grad, torch.zeros_like(m.b.weight))
        expect = torch.full((3, 4), 2.0 * (1 + 2) / 2)  # d(sum)/dW = sum_b x, averaged over ranks
        assert torch.allclose(m.a.weight.grad, expect)
    else:
        with pytest.raises(RuntimeError, match="never became ready"):
            ddp(x).sum().backward()
    dist.destroy_process_group()


@pytest.mark.parametrize("find_unused", [True, False])
def test_native_reducer_unused_parameters(find_unused):
    launch.spawn(_w_unused, args=(2, launch.find_free_port(), find_unused), nprocs=2, timeout=120)


# ---------------------------------------------------------------- sampler
def test_distributed_sampler_matches_torch():
    from torch.utils.data.distributed import DistributedSampler as TorchDS

    from torch_distributed_sandbox_amd.parallel import DistributedSampler

    ds = list(range(23))
    for W in (1, 2, 3, 4):
        for r in range(W):
            for drop in (False, True):
                ours = DistributedSampler(len(ds), num_replicas=W, rank=r, drop_last=drop)
                theirs = TorchDS(ds, num_replicas=W, rank=r, drop_last=drop)
                for ep in (0, 1):
                    ours.set_epoch(ep)
                    theirs.set_epoch(ep)
                    assert list(ours) == list(theirs)
                    assert len(ours) == len(theirs)


# ---------------------------------------------------------------- launcher / faults
def _w_fault(rank, world, port, mode):
    os.environ.update({"TDS_FAULT_RANK": "1", "TDS_FAULT_STEP": "2", "TDS_FAULT_MODE": mode,
                       "TDS_FAULT_HANG_S": "60"})
    from torch_distributed_sandbox_amd.utils import fault

    dist = _init(rank, world, port)
    for step in range(5):
        fault.maybe_inject(rank, step)
        t = torch.ones(1)
        dist.all_reduce(t)


@pytest.mark.parametrize("mode", ["raise", "exit"])
def test_fail_fast_on_rank_fault(mode):
    with pytest.raises((launch.ProcessRaisedException, launch.ProcessExitedException)) as ei:
        launch.spawn(_w_fault, args=(2, launch.find_free_port(), mode), nprocs=2, timeout=120)
    assert ei.value.error_index == 1
    if mode == "raise":
        assert "injected fault on rank 1 at step 2" in str(ei.value)


def test_spawn_timeout_on_hang():
    with pytest.raises(TimeoutError):
        launch.spawn(_w_fault, args=(2, launch.find_free_port(), "hang"), nprocs=2, timeout=15)


def _w_ok(i, path):
    with open(os.path.join(path, f"r{i}"), "w") as f:
        f.write(str(i))


def test_spawn_runs_all(tmp_path):
    launch.spawn(_w_ok, args=(str(tmp_path),), nprocs=3, timeout=60)
    assert sorted(os.listdir(tmp_path)) == ["r0", "r1", "r2"]


def test_find_free_port():
    p = int(launch.find_free_port())
    assert 0 < p < 65536


# ---------------------------------------------------------------- activation exchange (parallel/factored.py)
def _w_exchange(rank, world, port, backend, H, B, mode="auto"):
    dist = _init(rank, world, port, backend)
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    m_ex = ConvNet(image_shape=(H, H))
    m_ar = copy.deepcopy(m_ex)
    d_ex = DistributedDataParallel(m_ex, grad_exchange=mode, allreduce_chunks=3 if mode == "chunked" else None)
    d_ar = DistributedDataParallel(m_ar, grad_exchange="allreduce")
    assert len(d_ex.exchanges) == 1 and not d_ar.exchanges
    # the fc layer owns bucket 0 alone in both layouts
    assert d_ex.bucket_layout()[0][2] == [(10,), (10, 32 * (H // 4) ** 2)]
    o_ex = d_ex.attach_optimizer(SGD(m_ex.parameters(), 0.05))
    o_ar = d_ar.attach_optimizer(SGD(m_ar.parameters(), 0.05))
    crit = CrossEntropyLoss()
    g = torch.Generator().manual_seed(11)
    for step in range(3):
        xs = torch.rand(world, B, 1, H, H, generator=g)
        ys = torch.randint(0, 10, (world, B), generator=g)
        if step:
            # re-align the replicas: each step compares one exchange against one all-reduce
            # (the updates' summation order differs, and at W=8 the drift of a chaotic model
            # alone would pass 1e-5 by step 2)
            with torch.no_grad():
                for p, q in zip(m_ex.parameters(), m_ar.parameters()):
                    q.copy_(p)
                for p, q in zip(m_ex.buffers(), m_ar.buffers()):
                    q.copy_(p)
        for d, o in ((d_ex, o_ex), (d_ar, o_ar)):
            loss = crit(d(xs[rank]), ys[rank])
            o.zero_grad()
            loss.backward()
        for (n, p), q in zip(m_ex.named_parameters(), m_ar.parameters()):
            if n.endswith("0.bias"):  # conv bias before BN: analytically zero, rounding noise both ways
                continue
            rel = ((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30)).item()
            assert rel < 1e-5, (step, n, rel)
        # gradient lives in the flat bucket, like every other DDP gradient
        assert m_ex.fc.weight.grad.data_ptr() == d_ex.grad_view(m_ex.fc.weight).data_ptr()
        o_ex.step()
        o_ar.step()
    assert d_ex.exchanges[0].steps_exchanged == 3
    assert d_ex.fc_grad_path() == {"sharded": "sharded-exchange(zs)", "chunked": "chunked-allreduce"}.get(
        mode, "activation-exchange(zs)")
    # accumulation: a no_sync step, then a synced step: the locally accumulated fc
    # gradient is all-reduced as it is and this step's exchanged average added
    with torch.no_grad():  # re-align the replicas (3 updates of a chaotic model drift at 1e-5)
        for p, q in zip(m_ex.parameters(), m_ar.parameters()):
            q.copy_(p)
        for p, q in zip(m_ex.buffers(), m_ar.buffers()):
            q.copy_(p)
    for d, o in ((d_ex, o_ex), (d_ar, o_ar)):
        o.zero_grad()
        with d.no_sync():
            crit(d(xs[rank]), ys[rank]).backward()
        crit(d(xs[rank] * 0.5), ys[rank]).backward()
    assert d_ex.exchanges[0].steps_exchanged == 4
    for (n, p), q in zip(m_ex.named_parameters(), m_ar.parameters()):
        if not n.endswith("0.bias"):
            rel = ((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30)).item()
            assert rel < 1e-5, ("accumulate", n, rel)
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "host"])
def test_activation_exchange_matches_allreduce(backend):
    # H = 232 -> fc.weight 10 x 107648 (> 1M elements: exchange candidate); W=2, B=2 -> exchange wins
    launch.spawn(_w_exchange, args=(2, launch.find_free_port(), backend, 232, 2), nprocs=2, timeout=300)


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("host", 3), ("gloo", 4), ("gloo", 8)])
def test_sharded_exchange_matches_allreduce(backend, world):
    """Column-sharded fc gradient (all-to-all of X shards, per-shard dW, all-gather of the
    shards) equals the bucket all-reduce average, including no_sync accumulation; gloo uses
    batched isend/irecv, the ring-only host backend the packed all-gather fallback."""
    launch.spawn(_w_exchange, args=(world, launch.find_free_port(), backend, 232, 2, "sharded"), nprocs=world,
                 timeout=300)


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("host", 4)])
def test_chunked_allreduce_matches_allreduce(backend, world):
    """K-chunked fc weight gradient (column chunks formed one by one, each chunk's row
    segments all-reduced as soon as it exists) equals the bucket all-reduce average."""
    launch.spawn(_w_exchange, args=(world, launch.find_free_port(), backend, 232, 2, "chunked"), nprocs=world,
                 timeout=300)


def test_exchange_byte_model():
    from torch_distributed_sandbox_amd.parallel import factored as F

    K, N, B = 18_000_000, 10, 5
    mb = lambda p, w: F.link_bytes(p, B, N, K, w) / 1e6  # noqa: E731
    assert (round(mb("allreduce", 2)), round(mb("activations", 2)), round(mb("sharded", 2))) == (720, 360, 540)
    assert (round(mb("allreduce", 8)), round(mb("activations", 8)), round(mb("sharded", 8))) == (180, 360, 135)
    assert [F.choose_path(B, N, K, w) for w in (2, 3, 4, 8)] == ["activations", "activations", "sharded", "sharded"]
    assert F.choose_path(16, 10, K, 8) == "allreduce"  # more rows than outputs: the dense gradient is smaller
    for w in (1, 2, 3, 7, 8):
        b = F.shard_bounds(K, w)
        assert b[0][0] == 0 and b[-1][1] == K and all(b[i][1] == b[i + 1][0] for i in range(w - 1))
        assert all(a % 64 == 0 for a, _ in b)


def _w_exchange_policy(rank, world, port):
    dist = _init(rank, world, port, "host")
    from torch_distributed_sandbox_amd.ops import Linear
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel
    from torch_distributed_sandbox_amd.parallel import factored as F

    lin = Linear(1 << 17, 10)
    d = DistributedDataParallel(lin)
    ex = d.exchanges[0]
    for rows in (5, 6, 16):
        want = F.choose_path(rows, 10, 1 << 17, world)
        assert ex.path(rows) == (None if want == "allreduce" else want)
    assert ex.worthwhile(16) is False  # 16 rows > 10 outputs: all-reduce of dW is cheapest
    x = torch.randn(6, 1 << 17)
    d(x).sum().backward()
    assert ex.steps_exchanged == 1
    assert d.fc_grad_path() == ("activation-exchange(zs)" if world == 2 else "sharded-exchange(zs)")
    # the chunked all-reduce is never picked by auto (only on request): auto's all-reduce
    # regime is the plain bucket all-reduce
    assert DistributedDataParallel(Linear(1 << 17, 10), allreduce_chunks=4).exchanges[0].path(16) is None
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_activation_exchange_policy(world):
    launch.spawn(_w_exchange_policy, args=(world, launch.find_free_port()), nprocs=world, timeout=120)


# ---------------------------------------------------------------- TDS_DEBUG_SYNC
def test_debug_sync_mode_collectives_and_ddp(monkeypatch):
    """Stream-ordering assertion mode (every collective waited + device synced on issue)
    must not change results: collectives and the DDP equivalence check pass under it."""
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    monkeypatch.setenv("TDS_DEBUG_SYNC", "1")
    assert dist.debug_sync_enabled()
    launch.spawn(_w_collectives, args=(2, launch.find_free_port(), "gloo"), nprocs=2, timeout=180)
    launch.spawn(_w_ddp, args=(2, launch.find_free_port(), 32, 2, "gloo"), nprocs=2, timeout=300)


# ---------------------------------------------------------------- zero-suppressed activation exchange
def _w_zs_exchange(rank, world, port, backend, H, B, mode="activations"):
    """Compressed vs dense activation exchange on identical replicas: gradients and post-step
    parameters bitwise equal, every step; step 2 runs with a capacity below the count (the
    overflow falls back to the dense rows, still bitwise equal)."""
    dist = _init(rank, world, port, backend)
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    m_z = ConvNet(image_shape=(H, H))
    m_d = copy.deepcopy(m_z)
    d_z = DistributedDataParallel(m_z, grad_exchange=mode, exchange_compress=True)
    d_d = DistributedDataParallel(m_d, grad_exchange=mode, exchange_compress=False)
    o_z = d_z.attach_optimizer(SGD(m_z.parameters(), 0.05))
    o_d = d_d.attach_optimizer(SGD(m_d.parameters(), 0.05))
    crit = CrossEntropyLoss()
    g = torch.Generator().manual_seed(5)
    ex = d_z.exchanges[0]
    for step in range(3):
        if step == 2:
            ex._cap = {mode: 1}  # below the count: this step overflows and sends the dense rows
        xs = torch.rand(world, B, 1, H, H, generator=g)
        ys = torch.randint(0, 10, (world, B), generator=g)
        for d, o in ((d_z, o_z), (d_d, o_d)):
            loss = crit(d(xs[rank]), ys[rank])
            o.zero_grad()
            loss.backward()
        for (n, p), q in zip(m_z.named_parameters(), m_d.parameters()):
            assert torch.equal(p.grad, q.grad), (step, n)
        o_z.step()
        o_d.step()
        for (n, p), q in zip(m_z.named_parameters(), m_d.parameters()):
            assert torch.equal(p, q), ("params", step, n)
    last = ex.zs_stats["last_nnz"]
    last = max(last) if isinstance(last, list) else last
    assert ex.zs_stats["steps"] == 3 and ex.zs_stats["overflows"] == (1 if last > 1 else 0), (rank, ex.zs_stats)
    assert 0.0 < ex.x_ratio < 1.0  # ReLU rows: zeros were suppressed
    base = "activation-exchange" if mode == "activations" else "sharded-exchange"
    assert d_z.fc_grad_path() == base + "(zs)" and d_d.fc_grad_path() == base
    dist.destroy_process_group()


@pytest.mark.parametrize("mode,backend,world,B", [("activations", "gloo", 2, 2), ("activations", "host", 4, 2),
                                                  ("activations", "gloo", 8, 2), ("sharded", "gloo", 2, 2),
                                                  ("sharded", "host", 3, 2), ("sharded", "gloo", 8, 2),
                                                  # B=1 at 232²: 53 pages, an odd record length (the
                                                  # count's int64 slot must stay 8-byte aligned)
                                                  ("activations", "gloo", 2, 1), ("sharded", "gloo", 2, 1)])
def test_zero_suppressed_exchange_bitwise_equal(mode, backend, world, B):
    launch.spawn(_w_zs_exchange, args=(world, launch.find_free_port(), backend, 232, B, mode), nprocs=world,
                 timeout=300)


def _w_step_record(rank, world, port, mode, compress):
    """The exchange holds one record per exchanged step and none between steps: after every
    backward -- accumulating under no_sync(), synced, and synced with a capacity below the counts
    (the overflow's dense re-send) -- no record is left, ``active`` is None, ``steps_exchanged``
    moved by exactly the synced steps and ``fc_grad_path()`` carries the path's tag."""
    dist = _init(rank, world, port, "gloo")
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    # 232: the smallest ConvNet image whose fc layer (10 x 107648 >= 2^20 elements) DDP gives an
    # exchange at all; a 64 x 64 image's fc layer (10 x 8192) takes the plain bucket all-reduce
    H, B = 232, 2
    assert not DistributedDataParallel(ConvNet(image_shape=(64, 64)), grad_exchange="activations").exchanges
    m = ConvNet(image_shape=(H, H))
    d = DistributedDataParallel(m, grad_exchange=mode, exchange_compress=compress,
                                allreduce_chunks=3 if mode == "chunked" else None)
    o = d.attach_optimizer(SGD(m.parameters(), 0.05))
    crit = CrossEntropyLoss()
    ex, = d.exchanges
    tag = {"activations": "activation-exchange", "sharded": "sharded-exchange"}.get(mode)
    tag = "chunked-allreduce" if tag is None else tag + ("(zs)" if compress else "")
    g = torch.Generator().manual_seed(7)
    xs = torch.rand(world, B, 1, H, H, generator=g)
    ys = torch.randint(0, 10, (world, B), generator=g)
    assert ex._step is None and ex.active is None and ex.steps_exchanged == 0

    def backward(sync, what):
        before = ex.steps_exchanged
        if sync:
            crit(d(xs[rank]), ys[rank]).backward()
        else:
            with d.no_sync():
                crit(d(xs[rank]), ys[rank]).backward()
        assert ex._step is None and ex.active is None, what
        assert ex.steps_exchanged == before + (1 if sync else 0), what
        # (before the first exchanged step the layer's gradient has only met the plain path)
        assert d.fc_grad_path() == (tag if ex.steps_exchanged else "allreduce"), (what, d.fc_grad_path())

    o.zero_grad()
    backward(False, "no_sync")
    backward(True, "synced after no_sync")
    o.step()
    o.zero_grad()
    ex.force_capacity_once(1)  # below any count: an encoded step overflows and re-sends dense
    backward(True, "forced capacity 1")
    if compress and mode != "chunked":
        assert ex.zs_stats["steps"] == 2 and ex.zs_stats["overflows"] == 1, ex.zs_stats
    dist.destroy_process_group()


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("mode", ["activations", "sharded", "chunked"])
def test_exchange_step_record_dropped_after_every_backward(mode, compress):
    launch.spawn(_w_step_record, args=(2, launch.find_free_port(), mode, compress), nprocs=2, timeout=120)


def test_zs_codec_reference_roundtrip():
    from torch_distributed_sandbox_amd.parallel import zs

    torch.manual_seed(3)
    for n in (1, 31, 2048, 2049, 70000):
        x = torch.relu(torch.randn(n))
        x[::5] = -0.0  # negative zero must survive (bits, not value, decide)
        meta = torch.empty(zs.meta_numel(n), dtype=torch.int32)
        vals = torch.empty(n)
        nnz = int(zs.encode(x, meta, vals))
        assert nnz == int((x.view(torch.int32) != 0).sum())
        assert int(zs.nnz_of(meta, n)) == nnz
        out = torch.full((n,), 7.0)
        zs.decode(meta, vals, out)
        assert torch.equal(out.view(torch.int32), x.view(torch.int32))


def test_pooled_exchange_geometry_and_pricing():
    """The pooled activation-exchange source (parallel/factored.py): the pooled plane of the fused
    head's fc inputs (csrc/kernels/pooled_layout.h: 4 x 8 blocks), and no pooled pricing for a layer
    that cannot take it (CPU weight, or inputs that are not 32 square planes)."""
    import torch

    from torch_distributed_sandbox_amd.parallel import factored

    assert factored.pooled_plane(32 * 747 * 747) == 748 * 752
    assert factored.pooled_plane(32 * 64 * 64) == 64 * 64
    assert factored.pooled_plane(32 * 10 * 11) is None and factored.pooled_plane(33) is None
    w = torch.nn.Parameter(torch.zeros(10, 32 * 64 * 64))
    ex = factored.ActivationExchange(w, None, None, 2, "auto", lambda on: None, lambda: None, None)
    assert ex.source == "pooled" and not ex.pooled_capable()  # a CPU weight: the rows path prices it
    ex.detach()
    try:
        factored.ActivationExchange(w, None, None, 2, "auto", lambda on: None, lambda: None, None, source="x")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown source must be refused")
