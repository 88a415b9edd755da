"""The activation exchange's sign-masked ya payload (``source="pooled-masked"``; parallel/pooled_masked.py,
csrc/kernels/head_pb.hip): the encode kernels against the torch reference, the masked update ops bitwise
against the dense pooled ops, the capacity overflow, and the exchange end to end against "pooled".

Shapes (H; P = H/2, Q = H/4): 36 -> Q = 9 (one partial block column), 44 -> Q = 11 (odd rows off the 16-B
grid), 1040 -> Q = 260, Q8 = 33 (two pages per block row, the second with one block)."""
import copy
import os

import pytest
import torch

from test_fused_gpu import _check, new_mag, set_ya_scale
from torch_distributed_sandbox_amd.parallel import pooled_masked as pm

pytestmark = pytest.mark.gpu

D = 0.5  # ya's decode factor


def _ops():
    import torch_distributed_sandbox_amd as tds

    return tds._ext.ops()


def _rank(H, B, seed, special=False):
    """One rank's ya [B, 32, plane] (padding entries random, as a producer leaves them) and record, on
    the host.  a, b, b2 are multiples of 2^-8 and d a power of two, so a*d*h + (a*b2 + b) is exact in
    fp64 and the reference's single rounding to fp32 is the kernels' fused multiply-add.  special: a
    -0.0 and a NaN, a fully dropped and a fully kept block; channel 1 always has a negative a."""
    Q = H // 4
    q4, q8, _ = pm.geom(Q)
    g = torch.Generator().manual_seed(seed)
    q = lambda s: (torch.randn(32, generator=g) * s * 256).round() / 256
    a, b, b2 = q(1.0), q(0.3), q(0.1)
    a[1] = -a[1].abs() - 0.5
    a[2], a[3] = 1.5, 1.5
    ya = torch.randn(B, 32, q4, q8, 32, generator=g).half()
    if special:
        ya[0, 0, 0, 0, 0], ya[0, 0, 0, 0, 1] = -0.0, float("nan")
        ya[0, 2, 0, 0], ya[0, 3, 0, 0] = -8.0, 8.0  # z = -6 + ..., 6 + ...: block (0, 0) is inside the image
    rec = torch.zeros(128)
    rec[:32], rec[32:64], rec[64:67], rec[68:100] = a, b, torch.tensor([D, 1.0, 1.0]), b2
    return ya.view(B, 32, -1), rec


def _encode(ya, rec, P, cap=None):
    ops = _ops()
    meta = torch.empty(ops.head_pooled_masked_pages(ya.shape[0], P) * 33, dtype=torch.int32, device=ya.device)
    vals = torch.zeros(cap or ya.numel(), dtype=torch.float16, device=ya.device)
    return meta, vals, ops.head_pooled_encode(ya, rec, P, meta, vals)


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [36, 44, 1040])
def test_encode_matches_reference(gpu, H, B):
    """meta, values and the count against encode_ref; X decoded from the GPU payload is bitwise the dense
    head forward's X rows and within fp32 rounding of relu(a*y + b) in fp64."""
    P, Q = H // 2, H // 4
    ya, rec = _rank(H, B, 100 + H + B, special=True)
    meta, vals, nnz = _encode(ya.to(gpu), rec.to(gpu), P)
    mref, vref, nref = pm.encode_ref(ya, rec, Q)
    assert int(nnz) == nref and 0 < nref < ya.numel()
    assert torch.equal(meta.cpu(), mref)
    assert torch.equal(_bits(vals[:nref]), _bits(vref)) and not vals[nref:].any()
    words = mref.view(-1, 33)[:, 1:]
    page = ((0 * 32 + 2) * pm.geom(Q)[0]) * pm.geom(Q)[2]  # (image 0, channel 2, block row 0, chunk 0)
    assert words[page, 0] == 0 and words[page + pm.geom(Q)[0] * pm.geom(Q)[2], 0] == -1  # dropped / kept blocks
    x = pm.decode_ref(meta.cpu(), vals.cpu(), rec, B, Q)
    ops = _ops()
    wfc = torch.zeros(10, 32 * Q * Q, device=gpu)
    xo = torch.empty(B, 32 * Q * Q, device=gpu)
    aff2, b2 = rec[:64].to(gpu), rec[68:100].contiguous().to(gpu)
    ops.fused_head_forward_aff(ya.to(gpu), aff2, b2, set_ya_scale(new_mag(gpu, B, P), D), wfc, None, P, xo)
    assert torch.equal(_bits(x), _bits(xo))
    assert x.isnan().sum() == 1  # the NaN value travels
    q4, q8, _ = pm.geom(Q)
    h = ya.view(B, 32, q4, q8, 4, 8).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, 4 * q4, 8 * q8)[:, :, :Q, :Q].double()
    a, b, b2d = (rec[s].double().view(1, 32, 1, 1) for s in (slice(0, 32), slice(32, 64), slice(68, 100)))
    ref = torch.relu(a * (h * D + b2d) + b).reshape(B, -1)
    bound = 2.0 ** -22 * ((a * h * D).abs() + (a * b2d).abs() + b.abs()).reshape(B, -1)
    ok = ~ref.isnan()
    assert ((x.double() - ref).abs()[ok] <= bound[ok]).all()


def _payload(gpu, H, B, W, seed):
    """W ranks' dense ya / records and their gathered masked payloads at a common capacity."""
    P = H // 2
    ranks = [_rank(H, B, seed + r) for r in range(W)]
    ya_all = torch.stack([ya for ya, _ in ranks]).to(gpu)
    rec_all = torch.stack([rec for _, rec in ranks]).to(gpu)
    enc = [_encode(ya_all[r], rec_all[r], P) for r in range(W)]
    cap = max(int(n) for _, _, n in enc)
    meta_all = torch.stack([m for m, _, _ in enc])
    vals_all = torch.stack([v[:cap] for _, v, _ in enc])
    return ya_all, rec_all, meta_all, vals_all


def _masked_vs_dense(gpu, H, B, W, NC, seed, fp64=False):
    ops = _ops()
    P, Q = H // 2, H // 4
    ya_all, rec_all, meta_all, vals_all = _payload(gpu, H, B, W, seed)
    torch.manual_seed(seed)
    wfc = torch.randn(NC, 32 * Q * Q, device=gpu) * 0.01
    dl = torch.randn(W * B, NC, device=gpu)
    scale, lr = 1.0 / W, 0.25
    outs = []
    for masked in (False, True):
        src = (meta_all, vals_all) if masked else (ya_all,)
        upd = ops.head_update_pooled_masked if masked else ops.head_update_pooled
        step = ops.head_update_pooled_masked_step if masked else ops.head_update_pooled_step
        out, w0, w3 = torch.full_like(wfc, 7.0), wfc.clone(), wfc.clone()
        upd(dl, *src, rec_all, wfc, out, P, scale, 0.0, 1)
        dw = out.clone()
        upd(dl, *src, rec_all, wfc, out, P, scale, 0.0, 2)
        upd(dl, *src, rec_all, w0, None, P, scale, lr, 0)
        mbuf = torch.randn(NC, 32 * Q * Q, device=gpu, generator=torch.Generator(device=gpu).manual_seed(seed))
        step(dl, *src, rec_all, w3, mbuf, P, scale, lr, 1e-3, 0.9, 0.1, False, False)
        outs.append((dw, out, w0, w3, mbuf))
    for name, d, m in zip(("mode 1", "mode 2", "mode 0", "mode 3 W", "mode 3 buffer"), *outs):
        assert torch.equal(d, m), (name, (d - m).abs().max().item())
    if fp64:
        x = torch.cat([pm.decode_ref(*pm.encode_ref(ya_all[r].cpu(), rec_all[r].cpu(), Q)[:2], rec_all[r].cpu(), B, Q)
                       for r in range(W)])
        _check(outs[1][0], (dl.double().cpu().t() @ x.double()) * scale, 1e-6, "dW against fp64 dl^T X")


@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("NC", [7, 10])
@pytest.mark.parametrize("H", [36, 44])
def test_masked_update_is_bitwise_the_dense_update(gpu, H, NC, W, B):
    """head_update_pooled_masked[_step] against head_update_pooled[_step] on the same inputs, modes 0 to 3,
    each rank with its own record; one case also against fp64 with test_head_update_pooled's tolerance."""
    _masked_vs_dense(gpu, H, B, W, NC, 1000 * H + 100 * NC + 10 * W + B, fp64=(H, NC, W, B) == (44, 10, 3, 5))


def test_masked_update_two_pages_per_block_row(gpu):
    _masked_vs_dense(gpu, 1040, 2, 2, 10, 7)


@pytest.mark.parametrize("H,B", [(36, 1), (44, 3)])
def test_encode_overflow_drops_past_capacity(gpu, H, B):
    """cap below the kept count: the true count is returned and nothing is written past cap (guard words)."""
    P, Q = H // 2, H // 4
    ya, rec = _rank(H, B, 5 + H)
    _, vref, nref = pm.encode_ref(ya, rec, Q)
    cap, guard = nref // 2, 64
    buf = torch.full((cap + guard,), 1.5, dtype=torch.float16, device=gpu)
    meta = torch.empty(pm.meta_numel(B, Q), dtype=torch.int32, device=gpu)
    nnz = _ops().head_pooled_encode(ya.to(gpu), rec.to(gpu), P, meta, buf[:cap])
    assert int(nnz) == nref
    assert torch.equal(_bits(buf[:cap]), _bits(vref[:cap])) and (buf[cap:] == 1.5).all()


# ---------------------------------------------------------------- the exchange, against "pooled"
HX, STEPS = 256, 2  # fc: 10 x 131072 (exchange candidate)


def _two_sources(dev, world, rank, overlap, momentum):
    """Two steps of twin models under "pooled-masked" and "pooled"; the masked twin's second step gets a
    capacity below its counts (the dense fallback).  Every parameter must end bitwise equal."""
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    m1 = ConvNet(image_shape=(HX, HX), device=dev, mode="fused")
    m2 = copy.deepcopy(m1)
    d1 = DistributedDataParallel(m1, grad_exchange="activations", overlap_optimizer=overlap,
                                 exchange_source="pooled-masked")
    d2 = DistributedDataParallel(m2, grad_exchange="activations", overlap_optimizer=overlap, exchange_source="pooled")
    o1 = d1.attach_optimizer(SGD(m1.parameters(), 0.05, momentum=momentum))
    o2 = d2.attach_optimizer(SGD(m2.parameters(), 0.05, momentum=momentum))
    crit = CrossEntropyLoss()
    g = torch.Generator().manual_seed(21)
    xs = torch.rand(STEPS, world, 2, 1, HX, HX, generator=g)
    ys = torch.randint(0, 10, (STEPS, world, 2), generator=g)
    ex = d1.exchanges[0]
    for s in range(STEPS):
        if s == 1:
            ex.force_capacity_once(64)
        for d, o in ((d1, o1), (d2, o2)):
            loss = crit(d(xs[s, rank].to(dev)), ys[s, rank].to(dev))
            o.zero_grad()
            loss.backward()
            o.step()
        if s == 0:
            assert d1.fc_grad_path() == "activation-exchange(pooled-masked)"
            sent = ex.x_ratio * 2 * 131072 * 4
    d1.wait_pending_updates()
    d2.wait_pending_updates()
    torch.cuda.synchronize()
    assert ex.zs_stats["steps"] == 2 and ex.zs_stats["overflows"] == 1
    assert round(sent) == pm.payload_bytes(2, HX // 4, 2 * 32 * 64 * 64)  # the first step: capacity = dense
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), n


@pytest.fixture(scope="module")
def pg(gpu):
    from torch_distributed_sandbox_amd.parallel import distributed as dist
    from torch_distributed_sandbox_amd.parallel import launch

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = launch.find_free_port()
    dist.init_process_group("rccl-native", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


@pytest.mark.parametrize("overlap,momentum", [(False, 0.0), (True, 0.0), (True, 0.9)])
def test_forced_exchange_world_one_matches_pooled(pg, gpu, overlap, momentum):
    _two_sources(gpu, 1, 0, overlap, momentum)


def _worker(rank, world, port):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _two_sources(dev, world, rank, True, 0.9)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_match_pooled(gpu):
    """Two gloo ranks sharing the device, as tests/test_multirank_gpu.py runs them."""
    from torch_distributed_sandbox_amd.parallel import launch

    launch.spawn(_worker, args=(2, launch.find_free_port()), nprocs=2, timeout=240)
