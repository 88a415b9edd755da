"""The pooled fc exchange for 11 .. 64 classes: ops.head_update_pooled on csrc/kernels/head_wide.hip's
head_wide_upd_kernel against fp64, the wide backward's no-dW form, and the fused plan under DDP with
the exchange forced at world size 1 and chosen by ``auto`` on two ranks."""
import copy
import functools
import os

import pytest
import torch

from test_comm_gpu import pg  # noqa: F401  (the world-1 process group fixture)
from test_fused_gpu import _check, _ops, mag_floats, new_mag, set_ya_scale, ya_of
from test_head_wide_gpu import _backward
from test_head_wide_gpu import _case as _wide_case

pytestmark = pytest.mark.gpu

CASES = [  # (P, B, NC, W)
    (8, 1, 11, 1),     # Q = 4, one image, a second class tile of one class
    (18, 5, 16, 2),    # odd Q: all four alignment classes; 10 images: K padding, a K step of two ranks
    (64, 3, 64, 3),    # every class tile full, rank boundaries inside K steps
    (38, 16, 33, 2),   # 32 images, the image tile full per rank
    (150, 2, 11, 1),   # a second, partial 64-column span
    (8, 16, 11, 9),    # 144 images: a second image chunk (128 per launch)
]


@functools.lru_cache(maxsize=None)
def _case(gpu, P, B, NC, W):
    """W ranks' ya, head records (each its own BN2 affine and ya scale) and the X rows their ten-class
    head forward wrote (<= 8 images per call).  Computed once; nothing in it is written afterwards."""
    ops, Q = _ops(), P // 2
    K = 32 * Q * Q
    torch.manual_seed(P + 10 * B + NC + W)
    w10, b2 = torch.randn(10, K, device=gpu) * 0.01, torch.randn(32, device=gpu) * 0.1
    yas, recs, xs = [], [], []
    for r in range(W):
        mag = set_ya_scale(new_mag(gpu, B, P), 0.25 if r % 2 else 0.5)
        ya = ya_of(torch.randn(B, P, P, 32, device=gpu).half(), torch.randn(32, device=gpu), Q)
        aff2 = torch.cat([torch.randn(32, device=gpu), torch.randn(32, device=gpu) * 0.1])
        xo = torch.empty(B, K, device=gpu)
        for b0 in range(0, B, 8):
            ops.fused_head_forward_aff(ya[b0:b0 + 8], aff2, b2, mag, w10, None, P, xo[b0:b0 + 8])
        yas.append(ya), recs.append(ops.head_pooled_record(aff2, b2, mag)), xs.append(xo)
    return torch.stack(yas), torch.stack(recs), torch.cat(xs)


@pytest.mark.parametrize("P,B,NC,W", CASES)
def test_head_update_pooled_wide(gpu, P, B, NC, W):
    """X recomputed bit for bit (one-hot dl), the three modes against fp64 at the wide backward's dW
    bound, two launches bit-equal, nothing written outside [NC, K]."""
    ops, M = _ops(), W * B
    ya_all, rec_all, x_all = _case(gpu, P, B, NC, W)
    K = x_all.shape[1]
    wfc = torch.randn(NC, K, device=gpu) * 0.01
    buf = torch.full((NC + 2, K), 7.0, device=gpu)  # rows 0 and NC + 1: sentinels
    out = buf[1:NC + 1]
    if M <= NC:
        eye = torch.zeros(M, NC, device=gpu)
        eye[torch.arange(M), torch.arange(M)] = 1.0
        ops.head_update_pooled(eye, ya_all, rec_all, wfc, out, P, 1.0, 0.0, 1)
        assert torch.equal(out[:M], x_all), (out[:M] - x_all).abs().max()
        assert (out[M:] == 0).all()
    dl = torch.randn(M, NC, device=gpu)
    scale, lr = 1.0 / W, 0.25
    ref = (dl.double().t() @ x_all.double()) * scale
    ops.head_update_pooled(dl, ya_all, rec_all, wfc, out, P, scale, 0.0, 1)
    _check(out, ref, 1e-5, "dW (=)")
    again = torch.full_like(out, 3.0)
    ops.head_update_pooled(dl, ya_all, rec_all, wfc, again, P, scale, 0.0, 1)
    assert torch.equal(again, out)
    ops.head_update_pooled(dl, ya_all, rec_all, wfc, out, P, scale, 0.0, 2)
    _check(out, 2 * ref, 1e-5, "dW (+=)")
    assert (buf[0] == 7.0).all() and (buf[-1] == 7.0).all()
    w0 = wfc.double()
    ops.head_update_pooled(dl, ya_all, rec_all, wfc, None, P, scale, lr, 0)
    _check(wfc, w0 - lr * ref, 1e-5, "W update")


@pytest.mark.parametrize("P,B,NC", [(18, 5, 16), (38, 16, 33)])
def test_wide_backward_without_dw(gpu, P, B, NC):
    c = _wide_case(gpu, P, B, NC)
    w = c["wfc"].clone()
    mags = [set_ya_scale(new_mag(gpu, B, P)) for _ in range(2)]
    full = _backward(c, P, c["wfc"], mag=mags[0])
    nodw = _backward(c, P, w, mag=mags[1], compute_dw=False)
    assert nodw[0].numel() == 0 and torch.equal(w, c["wfc"])
    for a, b in zip(full[1:], nodw[1:]):  # dbfc, dgamma2, dbeta2, g2m, kbuf
        assert torch.equal(a, b)
    assert torch.equal(mag_floats(mags[0])[32], mag_floats(mags[1])[32])
    with pytest.raises(RuntimeError):
        _backward(c, P, w, None, 0.5, compute_dw=False)
    with pytest.raises(RuntimeError):
        _backward(c, P, w, mom_buf=torch.zeros_like(w), momentum=0.9, compute_dw=False)
    assert torch.equal(w, c["wfc"])


H, NC = 160, 26  # fc: 26 x 51200, an exchange candidate


def _models(dev, fused_overlap=False, mode="fused", lr=0.01):
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel as DDP

    torch.manual_seed(0)
    m1 = ConvNet(num_classes=NC, image_shape=(H, H), device=dev, mode=mode)
    m2 = copy.deepcopy(m1)
    d1 = DDP(m1, grad_exchange="activations" if torch.distributed.get_world_size() == 1 else "auto",
             overlap_optimizer=fused_overlap, fuse_update_in_backward=fused_overlap)
    d2 = DDP(m2, grad_exchange="allreduce")
    return [(d, d.attach_optimizer(SGD(d.module.parameters(), lr))) for d in (d1, d2)]


def _step(d, o, x, y):
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    loss = CrossEntropyLoss()(d(x), y)
    o.zero_grad()
    loss.backward()
    o.step()


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("B,overlap", [(3, False), (9, False), (3, True)])
def test_wide_plan_exchange_forced(pg, gpu, B, overlap):  # noqa: F811
    (d1, o1), (d2, o2) = _models(gpu, overlap, lr=1e-4 if overlap else 0.01)
    g = torch.Generator(device=gpu).manual_seed(5)
    for step in range(2):
        x = torch.rand(B, 1, H, H, device=gpu, generator=g)
        y = torch.randint(0, NC, (B,), device=gpu, generator=g)
        _step(d1, o1, x, y), _step(d2, o2, x, y)
        for (n, p), q in zip(d1.module.named_parameters(), d2.module.parameters()):
            if overlap or n.endswith("0.bias"):
                continue
            assert _rel(p.grad, q.grad) < 1e-5, (step, n)
            q.data.copy_(p.data)
    d1.wait_pending_updates()
    torch.cuda.synchronize()
    assert d1.fc_grad_path() == "activation-exchange(pooled)" and d1.exchanges[0].steps_exchanged == 2
    if overlap:
        for (n, p), q in zip(d1.module.named_parameters(), d2.module.parameters()):
            assert torch.allclose(p, q, rtol=1e-6, atol=1e-9), n


def test_wide_layers_plan_keeps_the_bucket(pg, gpu):  # noqa: F811
    (d1, o1), _ = _models(gpu, mode="layers")
    _step(d1, o1, torch.rand(2, 1, H, H, device=gpu), torch.tensor([3, 25], device=gpu))
    assert d1.fc_grad_path() == "local" and d1.exchanges[0].steps_exchanged == 0
    assert d1.module.fc.weight.grad is not None


def _worker(rank, world, port, out):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pairs = _models(dev)
    g = torch.Generator().manual_seed(21)
    xs, ys = torch.rand(2, world, 2, 1, H, H, generator=g), torch.randint(0, NC, (2, world, 2), generator=g)
    for s in range(2):
        for d, o in pairs:
            _step(d, o, xs[s, rank].to(dev), ys[s, rank].to(dev))
    torch.cuda.synchronize()
    torch.save({"path": pairs[0][0].fc_grad_path(),
                "params": [[p.detach().cpu() for p in d.module.parameters()] for d, _ in pairs]},
               os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_wide_exchange_two_ranks(gpu, tmp_path):
    from torch_distributed_sandbox_amd.parallel import launch

    launch.spawn(_worker, args=(2, launch.find_free_port(), str(tmp_path)), nprocs=2, timeout=240)
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(2))
    assert r0["path"] == r1["path"] == "activation-exchange(pooled)"
    for p0, p1, q in zip(r0["params"][0], r1["params"][0], r0["params"][1]):
        assert torch.equal(p0, p1)
        assert _rel(p0, q) < 1e-5
