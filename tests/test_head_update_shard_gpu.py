"""The shard form of the pooled fc step (ops.head_update_pooled_shard, kernels/head_pb.hip
head_upd_pb_shard_kernel): the pooled sharded exchange's owner forms the fc columns of its channels
[c0, c1) from every rank's ya planes of those channels.  It must reproduce, bit for bit, those
columns of the full sweep (ops.head_update_pooled) and of the head forward's own X rows, and touch
nothing outside them."""
import pytest
import torch

from test_fused_gpu import _check, _ops, new_mag, set_ya_scale, ya_of

pytestmark = pytest.mark.gpu

NC = 10
SENTINEL = 7.0

# (P, B, W, c0, c1)
CASES = [
    (64, 3, 2, 0, 16),     # the plain case
    (38, 5, 8, 28, 32),    # odd Q = 19 (rows off the 16-B grid), the last channels, 40 source images
    (130, 2, 3, 11, 22),   # Q = 65: a partial 8-column block, the uneven middle shard
    (520, 1, 2, 5, 6),     # Q8 = 33: the second 32-block chunk and its idle lanes, one channel
]


def _case(gpu, P, B, W):
    """W ranks' ya, head records and the head forward's X rows, as test_head_update_pooled builds them."""
    ops = _ops()
    Q = P // 2
    torch.manual_seed(P + 10 * B + W)
    wfc = torch.randn(NC, 32 * Q * Q, device=gpu) * 0.01
    bfc = torch.randn(NC, device=gpu)
    b2 = torch.randn(32, device=gpu) * 0.1
    mag = set_ya_scale(new_mag(gpu, B, P), 0.5)  # ya decode d = 0.5
    yas, recs, xs = [], [], []
    for _ in range(W):
        h = torch.randn(B, P, P, 32, device=gpu).half()
        ya = ya_of(h, torch.randn(32, device=gpu), Q)
        aff2 = torch.cat([torch.randn(32, device=gpu), torch.randn(32, device=gpu) * 0.1])
        xo = torch.empty(B, 32 * Q * Q, device=gpu)
        ops.fused_head_forward_aff(ya, aff2, b2, mag, wfc, bfc, P, xo)
        yas.append(ya)
        recs.append(ops.head_pooled_record(aff2, b2, mag))
        xs.append(xo)
    return wfc, torch.stack(yas), torch.stack(recs), torch.cat(xs)


@pytest.mark.parametrize("P,B,W,c0,c1", CASES)
def test_head_update_pooled_shard(gpu, P, B, W, c0, c1):
    ops = _ops()
    Q = P // 2
    wfc, ya_all, rec_all, x_all = _case(gpu, P, B, W)
    ya_sh = ya_all[:, :, c0:c1].contiguous()
    M, k0, k1 = W * B, c0 * Q * Q, c1 * Q * Q

    def outside_kept(t, want):
        assert torch.equal(t[:, :k0], want[:, :k0]) and torch.equal(t[:, k1:], want[:, k1:])

    sentinel = torch.full_like(wfc, SENTINEL)
    w_before = wfc.clone()
    # one-hot dl, scale 1, NC source images per call: row j of the result is image m0 + j's X itself
    # (exact products and sums) on the shard's columns
    for m0 in range(0, M, NC):
        n = min(NC, M - m0)
        eye = torch.zeros(M, NC, device=gpu)
        eye[torch.arange(m0, m0 + n), torch.arange(n)] = 1.0
        out = sentinel.clone()
        ops.head_update_pooled_shard(eye, ya_sh, rec_all, wfc, out, P, c0, c1, 1.0, 0.0, 1)
        assert torch.equal(out[:n, k0:k1], x_all[m0:m0 + n, k0:k1]), m0
        assert (out[n:, k0:k1] == 0).all()
        outside_kept(out, sentinel)
    assert torch.equal(wfc, w_before)
    # random dl: bitwise the columns of the full sweep
    dl = torch.randn(M, NC, device=gpu)
    scale, lr = 1.0 / W, 0.25
    full = torch.empty_like(wfc)
    ops.head_update_pooled(dl, ya_all, rec_all, wfc, full, P, scale, 0.0, 1)
    out = sentinel.clone()
    ops.head_update_pooled_shard(dl, ya_sh, rec_all, wfc, out, P, c0, c1, scale, 0.0, 1)
    assert torch.equal(out[:, k0:k1], full[:, k0:k1])
    outside_kept(out, sentinel)
    # += : within the fp64 bound of test_head_update_pooled
    ref = (dl.double().t() @ x_all[:, k0:k1].double()) * scale
    ops.head_update_pooled_shard(dl, ya_sh, rec_all, wfc, out, P, c0, c1, scale, 0.0, 2)
    _check(out[:, k0:k1], 2 * ref, 1e-6, "dW (+=)")
    outside_kept(out, sentinel)
    assert torch.equal(wfc, w_before)
    # the update: the shard's columns as the full sweep updates them, every other bit of W kept
    w_full = wfc.clone()
    ops.head_update_pooled(dl, ya_all, rec_all, w_full, None, P, scale, lr, 0)
    ops.head_update_pooled_shard(dl, ya_sh, rec_all, wfc, None, P, c0, c1, scale, lr, 0)
    assert torch.equal(wfc[:, k0:k1], w_full[:, k0:k1])
    assert not torch.equal(wfc[:, k0:k1], w_before[:, k0:k1])
    outside_kept(wfc, w_before)
