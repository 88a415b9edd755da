"""The rolling conv2 backward on LONG tile lists: test_fused_gpu's conv2-backward cases run on a full
grid, where every workgroup gets at most two tiles -- no descriptor base carried from tile to tile,
no segment start in the middle of a list, no column or image change.  Here the grid is shrunk to 32
workgroups (ops.set_cu_reserve), so a list walks down segments, across columns and across images.

Each case asserts (a) dp1 / dw2 / db2 within exactly the bounds
test_conv2_backward_fused_with_bn2_pool derives (fp64 reference, TF32-operand reference), and (b)
dp1h bit-identical to the same call on the full grid: there every tile is reached through another
list (other carried bases, other look-ahead sets), and a tile's bytes may not depend on that.  dw2
and db2 are summed in another order on another grid, so they are held to the references only."""
import pytest
import torch
import torch.nn.functional as F

from _tf32ref import tf32
from test_fused_gpu import (_check_conv, _err, _head_case, _ops, dp1h_decode, mag_floats, new_mag, y2h_encode,
                            ya_of, ypart)

pytestmark = pytest.mark.gpu

NWG = 32


@pytest.fixture
def small_grid():
    """-> switch(on): on leaves NWG workgroups to the persistent kernels, off all of them; the
    reserve is back at 0 after the test however it ends."""
    ops = _ops()

    def use(on):
        ops.set_cu_reserve(ops.device_cus() - NWG if on else 0)

    try:
        yield use
    finally:
        ops.set_cu_reserve(0)


# (i) 49 x 25 tiles: every column a 48-tile segment and a 1-tile one, ~38 tiles per list;
# (ii) odd size (border paths, unpooled last row / column), lists crossing images;
# (iii) 15 / 45 / 153 tiles: lists of 0-1, 1-2, 4-5 tiles (look-ahead start-up, padded tail)
@pytest.mark.parametrize("P,B", [(392, 1), (37, 3), (40, 1), (72, 1), (130, 1)])
def test_conv2_backward_long_walks(gpu, small_grid, P, B):
    ops = _ops()
    assert ops.device_cus() - NWG >= 0
    y2, b2, g2, be2, wfc, bfc, _, _ = _head_case(gpu, P, B, 7 * P + B)
    dl = torch.randn(B, wfc.shape[0], device=gpu)
    p = torch.relu(torch.randn(B, P, P, 16, device=gpu)).half()
    w2 = torch.randn(32, 16, 5, 5, device=gpu) * 0.05
    mag = new_mag(gpu, B, P)
    _, wd = ops.conv2_pack(w2, mag)
    y2h, a2, y2 = y2h_encode(y2, b2, g2, mag)
    Q = P // 2
    yc = (y2 - b2).double()
    partial2 = torch.stack([yc.sum((0, 1, 2)), (yc * yc).sum((0, 1, 2))], dim=1).contiguous()
    ya = ya_of(y2h, g2, Q)
    _, stats2, aff2 = ops.fused_head_forward(ya, partial2, b2, g2, be2, None, None, None, 0.1, 1e-5, wfc, bfc, P,
                                             mag=mag)
    yp = ypart(mag)
    yp.zero_()
    yp[:, 0] = (y2 - b2).abs().amax((0, 1, 2)).view(torch.int32)
    _, _, _, _, g2m, kbuf = ops.fused_head_backward(dl, ya, stats2, aff2, b2, g2, wfc, P, None, 1.0, True, mag=mag)
    # the full grid first (reserve 0), then the same call on NWG workgroups
    full_dp1h, _, _ = ops.fused_conv2_backward_y2(y2h, a2, g2m, aff2, kbuf, b2, mag, p, wd, 1.0)
    small_grid(True)
    dp1h, dw2, db2 = ops.fused_conv2_backward_y2(y2h, a2, g2m, aff2, kbuf, b2, mag, p, wd, 1.0)
    small_grid(False)
    torch.cuda.synchronize()
    assert torch.equal(dp1h, full_dp1h), "dp1h depends on the workgroup count"
    dp1 = dp1h_decode(dp1h, mag_floats(mag)[44].item(), P)
    # the references and bounds of test_conv2_backward_fused_with_bn2_pool
    yr = y2.permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    z = F.batch_norm(yr, None, None, g2.double().cpu(), be2.double().cpu(), True, 0.1, 1e-5)
    pz = F.max_pool2d(F.relu(z), 2, 2)
    F.linear(pz.reshape(B, -1), wfc.double().cpu(), bfc.double().cpu()).backward(dl.double().cpu())
    dy2 = yr.grad
    pr = p.permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    wr = w2.double().cpu().requires_grad_(True)
    br = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    F.conv2d(pr, wr, br, padding=2).backward(dy2)
    prt = p.permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    wrt = tf32(w2.cpu()).requires_grad_(True)
    F.conv2d(prt, wrt, None, padding=2).backward(tf32(dy2))
    e, sc = _err(dp1.permute(0, 3, 1, 2), pr.grad)
    et, _ = _err(prt.grad, pr.grad)
    bound = max(1e-5 * sc, 2.5 * et) + 2.0 ** -11 * sc
    print(f"P={P} B={B}: dp1 err {e:.3e} bound {bound:.3e} (TF32 convs {et:.3e}, scale {sc:.3e})")
    assert e <= bound, f"dp1: max err {e:.3e} vs bound {bound:.3e} (scale {sc:.3e})"
    print(f"P={P} B={B}: dw2 err {_err(dw2, wr.grad)[0]:.3e}, TF32 convs {_err(wrt.grad, wr.grad)[0]:.3e}")
    _check_conv(dw2, wr.grad, wrt.grad, "dw2", k=2.5)
    err = (db2.double().cpu() - br.grad).abs()
    bound = dy2.abs().sum((0, 2, 3)) * 2.0 ** -11 * 1.01 + 1e-4 * wr.grad.abs().max().item()
    print(f"P={P} B={B}: db2 err {err.max().item():.3e}, least bound {bound.min().item():.3e}")
    assert bool((err <= bound).all()), (err.max().item(), bound.min().item())
