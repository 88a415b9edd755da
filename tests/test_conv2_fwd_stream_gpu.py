"""The conv2 forward on LONG tile lists and on the all-positive-gamma2 path: test_fused_gpu's
conv2-forward cases run on a full grid (at most one tile per workgroup: nothing carried from tile to
tile, no look-ahead entry) with randn gammas, which make a wave's channels all positive with
probability 2^-16.  Here the grid is shrunk to 96 workgroups (ops.set_cu_reserve), so a list walks
border and interior tiles in turn and crosses images, and gamma2 is chosen per wave.

Each case asserts (a) everything test_conv2_forward asserts, with its bounds (y2 against the
TF32-operand fp64 reference, ymax, the BN2 partial sums, ya bit-equal to the window extreme of the
stored y2h, the a2 codes), on both grids; (b) y2h, ya and a2 of the 96-workgroup call bit-identical to
the full grid's: there every tile is reached through another list, and a tile's bytes may not depend
on that (the partials are grouped differently and are held to the references only); (c) ya of the
inference launch bit-identical to the training launch's, on both grids.

gamma2 == 0 (kernels/conv2_fwd2.hip): every BN2 output of a window is beta2 and torch's max-pool keeps
the first position, so that channel's ya is y2h at position 0 and its a2 code is 0."""
import pytest
import torch
import torch.nn.functional as F

from _tf32ref import tf32
from test_fused_gpu import (_check_conv, _err, _ops, _windows, a2_decode, first_extreme, new_mag, pb_to_planar,
                            window_extreme, y2h_decode_factor, ypart)

pytestmark = pytest.mark.gpu

NWG = 32  # CUs left to the persistent kernels: the forward launches 3 workgroups on each, 96


@pytest.fixture
def small_grid():
    """-> switch(on): on leaves NWG CUs to the persistent kernels, off all of them; the reserve is
    back at 0 after the test however it ends."""
    ops = _ops()

    def use(on):
        ops.set_cu_reserve(ops.device_cus() - NWG if on else 0)

    try:
        yield use
    finally:
        ops.set_cu_reserve(0)


_CASES = {}


def _case(gpu, P, B):
    """p1, conv2 weights and bias of a shape and their fp64 references (exact and TF32-operand),
    computed once: gamma2 does not enter them."""
    if (P, B) not in _CASES:
        torch.manual_seed(11 * P + B)
        p = torch.relu(torch.randn(B, P, P, 16, device=gpu)).half()  # the fp16 operand as layer 1 stores it
        w2 = torch.randn(32, 16, 5, 5, device=gpu) * 0.05
        b2 = torch.randn(32, device=gpu)
        pin = p.permute(0, 3, 1, 2).double().cpu()
        ref = F.conv2d(pin, w2.double().cpu(), b2.double().cpu(), padding=2)
        reft = F.conv2d(pin, tf32(w2.cpu()), b2.double().cpu(), padding=2)
        _CASES[(P, B)] = (p, w2, b2, ref, reft)
    return _CASES[(P, B)]


def _gamma(gpu, kind, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.randn(32, generator=g)
    if kind == "positive":  # every wave on the all-positive path
        g2 = r.abs() + 0.1
    elif kind == "mixed":  # max and min windows in every wave
        g2 = r
    elif kind == "half":  # the two waves of a tile row half take different paths
        g2 = torch.cat([r[:16].abs() + 0.1, r[16:]])
        g2[17], g2[20] = -0.8, 1.1
    else:  # one channel exactly 0: first-position windows
        g2 = r.abs() + 0.1
        g2[5] = 0.0
    return g2.to(gpu)


def _check_codes(a2, ref_nchw, g2, Q, gap=1e-5):
    """test_fused_gpu._check_argmax_kept with the gamma2 == 0 rule: the codes name the reference's
    first extreme of every window whose top two values differ by more than fp32 accumulation noise;
    a channel with gamma2 == 0 has code 0 everywhere."""
    assert a2.dtype == torch.int32 and a2.shape == (ref_nchw.shape[0], Q, Q, 2)
    r = _windows(ref_nchw.permute(0, 2, 3, 1).to(a2.device), Q)
    neg = g2 < 0
    key = torch.where(neg.view(1, 1, 1, 32, 1), -r, r)
    top2 = key.topk(2, -1).values
    zero = (g2 == 0).view(1, 1, 1, 32)
    clear = ((top2[..., 0] - top2[..., 1]) > gap * r.abs().max()) | zero
    got = a2_decode(a2)
    want = torch.where(zero, torch.zeros_like(got), first_extreme(r, neg).to(got.dtype))
    assert clear.float().mean().item() > 0.5
    bad = (got != want) & clear
    assert not bad.any(), f"{int(bad.sum())} of {int(clear.sum())} windows lost their argmax"


def _check_forward(out, mag, yp, g2, b2, ref, reft, P, B, tag):
    """test_conv2_forward's assertions on one launch's results"""
    y2h, partial, ya, a2 = out
    assert y2h.dtype == torch.float16 and y2h.shape == (B, P, P, 32)
    v = y2h.float() * y2h_decode_factor(mag)  # y2 - b2 as stored (fp16 grid: 2^-11 relative)
    y2 = v + b2
    vmax = v.abs().max().item()
    e, sc = _err(y2.permute(0, 3, 1, 2), reft)
    print(f"{tag}: y2 err {e:.3e} bound {2.0 ** -10 * vmax + 1e-5 * sc:.3e}")
    assert e <= 2.0 ** -10 * vmax + 1e-5 * sc, (tag, e, vmax)
    ymax = yp.amax(1).view(torch.float32)
    assert ((ymax - v.abs().amax((0, 1, 2))).abs() <= 2.0 ** -10 * vmax).all(), tag
    s = partial.view(32, -1, 2).sum(1).cpu()
    yc = ref - b2.double().cpu().view(1, 32, 1, 1)
    yct = reft - b2.double().cpu().view(1, 32, 1, 1)
    _check_conv(s[:, 0], yc.sum((0, 2, 3)), yct.sum((0, 2, 3)), tag + " sum")
    _check_conv(s[:, 1], (yc * yc).sum((0, 2, 3)), (yct * yct).sum((0, 2, 3)), tag + " sumsq")
    Q = P // 2
    assert ya.dtype == torch.float16
    stored = y2h.float().permute(0, 3, 1, 2)[:, :, :2 * Q, :2 * Q]
    want = window_extreme(stored, (g2 < 0))
    want = torch.where((g2 == 0).view(1, 32, 1, 1), stored[:, :, 0::2, 0::2], want)
    got = pb_to_planar(ya, Q).float()
    assert torch.equal(got, want), (tag, (got - want).abs().max())
    _check_codes(a2, reft, g2, Q)


def _bits(ya, Q):
    return pb_to_planar(ya.view(torch.int16), Q)


def _run(gpu, small_grid, P, B, kind):
    ops = _ops()
    assert ops.device_cus() - NWG >= 0
    p, w2, b2, ref, reft = _case(gpu, P, B)
    g2 = _gamma(gpu, kind, 13 * P + B)
    res = {}
    for small in (False, True):
        small_grid(small)
        mag = new_mag(gpu, B, P)  # (sized by the grid: after the reserve is set)
        wp, _ = ops.conv2_pack(w2, mag)
        out = ops.fused_conv2_forward(p, wp, b2, g2, mag)
        ya_i = ops.fused_conv2_forward_inference(p, wp, g2, mag)
        if small:
            assert out[1].numel() == 32 * 3 * NWG * 2  # 96 workgroups' partial rows
        res[small] = (out, mag, ya_i, ypart(mag))  # (ypart's view while its grid is set)
    small_grid(False)
    torch.cuda.synchronize()
    Q = P // 2
    (full, mag_f, yai_f, yp_f), (few, mag_s, yai_s, yp_s) = res[False], res[True]
    # (b) a tile's bytes do not depend on the list that reaches it
    assert torch.equal(few[0].view(torch.int16), full[0].view(torch.int16)), "y2h depends on the workgroup count"
    assert torch.equal(_bits(few[2], Q), _bits(full[2], Q)), "ya depends on the workgroup count"
    assert torch.equal(few[3], full[3]), "a2 depends on the workgroup count"
    # (c) the inference launch's ya is the training launch's
    assert torch.equal(_bits(yai_f, Q), _bits(full[2], Q)), "inference ya differs (full grid)"
    assert torch.equal(_bits(yai_s, Q), _bits(few[2], Q)), "inference ya differs (96 workgroups)"
    assert few[2].float().abs().sum().item() > 0  # (not untouched buffers)
    # (a) both launches against the references
    _check_forward(full, mag_f, yp_f, g2, b2, ref, reft, P, B, f"P={P} B={B} {kind} full grid")
    _check_forward(few, mag_s, yp_s, g2, b2, ref, reft, P, B, f"P={P} B={B} {kind} 96 workgroups")


# (16, 2): one tile per image, nothing carried; (37, 3): odd size, border tiles on both edges, an
# unpooled last row, lists crossing images; (40, 1): 15 tiles, most workgroups have none, no look-ahead
# entry; (130, 1): 153 tiles, lists of 1-2; (392, 1): 1225 tiles, ~13 per list, border and interior
# tiles alternating within a list
@pytest.mark.parametrize("P,B", [(16, 2), (37, 3), (40, 1), (130, 1), (392, 1)])
def test_conv2_forward_long_lists(gpu, small_grid, P, B):
    _run(gpu, small_grid, P, B, "mixed")


@pytest.mark.parametrize("kind", ["positive", "half", "zero"])
@pytest.mark.parametrize("P,B", [(37, 3), (392, 1)])
def test_conv2_forward_gamma2_paths(gpu, small_grid, P, B, kind):
    _run(gpu, small_grid, P, B, kind)
