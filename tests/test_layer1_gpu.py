"""The layer-1 kernels (csrc/kernels/convnet_fused.hip: l1_conv_bf3_kernel, the Gram reducer,
l1_bwd_mfma_kernel + its finalizer) against fp64 references built on the CPU from the ops' inputs
(tests/_l1ref.py), with per-element bounds derived from the arithmetic -- no tolerance here is taken
from a kernel's output.

1. the conv + epilogue kernel alone on a hand-built affine (ops.fused_l1_forward_inference): both
   input types, every tile remainder, positive / mixed-sign / zero / 1e-3..1e3 BN1 scales, several
   tiles per workgroup, and the general (non-finite) epilogue's locality;
2. the training forward (ops.fused_l1_forward): statistics and Gram at the smallest images and at
   batches above 16, p1 within the bound of part 1, the argmax byte exactly on every window the fp64
   reference decides, designed exact ties, zero / negative gamma1, a poisoned batch;
3. the backward (ops.fused_l1_backward), its reference routed by the very idx1 the op is given, so
   that an argmax flip cannot move it and the bounds are arithmetic only.

The forward bound (per element, _l1ref.dz_bound / p1_bound).  The kernel forms
z = a * acc + (a * b1 + b) with acc the MFMA sum of the 25 products w1 * x:
  - a product on bf16x3 (fp32 image: hi*hi + hi*lo + lo*hi, lo*lo dropped) or bf16x2 (levels: the
    level exact, the weight hi + lo) is within 2^-16 relative (docs/KERNELS.md "Precision");
  - the 25 products are accumulated in fp32: <= 25 * 2^-24 < 2^-19 of sum |w1 x| more, so
    |acc - conv| <= 2^-15 (|w1| * |x|) (with a factor 2 left over the products' own 2^-16);
  - the epilogue's two fp32 FMAs (a b1 + b; a acc + that; for levels the 1/255 folded into a):
    <= 3 * 2^-24 < 2^-22 of |a conv| + |a b1 + b|.
  So dz = |a| 2^-15 (|w1| * |x|) + 2^-22 (|a conv| + |a b1 + b|) bounds |z - z_ref| per pixel; max
  and ReLU are 1-Lipschitz and p1 is rounded once to fp16, so
  |p1 - ref| <= max dz over the window + 2^-11 |ref|.
Where the kernel is handed the fp32 affine of the training forward while the reference keeps its fp64
one, 2^-22 (|a y| + |b|) is added for that rounding (a, b rounded to fp32; the statistics themselves are
fp64 in the kernel)."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import _l1ref as R
from test_fused_gpu import _check, _ops, dp1h_encode

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
SMALL_CUS = 8  # tds_device_cus' floor: 64 workgroups of the forward, 32-40 of the backward


@pytest.fixture
def small_grid():
    """-> switch(on): on leaves SMALL_CUS CUs to the persistent kernels, off all of them; the reserve
    is back at 0 after the test however it ends."""
    ops = _ops()
    ops.set_cu_reserve(0)
    total = ops.device_cus()

    def use(on):
        ops.set_cu_reserve(total - SMALL_CUS if on else 0)

    try:
        yield use
    finally:
        ops.set_cu_reserve(0)


def _to_image(x):
    from torch_distributed_sandbox_amd.models.convnet import to_image

    return to_image(x)


_CASES = {}


def _case(gpu, H, B, levels):
    """x (uint8 levels or an fp32 image), conv1's weights and bias of a shape and the fp64
    convolutions of them, computed once and left unchanged: the affine does not enter them."""
    key = (H, B, levels)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * H + 10 * B + int(levels))
        if levels:
            xin = torch.randint(0, 256, (B, 1, H, H), generator=g, dtype=torch.uint8)
        else:
            xin = torch.rand(B, 1, H, H, generator=g)
        _CASES[key] = _make_case(gpu, xin, *_conv1(g))
    return _CASES[key]


def _conv1(g):
    """conv1's weights and bias with test_layer1_forward's draws"""
    return torch.randn(16, 1, 5, 5, generator=g) * 0.2, torch.randn(16, generator=g) * 0.1


def _make_case(gpu, xin, w1, b1):
    x64 = _to_image(xin).double()  # the references of a level batch get to_image(levels)
    yc, ya = R.conv_parts(x64, w1)
    return SimpleNamespace(xin=xin.to(gpu), x64=x64, w1=w1.to(gpu), b1=b1.to(gpu), w64=w1.double(), b64=b1.double(),
                           yc=yc, ya=ya, B=xin.shape[0], H=xin.shape[2])


KINDS = ("positive", "mixed", "zero", "span")


def _affine(kind, seed):
    """a[16], b[16] fp32 as the kernel gets them.  positive: the fast epilogue, no channel folded;
    mixed: R.SIGNS (a negative channel in every lane group, one group all negative); zero: mixed with
    a = 0, b > 0 on channel 5 and a = 0, b < 0 on channel 10 -- one zero scale sends the whole launch to
    the general epilogue; span: |a| from 1e-3 to 1e3 across the channels.  (span, |a| < 1e-2: b = 0.05
    keeps z above fp16's subnormals, whose 2^-25 quantum the 2^-11 |ref| term does not cover and
    |a| 2^-15 (|w1| * |x|) only covers from |a| ~ 1e-3 up; the other channels cross zero.)"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.rand(16, generator=g) + 0.5
    b = torch.randn(16, generator=g) * 0.3
    if kind == "positive":
        a = mag
    elif kind == "mixed":
        a = mag * R.SIGNS.float()
    elif kind == "zero":
        a = mag * R.SIGNS.float()
        a[5], b[5], a[10], b[10] = 0.0, 0.25, 0.0, -0.25
    else:
        a = 10.0 ** torch.linspace(-3.0, 3.0, 16)[torch.randperm(16, generator=g)]
        b = torch.where(a < 1e-2, torch.full_like(b, 0.05), a * b)
    return a.float(), b.float()


def _aff33(gpu, a, b):
    return torch.cat([a, b, torch.ones(1)]).to(gpu)  # the kernel reads a and b only: p1 scale 1


def _ratio(err, bound):
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def _check_p1(p1, c, a, b, tag, rounded_affine=False):
    """p1 [B,P,P,16] fp16 finite and within the module docstring's bound of the fp64
    relu -> max-pool of z = a (conv + b1) + b; -> (err / bound's maximum, z, dz, ref)"""
    P = c.H // 2
    assert p1.dtype == torch.float16 and p1.shape == (c.B, P, P, 16), tag
    a64, b64 = a.double().cpu(), b.double().cpu()
    z, ref = R.p1_reference(a64, b64, c.b64, c.yc)
    dz = R.dz_bound(a64, b64, c.b64, c.yc, c.ya, rounded_affine)
    got = p1.double().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all(), tag
    worst = _ratio((got - ref).abs(), R.p1_bound(dz, ref)).max().item()
    print(f"{tag}: p1 err / bound {worst:.3f}")
    assert worst <= 1.0, f"{tag}: p1 err / bound {worst:.3f}"
    return worst, z, dz, ref


# ------------------------------------------------------------------ 1. conv + epilogue on a given affine
# H: 8 (half a tile row), 12, 20, 60 (one column tile, partly filled), 64 (exact), 68 (a 4-column second
# tile), 132 (three column tiles, nine tile rows); B = 17, 32: lists crossing many images
SHAPES = [(H, 3) for H in (8, 12, 20, 60, 64, 68, 132)] + [(20, 1), (20, 17), (20, 32)]
INPUTS = pytest.mark.parametrize("levels", [False, True], ids=["image", "levels"])


@INPUTS
@pytest.mark.parametrize("H,B", SHAPES)
def test_conv_epilogue_on_given_affine(gpu, H, B, levels):
    """l1_conv_bf3_kernel alone: p1 = fp16(relu(maxpool2(a (conv(x, w1) + b1) + b))) within the
    per-element bound of the module docstring, for every kind of affine (_affine)."""
    c = _case(gpu, H, B, levels)
    for k, kind in enumerate(KINDS):
        a, b = _affine(kind, 7 * H + B + k)
        p1 = _ops().fused_l1_forward_inference(c.xin, c.w1, c.b1, _aff33(gpu, a, b))
        _check_p1(p1, c, a, b, f"H={H} B={B} {'levels' if levels else 'image'} {kind}")


@INPUTS
def test_conv_epilogue_several_tiles_per_workgroup(gpu, small_grid, levels):
    """H = 264, B = 3 is 255 tiles: on 64 workgroups each walks 3 or 4 (the t += gridDim.x loop with
    the next tile's prefetch).  A tile's bytes may not depend on the list that reaches it: p1 bit-identical
    to the full grid's, and within the bound."""
    c = _case(gpu, 264, 3, levels)
    ops = _ops()
    for k, kind in enumerate(KINDS):
        a, b = _affine(kind, 90 + k)
        aff = _aff33(gpu, a, b)
        small_grid(False)
        full = ops.fused_l1_forward_inference(c.xin, c.w1, c.b1, aff)
        small_grid(True)
        few = ops.fused_l1_forward_inference(c.xin, c.w1, c.b1, aff)
        small_grid(False)
        assert torch.equal(few.view(torch.int16), full.view(torch.int16)), f"{kind}: p1 depends on the workgroup count"
        _check_p1(few, c, a, b, f"H=264 64 workgroups {'levels' if levels else 'image'} {kind}")


_BAD_PIXELS = {"row15_col63": (15, 63), "row15_col64": (15, 64), "row16_col0": (16, 0), "last": (131, 131)}


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("pix", list(_BAD_PIXELS))
def test_nonfinite_pixel_stays_local(gpu, pix, bad):
    """One NaN (or +inf) pixel of an fp32 image at a tile's last column / the next tile's first, at a
    tile's first row, at the image's last pixel; finite mixed-sign affine.  The tile holding it and the
    neighbours that see it only in their halo take the general epilogue (torch's NaN rule): p1 is NaN
    exactly where the fp64 max_pool2d(relu(z)) is, +inf exactly where that is +inf, and everywhere else
    finite and within the bound (formed with the pixel taken as 0: those windows do not see it, or see
    it as a -inf that neither ReLU nor the max passes).  The second image is clean."""
    H, B = 132, 2
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 1, H, H, generator=g)
    r, col = _BAD_PIXELS[pix]
    clean = x.clone()
    clean[0, 0, r, col] = 0.0
    x[0, 0, r, col] = bad
    w1, b1 = _conv1(g)
    c, cc = _make_case(gpu, x, w1, b1), _make_case(gpu, clean, w1, b1)
    a, b = _affine("mixed", 11)
    p1 = _ops().fused_l1_forward_inference(c.xin, c.w1, c.b1, _aff33(gpu, a, b))
    a64, b64 = a.double(), b.double()
    _, ref = R.p1_reference(a64, b64, c.b64, c.yc)
    got = p1.double().cpu().permute(0, 3, 1, 2)
    special = ~torch.isfinite(ref)
    assert special.any() and not special[1].any()  # (the case is real, and local in the reference)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (
        f"NaN in {int(torch.isnan(got).sum())} pooled values, the reference has {int(torch.isnan(ref).sum())}")
    assert torch.equal(torch.isinf(got), torch.isinf(ref)) and (got[torch.isinf(ref)] > 0).all()
    bound = R.p1_bound(R.dz_bound(a64, b64, c.b64, cc.yc, cc.ya), ref)
    worst = _ratio((got - ref).abs()[~special], bound[~special]).max().item()
    print(f"{pix} {bad}: p1 err / bound {worst:.3f}, {int(special.sum())} non-finite pooled values")
    assert worst <= 1.0


# ------------------------------------------------------------------ 2. the training forward
def _gamma(kind, seed):
    """gamma1, beta1 with test_layer1_forward's draws (rand + 0.5, randn * 0.1); mixed: R.SIGNS; zero:
    mixed with gamma = 0, beta > 0 on channel 5 and gamma = 0, beta < 0 on channel 10"""
    g = torch.Generator().manual_seed(seed)
    g1 = torch.rand(16, generator=g) + 0.5
    be1 = torch.randn(16, generator=g) * 0.1
    if kind != "positive":
        g1 = g1 * R.SIGNS.float()
    if kind == "zero":
        g1[5], be1[5], g1[10], be1[10] = 0.0, 0.25, 0.0, -0.25
    return g1, be1


def _forward(gpu, c, g1, be1, pre=False):
    """ops.fused_l1_forward on fresh running buffers (pre: on l1_input_stats' precomputed moments)
    -> (p1, idx1, stats, gram, p1_scale), running_mean, running_var, num_batches_tracked"""
    ops = _ops()
    rm, rv = torch.zeros(16, device=gpu), torch.ones(16, device=gpu)
    nbt = torch.zeros((), dtype=torch.long, device=gpu)
    moments = ops.l1_input_stats(c.xin) if pre else ()
    out = ops.fused_l1_forward(c.xin, c.w1, c.b1, g1.to(gpu), be1.to(gpu), rm, rv, nbt, MOM, EPS, *moments)
    return out, rm, rv, nbt


def _bn_affine(c, g1, be1):
    """the fp64 reference's BN1 affine z = a y + b of a case: a = gamma invstd, b = beta - a mean"""
    mean, invstd = R.bn_stats(c.yc + c.b64.view(1, 16, 1, 1), EPS)
    a = g1.double() * invstd
    return a, be1.double() - a * mean, mean, invstd


@INPUTS
@pytest.mark.parametrize("H,B", [(H, B) for H in (12, 16, 20, 28, 36) for B in (1, 3, 17, 32)] + [(68, 3)])
def test_training_forward_statistics(gpu, H, B, levels):
    """stats (mean | invstd), the running buffers (unbiased variance) and the Gram vs fp64, from the
    smallest image l1_gram takes (12) and at B > 16 (l1_build_gram's strip loop past its 16 loads in
    flight); the precomputed-moments entry (l1_input_stats) is bit-identical to the inline path."""
    c = _case(gpu, H, B, levels)
    g1, be1 = _gamma("mixed", H + B)
    (p1, idx1, stats, gram, p1s), rm, rv, nbt = _forward(gpu, c, g1, be1)
    y = c.yc + c.b64.view(1, 16, 1, 1)
    mean, invstd = R.bn_stats(y, EPS)
    n = B * H * H
    _check(stats[:16], mean, 1e-5, "mean")
    _check(stats[16:], invstd, 1e-5, "invstd")
    _check(rm, MOM * mean, 1e-5, "running_mean")
    _check(rv, (1 - MOM) + MOM * y.var((0, 2, 3), unbiased=False) * n / (n - 1), 1e-5, "running_var")
    assert int(nbt.item()) == 1 and p1s.item() == 1.0
    G, S = R.gram(c.x64)
    if levels:  # exact integer moments of the levels, scaled in fp64 by the fp32 constant
        sc = float(torch.tensor(1.0 / 255.0, dtype=torch.float32))
        Gl, Sl = R.gram(c.xin.double().cpu())
        _check(gram[:625].view(25, 25), Gl * (sc * sc), 1e-13, "G (levels)")
        _check(gram[625:], Sl * sc, 1e-13, "S (levels)")
        _check(gram[:625].view(25, 25), G, 1e-7, "G (image)")  # the fp32 image's own per-pixel rounding
    else:
        _check(gram[:625].view(25, 25), G, 2e-6, "G")
        _check(gram[625:], S, 2e-6, "S")
    (q1, qidx, qstats, qgram, _), qrm, qrv, qnbt = _forward(gpu, c, g1, be1, pre=True)
    for u, v, name in ((p1.view(torch.int16), q1.view(torch.int16), "p1"), (idx1, qidx, "idx1"), (stats, qstats, "stats"),
                       (gram, qgram, "gram"), (rm, qrm, "running_mean"), (rv, qrv, "running_var")):
        assert torch.equal(u, v), f"precomputed moments: {name} differs from the inline path"
    assert int(qnbt.item()) == 1


def _check_idx(idx1, z, dz, g1, tag, designed=None):
    """The argmax byte against the fp64 z [B,16,H,H] with its per-pixel bound dz.  A window is clear
    when its top two z differ by more than 2 dz (the kernel's order of the two cannot differ from the
    reference's): there bits 0-1 are the reference's first maximum in scan order.  Bit 2 is ref > 0
    wherever |top z| > dz; bits 3-7 are zero.  A channel with gamma = 0 ties everywhere: code 0, bit 2
    by the sign of beta (the caller checks it), not counted below, as windows tied by design
    (designed [B,P,P], checked by the caller) are not.  At most 0.5 % of the other windows may be
    unclear (the fp64 reference alone leaves 0.03-0.05 % with these draws).
    -> (unclear share, ReLU-unclear share)"""
    code = idx1.permute(0, 3, 1, 2).long().cpu()
    assert ((code & 0xF8) == 0).all(), f"{tag}: bits 3-7 of the argmax byte"
    zw, dw = R.windows(z), R.windows(dz).max(-1).values
    top2 = zw.topk(2, -1).values
    live = (g1 != 0).view(1, 16, 1, 1).expand_as(dw)
    if designed is not None:
        live = live & ~designed.unsqueeze(1)
    clear = ((top2[..., 0] - top2[..., 1]) > 2 * dw) & live
    bad = ((code & 3) != R.first_max(zw)) & clear
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {int(clear.sum())} clear windows lost their argmax"
    sure = (top2[..., 0].abs() > dw) & live
    bad = (((code & 4) != 0) != (top2[..., 0] > 0)) & sure
    assert not bad.any(), f"{tag}: {int(bad.sum())} ReLU bits differ from the reference"
    unclear = 1.0 - clear[live].float().mean().item()
    unsure = 1.0 - sure[live].float().mean().item()
    print(f"{tag}: unclear windows {100 * unclear:.3f} %, ReLU-unclear {100 * unsure:.3f} %")
    assert unclear <= 0.005, f"{tag}: {100 * unclear:.2f} % of the windows are unclear"
    return unclear, unsure


def _check_training_forward(gpu, c, kind, seed, tag):
    g1, be1 = _gamma(kind, seed)
    (p1, idx1, _, _, p1s), _, _, _ = _forward(gpu, c, g1, be1)
    assert p1s.item() == 1.0
    a, b, _, _ = _bn_affine(c, g1, be1)
    _, z, dz, _ = _check_p1(p1, c, a, b, tag, rounded_affine=True)
    _check_idx(idx1, z, dz, g1, tag)
    for ch in torch.nonzero(g1 == 0).flatten().tolist():
        # gamma = 0: z = beta at every pixel: p1 = beta (relu), code 0 (the first position), bit 2 = beta > 0
        want = torch.relu(be1[ch]).half().item()
        assert (p1[..., ch] == want).all(), f"{tag}: p1 of channel {ch} (gamma 0) is not relu(beta)"
        assert (idx1[..., ch] == (4 if be1[ch] > 0 else 0)).all(), f"{tag}: idx1 of channel {ch} (gamma 0)"
    return p1, idx1


@INPUTS
@pytest.mark.parametrize("kind", ["positive", "mixed", "zero"])
@pytest.mark.parametrize("H", [20, 68, 132])
def test_training_forward_p1_and_argmax(gpu, H, kind, levels):
    """p1 within the bound with the fp64 reference's own a = gamma invstd, b = beta - a mean, and the
    argmax byte exactly (_check_idx); mixed-sign gamma1 folds the sign into conv1's weights and pools the
    accumulators, a zero gamma1 takes the general epilogue."""
    _check_training_forward(gpu, _case(gpu, H, 3, levels), kind, 3 * H, f"H={H} {'levels' if levels else 'image'} {kind}")


@INPUTS
def test_training_forward_several_tiles_per_workgroup(gpu, small_grid, levels):
    """H = 264, B = 3 on 64 workgroups: p1 and idx1 bit-identical to the full grid's, and both right."""
    c = _case(gpu, 264, 3, levels)
    small_grid(True)
    p1, idx1 = _check_training_forward(gpu, c, "mixed", 264, f"H=264 64 workgroups {'levels' if levels else 'image'}")
    small_grid(False)
    g1, be1 = _gamma("mixed", 264)
    (q1, qidx, _, _, _), _, _, _ = _forward(gpu, c, g1, be1)
    assert torch.equal(p1.view(torch.int16), q1.view(torch.int16)), "p1 depends on the workgroup count"
    assert torch.equal(idx1, qidx), "idx1 depends on the workgroup count"


@INPUTS
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["signs", "flipped"])
def test_training_forward_exact_ties(gpu, sign, levels):
    """Constant blocks of levels 0, 255 and 128: a window whose four 5 x 5 patches (zero padding
    included) are the same integer array has four bit-equal accumulators, and the code must be 0,
    torch's choice, for a positive and for a negative gamma (R.SIGNS and its negation give every
    channel both).  The 0 blocks touch two image corners (the padding is level 0 too), a 255 block
    straddles the tile boundary at column 64."""
    H, B = 68, 3
    g = torch.Generator().manual_seed(68)
    lv = torch.randint(0, 256, (B, 1, H, H), generator=g, dtype=torch.uint8)
    lv[0, 0, :12, :12] = 0
    lv[0, 0, -12:, -12:] = 0
    lv[1, 0, 20:32, 56:68] = 255
    lv[2, 0, 4:14, 40:50] = 255
    lv[2, 0, 30:40, 20:30] = 128
    c = _make_case(gpu, lv if levels else _to_image(lv), *_conv1(g))
    pw = R.windows(F.unfold(lv.double(), 5, padding=2).view(B, 25, H, H))  # [B,25,P,P,4]
    tie = (pw == pw[..., :1]).all(-1).all(1)  # [B,P,P]
    assert tie[0, 0, 0] and tie[0, -1, -1] and tie[1, :, 31].any() and tie[1, :, 32].any() and tie[2].sum() >= 8
    g1, be1 = _gamma("positive", 4)
    g1 = g1 * R.SIGNS.float() * sign
    (p1, idx1, _, _, _), _, _, _ = _forward(gpu, c, g1, be1)
    a, b, _, _ = _bn_affine(c, g1, be1)
    tag = f"ties {'levels' if levels else 'image'} sign {sign:+.0f}"
    _, z, dz, _ = _check_p1(p1, c, a, b, tag, rounded_affine=True)
    _check_idx(idx1, z, dz, g1, tag, designed=tie)
    codes = (idx1.cpu() & 3)[tie]  # [windows, 16]
    assert (codes == 0).all(), f"{tag}: {int((codes != 0).sum())} of {codes.numel()} exactly tied windows not at code 0"


def test_training_forward_poisoned_batch(gpu):
    """One NaN pixel in an fp32 batch: every p1, every statistic and both running buffers are NaN, as
    torch's batch norm makes them, and num_batches_tracked advances by 1."""
    c0 = _case(gpu, 20, 3, False)
    x = c0.xin.clone()
    x[1, 0, 7, 9] = float("nan")
    g1, be1 = _gamma("mixed", 1)
    c = SimpleNamespace(xin=x, w1=c0.w1, b1=c0.b1)
    (p1, _, stats, _, _), rm, rv, nbt = _forward(gpu, c, g1, be1)
    assert torch.isnan(p1).all() and torch.isnan(stats).all() and torch.isnan(rm).all() and torch.isnan(rv).all()
    assert int(nbt.item()) == 1


# ------------------------------------------------------------------ 3. the backward
U24x64 = 64 * 2.0 ** -24


def _backward_reference(c, idx1, dp1, g1, be1):
    """fp64 autograd of batch_norm(conv2d(x)) under the dense dz1 built from the idx1 and the decoded
    dp1 the op receives, and the per-element bounds of test_backward's docstring.
    -> (stats, gram for the op, {name: (reference, bound)})"""
    n = c.B * c.H * c.H
    y = c.yc + c.b64.view(1, 16, 1, 1)
    mean, invstd = R.bn_stats(y, EPS)
    G, S = R.gram(c.x64)
    dz = R.dense_dz(idx1, dp1)
    prm = [t.clone().requires_grad_() for t in (c.w64, c.b64, g1.double(), be1.double())]
    yy = F.conv2d(c.x64, prm[0], prm[1], padding=2)
    F.batch_norm(yy, None, None, prm[2], prm[3], True, MOM, EPS).backward(dz)
    dw, db, dg, dbe = (p.grad for p in prm)
    dw = dw.view(16, 25)
    # the closed form the kernels use is an identity of that autograd (checked here, on the CPU)
    T, sdz = R.patch_sums(dz, c.x64)
    form = lambda T: R.l1_closed_form(T, sdz, G, S, c.w64.view(16, 25), c.b64, g1.double(), mean, invstd, n)
    for u, v in zip(form(T), (dw, dg, dbe)):
        assert (u - v).abs().max() <= 1e-9 * max(1.0, v.abs().max().item())
    if c.xin.dtype == torch.uint8:
        Te = T  # a level and the fp16 dz1 are exact MFMA operands: every product is exact
    else:
        # bf16x3.h on the operands as l1_bwd_mfma_kernel splits them (dz1 and x into bf16 hi + lo, the
        # lo * lo product dropped), arithmetic exact.  (dz1 is an fp16 value times a power of two: its hi +
        # lo is exact; x keeps 16 of its 24 bits)
        (dh, dl), (xh, xl) = R.bf16_split(dz), R.bf16_split(c.x64)
        Te = R.patch_sums(dh, xh)[0] + R.patch_sums(dh, xl)[0] + R.patch_sums(dl, xh)[0]
    ew, eg, ebe = form(Te)
    a = g1.double().abs() * invstd
    adz = dz.abs()
    mag_w = R.patch_sums(adz, c.x64.abs())[0] * a.view(16, 1)
    mag_be = adz.sum((0, 2, 3))
    mag_g = (adz * (y - mean.view(1, 16, 1, 1)).abs()).sum((0, 2, 3)) * invstd
    bound = lambda e, r, m: torch.maximum(1.5 * (e - r).abs(), U24x64 * m)
    refs = {"dw1": (dw, bound(ew, dw, mag_w)), "db1": (db, U24x64 * a * mag_be),
            "dgamma1": (dg, bound(eg, dg, mag_g)), "dbeta1": (dbe, bound(ebe, dbe, mag_be))}
    return torch.cat([mean, invstd]).float(), torch.cat([G.flatten(), S]), refs


def _check_backward(out, refs, tag):
    worst = {}
    for o, name in zip(out, ("dw1", "db1", "dgamma1", "dbeta1")):
        ref, bound = refs[name]
        got = o.double().cpu().view(ref.shape)
        assert torch.isfinite(got).all(), f"{tag} {name}"
        worst[name] = _ratio((got - ref).abs(), bound).max().item()
    print(f"{tag}: err / bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= 1.0, f"{tag}: {name} err / bound {v:.3f}"


def _backward_inputs(gpu, P, B, levels, own_idx=False):
    c = _case(gpu, 2 * P, B, levels)
    g = torch.Generator().manual_seed(31 * P + B)
    g1, be1 = _gamma("mixed", P + B)
    g1[5] = 0.0
    dp1h, dec, dp1 = dp1h_encode(torch.randn(B, P, P, 16, generator=g).to(gpu), 2.0 ** -9)
    p1 = torch.zeros(B, P, P, 16, dtype=torch.float16, device=gpu)  # (the kernel routes by idx1 alone)
    if own_idx:
        (p1, idx1, _, _, _), _, _, _ = _forward(gpu, c, g1, be1)
    else:  # every slot with the ReLU bit both ways, in every lane position
        idx1 = torch.randint(0, 8, (B, P, P, 16), generator=g, dtype=torch.uint8).to(gpu)
    stats, gram, refs = _backward_reference(c, idx1.cpu(), dp1.double().cpu(), g1, be1)
    args = (c.xin, p1, idx1, c.w1, c.b1, g1.to(gpu), stats.to(gpu), gram.to(gpu))
    return dp1h, dec, args, refs


# P % 4 = 2: dp1h's last column group is half padding (66: a partial third column tile); 32, 64: exact fits
BWD_SHAPES = [(6, 3), (10, 3), (34, 3), (66, 3), (32, 3), (64, 3), (10, 17), (10, 32)]


@INPUTS
@pytest.mark.parametrize("P,B,own", [(P, B, False) for P, B in BWD_SHAPES] + [(34, 3, True)])
def test_backward(gpu, P, B, own, levels):
    """ops.fused_l1_backward against fp64 autograd of batch_norm(conv2d(x)) under the dense dz1 built
    from the idx1 (bits 0-1 the slot, bit 2 the ReLU mask) and the decoded dp1 the op itself gets:
    random bytes 0..7 (own: the forward's own idx1 instead), so an argmax
    flip cannot enter and the bounds are arithmetic only.  gamma1 has mixed signs and a zero channel.

    What carries error is T = sum dz1 (x) xpatch and sum dz1: fp32 image on bf16x3 operands, levels
    with exact products; 256 pixels accumulated in fp32 per tile, fp64 beyond.  The operand rounding is
    emulated in fp64 (v -> bf16(v) + bf16(v - bf16(v)), lo * lo dropped: bf16x3.h as the kernel uses it)
    and pushed through the closed form; that emulation's own distance from the fp64 autograd is the
    yardstick, as tests/_tf32ref.py is for conv2.  Per element, each of dw1, dgamma1, dbeta1 lies within
      max(1.5 x that distance, 64 * 2^-24 * magnitude),
    1.5 the margin the conv2 tests use over an operand-rounded reference, the second term for the fp32
    accumulation and the fp32 outputs, with magnitudes sum |dz1| |x| |gamma| invstd (dw1), sum |dz1|
    (dbeta1) and sum |dz1| |y - mean| invstd (dgamma1).  db1 is analytically zero:
    |db1| <= 64 * 2^-24 |gamma| invstd sum |dz1|.

    Also: fp16 NaNs in dp1h's padding columns (pixels >= P of the last group) change nothing, and
    scale = 0.5 gives exactly half of every output."""
    dp1h, dec, args, refs = _backward_inputs(gpu, P, B, levels, own_idx=own)
    ops = _ops()
    out = ops.fused_l1_backward(dp1h, dec, *args, 1.0)
    _check_backward(out, refs, f"P={P} B={B} {'levels' if levels else 'image'}{' own idx1' if own else ''}")
    if P % 4:
        poisoned = dp1h.clone()
        poisoned[:, :, -1, :, P % 4:] = float("nan")
        for u, v, name in zip(ops.fused_l1_backward(poisoned, dec, *args, 1.0), out, ("dw1", "db1", "dgamma1", "dbeta1")):
            assert torch.equal(u, v), f"{name} reads dp1h's padding columns"
    for u, v, name in zip(ops.fused_l1_backward(dp1h, dec, *args, 0.5), out, ("dw1", "db1", "dgamma1", "dbeta1")):
        assert torch.equal(u, v * 0.5), f"{name} at scale 0.5 is not half of scale 1"


@INPUTS
def test_backward_several_tiles_per_workgroup(gpu, small_grid, levels):
    """P = 132, B = 3 is 255 tiles: on 32-40 workgroups each sums 6-8 of them in fp64 behind the
    prefetch of the next.  The partial rows differ from the full grid's, so each launch is held to the
    reference, not to the other bit for bit."""
    dp1h, dec, args, refs = _backward_inputs(gpu, 132, 3, levels)
    ops = _ops()
    for small in (False, True):
        small_grid(small)
        out = ops.fused_l1_backward(dp1h, dec, *args, 1.0)
        small_grid(False)
        _check_backward(out, refs, f"P=132 {'levels' if levels else 'image'} {'small' if small else 'full'} grid")
