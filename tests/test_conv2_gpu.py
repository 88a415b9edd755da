"""The conv2 kernels (conv2_pack, conv2_fwd2_kernel with and without its in-launch BN2 finalize,
conv2_bwd_roll_kernel) against fp64 references per element (tests/_conv2ref.py; docs/KERNELS.md
"conv2 tests").  Every bound comes from the arithmetic documented in conv2_common.h / conv2_pack.h
and from the op's inputs, none from a kernel's output; the power-of-two factors the kernels publish
in mag[40..44] are first asserted to be what the headers say, then used as decodes.

Each test prints the worst err / bound of every quantity it checks (pytest -s shows them)."""
import copy
import types

import pytest
import torch

import _conv2ref as R
from test_fused_gpu import (_ops, a2_decode, a2_encode, dp1h_decode, mag_floats, new_mag, pb_to_planar, window_extreme,
                            y2h_decode_factor, ypart)

pytestmark = pytest.mark.gpu

MOM, EPS = 0.1, 1e-5
SEG = 48  # tiles per vertical segment of the backward's walk (fused_ops.cpp bwd_walk)


@pytest.fixture
def small_grid():
    """-> use(ncu): leaves ncu CUs to the persistent kernels (None: all of them; the forward launches
    3 workgroups on each, the backward 1; the project keeps at least 8); the reserve is back at 0
    after the test however it ends."""
    ops = _ops()
    ops.set_cu_reserve(0)
    total = ops.device_cus()

    def use(ncu):
        ops.set_cu_reserve(0 if ncu is None else total - ncu)
        return ops.device_cus()

    try:
        yield use
    finally:
        ops.set_cu_reserve(0)


def _report(tag, ratios):
    print(f"{tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert R.ok(ratios), (tag, {k: v for k, v in ratios.items() if not v <= 1.0})


# ------------------------------------------------------------------------------------ 1. the pack
def _weights(kind, gpu, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randn(32, 16, 5, 5, generator=g) * 0.05
    if kind == "tiny":
        w = w * 1e-4  # randn * 5e-6: below fp16's normal range unscaled
    elif kind == "large":
        w = w * 6e4  # randn * 3e3
    elif kind == "one channel x100":
        w[11] *= 100
    elif kind == "one channel zero":
        w[11] = 0
    elif kind == "zero":
        w = torch.zeros_like(w)
    return w.to(gpu)


@pytest.mark.parametrize("kind", ["randn", "tiny", "large", "one channel x100", "one channel zero", "zero"])
def test_pack_scales_and_words(gpu, kind):
    """mag[40] = 2^-ew and mag[41] = 1 / p1 scale exactly; 2^k and 2^kd the powers of two of the
    documented inequalities (the ones that decide whether y2h / dp1h can overflow); wp and wd, through
    the index maps of conv2_pack.h, bit-equal to fp16(w 2^ew) at every (co, ci, tap), the ky = 5 slots 0."""
    ops = _ops()
    w = _weights(kind, gpu)
    s = 2.0 ** -3
    mag = new_mag(gpu, 2, 16)
    wp, wd = ops.conv2_pack(w, mag, torch.tensor([s], device=gpu), True)
    m = mag_floats(mag).cpu()
    ew, k, kd = R.check_pack_scales(m[40].item(), m[41].item(), m[42].item(), m[43].item(), w, s)
    print(f"{kind}: ew {ew} k {k} kd {kd}")
    assert (mag[:33] == 0).all()  # the step's bounds are reset
    want = R.packed_weights(w, ew).view(torch.int16)
    taps, pad = R.unpack_wp(wp)
    assert torch.equal(taps.view(torch.int16), want)
    assert (pad.view(torch.int16) == 0).all()
    assert torch.equal(R.unpack_wd(wd).view(torch.int16), want)


# ------------------------------------------------------------------------------------ 2. forward
_FWD = {}


def _p1(gpu, P, B, s, seed, sparse=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, P, P, 16, generator=g)
    return (torch.relu(x - 1.6 if sparse else x) * s).half().to(gpu)  # (s a power of two: p1h / s exact)


def _fwd_case(gpu, P, B, s=1.0, seed=None, sparse=False):
    """p1h, weights, bias and the fp64 reference of a shape, computed once (gamma2 enters the window
    checks only)"""
    key = (P, B, s, seed, sparse)
    if key not in _FWD:
        p1h = _p1(gpu, P, B, s, 17 * P + B if seed is None else seed, sparse)
        w2 = _weights("randn", gpu, seed=3 * P + B)
        b2 = torch.randn(32, generator=torch.Generator(device="cpu").manual_seed(P)).to(gpu)
        r = R.fwd_reference(p1h, w2, R.pack_ew(w2), s, b2, torch.ones(32))
        r.sums = R.sums_reference(r)
        _FWD[key] = (p1h, w2, b2, r)
    return _FWD[key]


def _gamma(gpu, kind, seed):
    r = torch.randn(32, generator=torch.Generator(device="cpu").manual_seed(seed))
    if kind == "positive":
        r = r.abs() + 0.1
    elif kind == "zero":
        r = r.abs() + 0.1
        r[5] = 0.0
    return r.to(gpu)


def _with_gamma(r, g2):
    r = copy.copy(r)
    r.g2 = g2.detach().double().cpu()
    r.want, r.clear = R.fwd_codes(r)
    return r


def _pack(ops, gpu, w2, s, B, P):
    """conv2_pack into a fresh workspace (sized by the grid: after the reserve is set); the scales
    asserted, -> (mag, wp, wd, d = the y2h decode, ew, k, kd)"""
    mag = new_mag(gpu, B, P)
    wp, wd = ops.conv2_pack(w2, mag, torch.tensor([s], device=gpu), True)
    m = mag_floats(mag).cpu()
    ew, k, kd = R.check_pack_scales(m[40].item(), m[41].item(), m[42].item(), m[43].item(), w2, s)
    d = 2.0 ** -ew / s / 2.0 ** k
    assert y2h_decode_factor(mag) == d
    return mag, wp, wd, d, ew, k, kd


def _check_windows(r, y2h, ya, a2, tag):
    """ya bit-equal to the extreme of the window's stored y2h (position 0 where gamma2 == 0); a2 the
    reference's first extreme on every clear window; -> the code ratios and the unclear share"""
    Q = r.P // 2
    g2 = r.g2.to(y2h.device)
    stored = y2h.float().permute(0, 3, 1, 2)[:, :, :2 * Q, :2 * Q]
    want = window_extreme(stored, g2 < 0)
    want = torch.where((g2 == 0).view(1, 32, 1, 1), stored[:, :, 0::2, 0::2], want)
    got = pb_to_planar(ya, Q).float()
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    assert bool(same.all()), (tag, "ya is not the window extreme of the stored y2h")
    assert a2.dtype == torch.int32 and a2.shape == (r.B, Q, Q, 2)
    return R.check_fwd_codes(r.want, r.clear, a2_decode(a2))


def _bn_buffers(gpu, seed=9):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(32, generator=g).to(gpu) * 0.3, (torch.rand(32, generator=g) + 0.5).to(gpu),
            torch.tensor(7, dtype=torch.int64, device=gpu))


def _forward_both(ops, gpu, p1h, w2, b2, g2, be2, s, bufs):
    """fused_conv2_forward and fused_conv2_forward_bn on the current grid, each into a workspace of
    its own; -> a namespace of everything they return (ymax read while the grid is set)"""
    B, P = p1h.shape[:2]
    o = types.SimpleNamespace()
    mag, wp, _, o.d, _, _, _ = _pack(ops, gpu, w2, s, B, P)
    o.y2h, partial, o.ya, o.a2 = ops.fused_conv2_forward(p1h, wp, b2, g2, mag)
    o.nwg = ops.mag_ypart_count()
    assert partial.numel() == 32 * o.nwg * 2
    o.partial = partial.view(32, o.nwg, 2).sum(1)
    o.ymax = ypart(mag).amax(1).view(torch.float32).clone()
    magb, wpb, _, _, _, _, _ = _pack(ops, gpu, w2, s, B, P)
    rm, rv, nbt = bufs
    o.rm0, o.rv0, o.nbt0 = rm.clone(), rv.clone(), int(nbt)
    o.y2h_b, o.ya_b, o.a2_b, o.stats2, o.aff2 = ops.fused_conv2_forward_bn(p1h, wpb, b2, g2, be2, rm, rv, nbt, MOM, EPS,
                                                                           magb)
    o.rm, o.rv, o.nbt = rm.clone(), rv.clone(), int(nbt)
    o.mag_y = mag_floats(magb)[:32].clone()
    return o


def _bits(t):
    return t.view(torch.int16)


def _check_forward(r, o, b2, g2, be2, tag, keep=None):
    """every forward check of one grid's pair of launches; -> (ratios, unclear share)"""
    assert o.y2h.dtype == torch.float16 and o.y2h.shape == (r.B, r.P, r.P, 32)
    assert torch.equal(_bits(o.y2h_b), _bits(o.y2h)), (tag, "y2h differs with the in-launch finalize")
    assert torch.equal(_bits(o.ya_b), _bits(o.ya)), (tag, "ya differs with the in-launch finalize")
    assert torch.equal(o.a2_b, o.a2), (tag, "a2 differs with the in-launch finalize")
    ratios = R.check_fwd_values(r, o.y2h, o.d, keep)
    codes, unclear = _check_windows(r, o.y2h, o.ya, o.a2, tag)
    ratios.update(codes)
    if keep is None:
        ratios.update(R.check_partial(r.sums, o.partial))
        ratios.update(R.check_ymax(r, o.ymax))
        ratios.update({"mag " + k: v for k, v in R.check_ymax(r, o.mag_y).items()})
        bn = R.bn_reference(r.sums, b2, g2, be2, o.rm0, o.rv0, MOM, EPS)
        ratios.update(R.check_bn(bn, o.stats2, o.aff2, o.rm, o.rv))
        assert o.nbt == o.nbt0 + 1
    return ratios, unclear


def _run_forward(gpu, small_grid, P, B, kind, s=1.0):
    ops = _ops()
    p1h, w2, b2, r0 = _fwd_case(gpu, P, B, s)
    g2 = _gamma(gpu, kind, 13 * P + B)
    be2 = _gamma(gpu, "mixed", 29 * P + B)
    r = _with_gamma(r0, g2)
    res = {}
    for ncu in (None, 32):
        small_grid(ncu)
        res[ncu] = _forward_both(ops, gpu, p1h, w2, b2, g2, be2, s, _bn_buffers(gpu))
    small_grid(None)
    torch.cuda.synchronize()
    assert res[32].nwg == 96
    # a tile's bytes do not depend on the list that reaches it
    assert torch.equal(_bits(res[32].y2h), _bits(res[None].y2h)), "y2h depends on the workgroup count"
    assert torch.equal(_bits(res[32].ya), _bits(res[None].ya)), "ya depends on the workgroup count"
    assert torch.equal(res[32].a2, res[None].a2), "a2 depends on the workgroup count"
    for ncu, o in res.items():
        tag = f"P={P} B={B} {kind} s={s} {'full grid' if ncu is None else '96 workgroups'}"
        ratios, unclear = _check_forward(r, o, b2, g2, be2, tag)
        print(f"{tag}: unclear windows {100 * unclear:.3f} %")
        _report(tag, ratios)


# (8, 1): one tile; (17, 2): odd, a 1-pixel second tile column, an unpooled last row and column;
# (34, 5): the smallest P with an interior-DMA tile, the bench's B; (37, 3): odd, border and interior
# tiles; (72, 2): a larger even size; (10, 63): the backward's image-field limit
SHAPES = [(8, 1), (17, 2), (34, 5), (37, 3), (72, 2), (10, 63)]


@pytest.mark.parametrize("kind", ["mixed", "positive", "zero"])
@pytest.mark.parametrize("P,B", SHAPES)
def test_forward_per_element(gpu, small_grid, P, B, kind):
    """|y2h d - ref| <= 1.01 416 u A + 2^-11 |ref| + 2^-25 d at every pixel of both launches (bit-identical
    y2h / ya / a2) on the full and the 96-workgroup grid; ya, a2, the BN2 partials, ypart and the
    in-launch finalize's outputs per channel."""
    _run_forward(gpu, small_grid, P, B, kind)


@pytest.mark.parametrize("P,B", [(17, 2), (37, 3)])
def test_forward_p1_scale(gpu, small_grid, P, B):
    """conv2_pack(p1_scale = 2^-3, write_p1=True): mag[41] = 8, and the forward takes the scale out"""
    _run_forward(gpu, small_grid, P, B, "mixed", s=2.0 ** -3)


# ------------------------------------------------------------------------------------ 3. BN2 in the launch
def _bn_launch(ops, gpu, p1h, w2, b2, g2, be2, bufs):
    B, P = p1h.shape[:2]
    mag, wp, _, d, _, _, _ = _pack(ops, gpu, w2, 1.0, B, P)
    rm, rv, nbt = bufs
    rm0, rv0 = rm.clone(), rv.clone()
    _, _, _, stats2, aff2 = ops.fused_conv2_forward_bn(p1h, wp, b2, g2, be2, rm, rv, nbt, MOM, EPS, mag)
    return rm0, rv0, stats2, aff2, rm.clone(), rv.clone(), mag_floats(mag)[:32].clone()


def _check_bn_launch(r, b2, g2, be2, res, **mut):
    rm0, rv0, stats2, aff2, rm, rv, mag_y = res
    sums = R.sums_reference(r, n=mut.pop("n")) if "n" in mut else r.sums
    ratios = R.check_bn(R.bn_reference(sums, b2, g2, be2, rm0, rv0, MOM, EPS, **mut), stats2, aff2, rm, rv)
    ratios.update({"mag " + k: v for k, v in R.check_ymax(r, mag_y).items()})
    return ratios


# all CUs; 33 CUs = 99 workgroups: groups of 32, 32, 32 and 3; one group: the fewest CUs the project
# leaves its persistent kernels (asked for 1; tds_device_cus keeps 8: 24 workgroups, a partial group)
@pytest.mark.parametrize("ncu", [None, 33, 1])
@pytest.mark.parametrize("P,B", [(37, 3), (34, 5)])
def test_bn_finalize_grids(gpu, small_grid, P, B, ncu):
    """stats2, aff2, the running statistics from non-trivial buffers, num_batches_tracked and
    mag[0..32) of fused_conv2_forward_bn per channel against fp64, gamma2 = 0 in one channel (a = 0,
    b = beta2 exactly)"""
    ops = _ops()
    p1h, w2, b2, r = _fwd_case(gpu, P, B)
    g2, be2 = _gamma(gpu, "zero", P), _gamma(gpu, "mixed", P + 1)
    have = small_grid(ncu)
    nwg = ops.mag_ypart_count()
    assert nwg == 3 * have
    if ncu == 33:
        assert nwg == 99
    if ncu == 1:
        assert nwg <= 32  # one group
    bufs = _bn_buffers(gpu)
    res = _bn_launch(ops, gpu, p1h, w2, b2, g2, be2, bufs)
    small_grid(None)
    torch.cuda.synchronize()
    assert int(bufs[2]) == 8
    _report(f"P={P} B={B} {nwg} workgroups", _check_bn_launch(r, b2, g2, be2, res))


def test_bn_counters_across_grids(gpu, small_grid):
    """full, 99, one group, full, full back to back on one stream: a fresh p1 per launch, the same BN
    buffers, a fresh workspace sized after the reserve is set.  A group counter or the groups' counter
    not back at 0, or a stale group of a wider grid, would finalize early or never: every launch must
    meet the bounds, and num_batches_tracked ends at + 5."""
    ops = _ops()
    P, B = 37, 3
    g2, be2 = _gamma(gpu, "mixed", 71), _gamma(gpu, "mixed", 72)
    bufs = _bn_buffers(gpu)
    launches = []
    for i, ncu in enumerate((None, 33, 1, None, None)):
        p1h, w2, b2, r = _fwd_case(gpu, P, B, seed=1000 + i)
        small_grid(ncu)
        launches.append((r, b2, ops.mag_ypart_count(), _bn_launch(ops, gpu, p1h, w2, b2, g2, be2, bufs)))
    small_grid(None)
    torch.cuda.synchronize()
    assert int(bufs[2]) == 7 + 5
    for i, (r, b2, nwg, res) in enumerate(launches):
        _report(f"launch {i} ({nwg} workgroups)", _check_bn_launch(r, b2, g2, be2, res))


def test_bn_one_window_image(gpu):
    """n = 4 (B = 1, P = 2: one pooling window): the unbiased variance of running_var is 4/3 of the biased"""
    ops = _ops()
    p1h, w2, b2, r = _fwd_case(gpu, 2, 1)
    g2, be2 = _gamma(gpu, "mixed", 3), _gamma(gpu, "mixed", 4)
    bufs = _bn_buffers(gpu)
    res = _bn_launch(ops, gpu, p1h, w2, b2, g2, be2, bufs)
    torch.cuda.synchronize()
    _report("P=2 B=1", _check_bn_launch(r, b2, g2, be2, res))
    assert not R.ok(_check_bn_launch(r, b2, g2, be2, res, biased_running=True))


# ------------------------------------------------------------------------------------ 4. backward
def _k_set(kind, seed, hd):
    """k1, k2, k3 with the three terms of dy2 = k1 dz + k2 (h d + b2) + k3 of like size, so that each
    is held by the bounds (hd: the size of y2 - b2 = h d; dz is O(1): _bwd_inputs)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    k1, k2, k3 = torch.randn(32, generator=g), torch.randn(32, generator=g) * 0.5 / hd, torch.randn(32, generator=g) * 0.5
    if kind == "k1 zero":
        k1[[0, 9, 17, 31]] = 0
    elif kind == "k2 k3 zero":  # dy2 is the routed dz alone: exact zeros elsewhere
        k2[[2, 9, 16, 30]] = 0
        k3[[2, 9, 16, 30]] = 0
    elif kind in ("1e-7", "3e4"):
        k1, k2, k3 = (t * float(kind) for t in (k1, k2, k3))
    elif kind == "1e4 apart":  # one e for channels four decades apart
        f = torch.where(torch.arange(32) % 3 == 0, 1e-4, 1.0)
        k1, k2, k3 = k1 * f, k2 * f, k3 * f
    return k1, k2, k3


def _bwd_inputs(gpu, P, B, seed, s):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Q = P // 2
    x = types.SimpleNamespace(P=P, B=B, s=s)
    x.y2h = (torch.randn(B, P, P, 32, generator=g) * 200).half().to(gpu)
    x.codes = torch.randint(0, 4, (B, Q, Q, 32), generator=g).to(gpu)
    x.a2 = a2_encode(x.codes)
    x.ginv = (2.0 ** torch.randint(-11, -6, (32,), generator=g).float()).to(gpu)  # g2m ginv = dz: 0.15 .. 2.3 randn
    buf = torch.zeros(B * 32 * Q * Q + 32, dtype=torch.float16, device=gpu)  # (the slack the op demands)
    x.g2m = buf[:B * 32 * Q * Q].view(B, 32, Q, Q)
    x.g2m.copy_((torch.randn(B, 32, Q, Q, generator=g) * 300).half())
    x.b2 = torch.randn(32, generator=g).to(gpu)
    x.aff2 = torch.randn(64, generator=g).to(gpu)
    x.p1h = _p1(gpu, P, B, s, seed + 1)
    x.w2 = _weights("randn", gpu, seed=seed + 2)
    x.hd = 200 * R.pack_d(x.w2, s)  # (the documented scale choices; _pack asserts the kernel's)
    return x


def _longest_list(ops, B, P, nwg):
    t = ops.conv2_bwd_walk_table(B, (P + 7) // 8, (P + 15) // 16, nwg, SEG).to(torch.int64) & 0xFFFFFFFF
    return int(((t & (1 << 30)) == 0).sum(0).max())


def _bwd_launch(ops, gpu, x, k, scale, sinks=False):
    """one fused_conv2_backward_y2 on the current grid with mag[0..33) = the true bounds"""
    k1, k2, k3 = (t.to(gpu) for t in k)
    o = types.SimpleNamespace()
    mag, _, wd, o.d, o.ew, _, o.kd = _pack(ops, gpu, x.w2, x.s, x.B, x.P)
    m = mag_floats(mag)
    m[:32] = (x.y2h.float() * o.d).abs().amax((0, 1, 2))  # max |y2 - b2| (exact: d a power of two)
    m[32] = (x.g2m.float() * x.ginv.view(1, 32, 1, 1)).abs().max()
    o.ymax, o.gmax = m[:32].clone(), m[32].item()
    kbuf = torch.cat([k1, k2, k3, x.ginv]).float().contiguous()
    dw_out = torch.full((32, 16, 5, 5), 7.0, device=gpu) if sinks else None
    db_out = torch.full((32,), 7.0, device=gpu) if sinks else None
    o.dp1h, o.dw2, o.db2 = ops.fused_conv2_backward_y2(x.y2h, x.a2, x.g2m, x.aff2, kbuf, x.b2, mag, x.p1h, wd, scale,
                                                       dw_out, db_out)
    if sinks:
        assert o.dw2.data_ptr() == dw_out.data_ptr() and o.db2.data_ptr() == db_out.data_ptr()
    o.dec = m[44].item()
    o.n_acc = 128 * _longest_list(ops, x.B, x.P, ops.device_cus())
    return o


def _bwd_reference(x, k, o, scale, e_from=None):
    """the fp64 reference of a launch; the dy2 scale's e is recomputed from the header's bound
    formula, and mag[44] must be 2^-e 2^-ew / 2^kd"""
    k1, k2, k3 = k
    e_hi, e_lo = R.bwd_e(*(k if e_from is None else e_from), x.b2, o.ymax, o.gmax)
    e = -(R.pow2_exp(o.dec) + o.ew + o.kd)
    assert e in (e_hi, e_lo), (e, e_hi, e_lo)
    wh = R.w_hat(x.w2, o.ew)
    p = x.p1h.double().cpu().permute(0, 3, 1, 2) / x.s
    return R.bwd_reference(x.y2h, x.codes, x.g2m, x.ginv, k1, k2, k3, x.b2, o.d, wh, p, e, scale)


def _run_backward(gpu, small_grid, P, B, kind, grids, scale=1.0, sinks=False, s=1.0):
    ops = _ops()
    x = _bwd_inputs(gpu, P, B, 31 * P + B, s)
    k = _k_set(kind, 7 * P + B, x.hd)
    res = {}
    for ncu in grids:
        small_grid(ncu)
        res[ncu] = _bwd_launch(ops, gpu, x, k, scale, sinks)
    small_grid(None)
    torch.cuda.synchronize()
    if len(grids) > 1:
        assert torch.equal(_bits(res[grids[1]].dp1h), _bits(res[grids[0]].dp1h)), "dp1h depends on the workgroup count"
    for ncu, o in res.items():
        r = R.bwd_wgrad_reference(_bwd_reference(x, k, o, scale), o.n_acc)
        if kind == "k2 k3 zero":  # (the bound is 0 there: the routed dz alone, exact zeros elsewhere)
            assert bool((r.dy2[:, 2] == 0).float().mean() > 0.7)
        tag = f"P={P} B={B} k {kind} scale={scale:.3g} s={s} {'full grid' if ncu is None else f'{ncu} workgroups'}"
        _report(tag, R.check_bwd(r, dp1h_decode(o.dp1h, o.dec, P), o.dec, o.dw2, o.db2))


BWD_SHAPES = [(8, 1, (None,)), (17, 2, (None,)), (37, 3, (None, 32)), (72, 2, (None, 32)), (10, 63, (None,))]


@pytest.mark.parametrize("kind", ["random", "k1 zero", "k2 k3 zero", "1e-7", "3e4", "1e4 apart"])
@pytest.mark.parametrize("P,B,grids", BWD_SHAPES)
def test_backward_per_element(gpu, small_grid, P, B, grids, kind):
    """fused_conv2_backward_y2 on synthesized inputs (random fp16 y2h, random argmax codes, fp16 g2m
    with per-channel power-of-two scales, free k1..k3: no BN consistency needed), dp1 / dw2 / db2 per
    element against the fp64 dy2 = k1 dz + k2 (h d + b2) + k3 and its convolutions.

    dp1 is the gradient with respect to the unscaled p = p1h / s: kc[160] = 2^-e 2^-ew carries no p1
    scale, and the layer-1 backward multiplies dp1h by mag[44] alone (l1_bwd_mfma_kernel's dec) while
    BN1's affine holds the scale -- consistent."""
    _run_backward(gpu, small_grid, P, B, kind, grids)


@pytest.mark.parametrize("P,B,grids", [(17, 2, (None,)), (37, 3, (None, 32))])
def test_backward_scale_sinks_p1_scale(gpu, small_grid, P, B, grids):
    """scale = 1/3 multiplies dw2 and db2 (not dp1), written into pre-filled dw_out / db_out sinks
    that are fully overwritten; p1 scale 2^-3: kc[161] = 2^-e / p1 scale takes it out of dw2"""
    _run_backward(gpu, small_grid, P, B, "random", grids, scale=1.0 / 3.0, sinks=True, s=2.0 ** -3)


# ------------------------------------------------------------------------------------ 5. the checks can fail
def test_bounds_reject_mutated_references(gpu):
    """One launch each of the forward, the in-launch finalize and the backward at (37, 3), checked by
    the functions above against deliberately wrong REFERENCES: each must be rejected.  (The biased
    variance moves running_var by var / (n - 1), 2.4e-4 of var at n = 4107: with a dense p1 that is
    0.6 of the worst-case bound of the sum of squares, so this launch's p1 is 5 % dense, where it is
    1.7; test_bn_one_window_image has the 4/3 of n = 4.)"""
    ops = _ops()
    P, B, s = 37, 3, 2.0 ** -3
    p1h, w2, b2, r0 = _fwd_case(gpu, P, B, s, sparse=True)
    g2, be2 = _gamma(gpu, "mixed", 5), _gamma(gpu, "mixed", 6)
    r = _with_gamma(r0, g2)
    o = _forward_both(ops, gpu, p1h, w2, b2, g2, be2, s, _bn_buffers(gpu))
    bn = (o.rm0, o.rv0, o.stats2, o.aff2, o.rm, o.rv, o.mag_y)
    x = _bwd_inputs(gpu, P, B, 77, s)
    k = _k_set("random", 78, x.hd)
    scale = 1.0 / 3.0
    ob = _bwd_launch(ops, gpu, x, k, scale)
    torch.cuda.synchronize()
    dp1 = dp1h_decode(ob.dp1h, ob.dec, P)
    bwd = lambda rr: R.check_bwd(rr, dp1, ob.dec, ob.dw2, ob.db2)
    good = _bwd_reference(x, k, ob, scale)
    # the unmutated references pass
    _report("forward", _check_forward(r, o, b2, g2, be2, "forward")[0])
    _report("finalize", _check_bn_launch(r, b2, g2, be2, bn))
    _report("backward", bwd(R.bwd_wgrad_reference(copy.copy(good), ob.n_acc)))
    rejected = {}
    # one tap dropped
    wm = w2.clone()
    wm[7, 3, 4, 4] = 0
    rm = R.fwd_reference(p1h, wm, R.pack_ew(w2), s, b2, g2)
    rejected["tap (7, 3, 4, 4) dropped"] = R.check_fwd_values(rm, o.y2h, o.d)
    # the last column shifted by one pixel
    rs = copy.copy(r)
    rs.ref = r.ref.clone()
    rs.ref[..., P - 1] = r.ref[..., P - 2]
    rejected["last column shifted"] = R.check_fwd_values(rs, o.y2h, o.d)
    rejected["n = B P (P - 1)"] = _check_bn_launch(r, b2, g2, be2, bn, n=B * P * (P - 1))
    rejected["biased running_var"] = _check_bn_launch(r, b2, g2, be2, bn, biased_running=True)
    # 0.2 % of the a2 codes changed (clear windows: an unclear one is not held to its code)
    wc = r.want.clone()
    idx = torch.nonzero(r.clear.flatten()).flatten()
    idx = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(1))[:max(1, wc.numel() // 500)]]
    wc.view(-1)[idx] = (wc.view(-1)[idx] + 1) % 4
    rejected["0.2 % of the codes"] = R.check_fwd_codes(wc, r.clear, a2_decode(o.a2))[0]
    # k3 dropped in one channel
    k3m = k[2].clone()
    k3m[int(k3m.abs().argmax())] = 0
    rejected["k3 dropped in one channel"] = bwd(
        R.bwd_wgrad_reference(_bwd_reference(x, (k[0], k[1], k3m), ob, scale, e_from=k), ob.n_acc))
    rejected["p1 scale ignored in dw2"] = bwd(R.bwd_wgrad_reference(copy.copy(good), ob.n_acc, p=good.p * s))
    rejected["scale ignored in db2"] = bwd(R.bwd_wgrad_reference(copy.copy(good), ob.n_acc, scale_b=1.0))
    for name, ratios in rejected.items():
        print(f"mutation '{name}': " + ", ".join(f"{k_} {v:.3g}" for k_, v in ratios.items()))
        assert not R.ok(ratios), f"the mutated reference '{name}' passes"


# ------------------------------------------------------------------------------------ 6. image index >= 128
def test_forward_image_index_past_127(gpu):
    """(8, 200): the tile order's image field is the word's top byte, read unsigned (f2_tile): images
    128 .. 199 meet the per-pixel bound like the rest"""
    ops = _ops()
    P, B = 8, 200
    p1h, w2, b2, r0 = _fwd_case(gpu, P, B)
    g2, be2 = _gamma(gpu, "mixed", 41), _gamma(gpu, "mixed", 42)
    r = _with_gamma(r0, g2)
    o = _forward_both(ops, gpu, p1h, w2, b2, g2, be2, 1.0, _bn_buffers(gpu))
    torch.cuda.synchronize()
    ratios, unclear = _check_forward(r, o, b2, g2, be2, "P=8 B=200")
    print(f"P=8 B=200: unclear windows {100 * unclear:.3f} %")
    _report("P=8 B=200", ratios)
    keep = torch.zeros(B, P, P, dtype=torch.bool)
    keep[128:] = True
    _report("P=8 B=200, images 128 ..", R.check_fwd_values(r, o.y2h, o.d, keep))


# ------------------------------------------------------------------------------------ 7. non-finite values
def test_forward_nan_p1_stays_local(gpu):
    """A NaN in one p1 pixel of image 1 at (37, 3).  Nothing is lost: y2h is NaN on the clipped 5 x 5
    neighbourhood in all 32 channels, ya on every window that holds such a pixel, and the partials,
    stats2, aff2 and mag[0..32) of all 32 channels.  Images 0 and 2 meet the bound at every pixel,
    image 1 at every pixel more than 3 rows or columns away.

    Stated deviation (docs/KERNELS.md "conv2 tests"): the forward's zero-weight ky = 5 K slots
    multiply real p1 rows (f2_compute), so a NaN at (r, c) may also reach (r - 3, c - 2); no other
    pixel outside the neighbourhood may be NaN."""
    ops = _ops()
    P, B = 37, 3
    p1h, w2, b2, _ = _fwd_case(gpu, P, B)
    p1h = p1h.clone()
    nr, nc = 20, 18
    p1h[1, nr, nc, 6] = float("nan")
    g2, be2 = _gamma(gpu, "mixed", 51), _gamma(gpu, "mixed", 52)
    r = R.fwd_reference(p1h, w2, R.pack_ew(w2), 1.0, b2, g2)
    r.want, r.clear = R.fwd_codes(r)
    o = _forward_both(ops, gpu, p1h, w2, b2, g2, be2, 1.0, _bn_buffers(gpu))
    torch.cuda.synchronize()
    assert r.nan.sum() == 25 and not r.nan[0].any() and not r.nan[2].any()
    got = torch.isnan(o.y2h).cpu()  # [B,P,P,32]
    assert bool(got[r.nan].all()), "a NaN of the 5 x 5 neighbourhood is lost in y2h"
    extra = got.any(-1) & ~r.nan
    allowed = torch.zeros_like(extra)
    allowed[1, nr - 3, nc - 2] = True
    assert not bool((extra & ~allowed).any()), torch.nonzero(extra & ~allowed)
    print(f"NaN at ({nr}, {nc}): y2h NaN outside the 5 x 5 neighbourhood at {torch.nonzero(extra).tolist()}, "
          f"channels {int(got[1, nr - 3, nc - 2].sum())} of 32")
    rr, cc = torch.meshgrid(torch.arange(P), torch.arange(P), indexing="ij")
    keep = torch.ones(B, P, P, dtype=torch.bool)
    keep[1] = ((rr - nr).abs() > 3) | ((cc - nc).abs() > 3)
    ratios, _ = _check_forward(r, o, b2, g2, be2, "NaN p1", keep=keep)
    ratios.pop("a2 wrong codes"), ratios.pop("a2 unclear / cap")  # (the NaN windows' codes are unused)
    _report("NaN p1, away from it", ratios)
    Q = P // 2
    ya_nan = torch.isnan(pb_to_planar(o.ya, Q)).cpu()  # [B,32,Q,Q]
    win_nan = R.windows(r.nan.unsqueeze(1).double(), Q).amax(-1)[:, 0] > 0  # [B,Q,Q]
    assert bool(ya_nan.permute(0, 2, 3, 1)[win_nan].all()), "a NaN window is lost in ya"
    for name, t in (("partial", o.partial), ("stats2", o.stats2.view(2, 32).t()), ("aff2", o.aff2.view(2, 32).t()),
                    ("ypart", o.ymax), ("mag", o.mag_y)):
        assert bool(torch.isnan(t.reshape(32, -1)).all()), f"{name}: a channel lost the NaN"


def test_backward_nan_constants_stay_in_their_channel(gpu):
    """NaN k1..k3 in one channel: that channel's dw2 and db2 rows are NaN, every other row meets its
    bound (dp1 sums over all 32 channels and is NaN throughout).  The dy2 scale's e is the other
    channels' or, the NaN reaching the bound, 0."""
    ops = _ops()
    P, B, c = 37, 3, 13
    x = _bwd_inputs(gpu, P, B, 91, 1.0)
    k = _k_set("random", 92, x.hd)
    kn = tuple(t.clone() for t in k)
    kz = tuple(t.clone() for t in k)
    for t, z in zip(kn, kz):
        t[c] = float("nan")
        z[c] = 0.0
    o = _bwd_launch(ops, gpu, x, kn, 1.0)
    torch.cuda.synchronize()
    e = -(R.pow2_exp(o.dec) + o.ew + o.kd)
    assert e in R.bwd_e(*kz, x.b2, o.ymax, o.gmax) + (0,), e
    wh = R.w_hat(x.w2, o.ew)
    p = x.p1h.double().cpu().permute(0, 3, 1, 2)
    r = R.bwd_reference(x.y2h, x.codes, x.g2m, x.ginv, *kz, x.b2, o.d, wh, p, e, 1.0)
    R.bwd_wgrad_reference(r, o.n_acc)
    skip = torch.zeros(32, dtype=torch.bool)
    skip[c] = True
    assert bool(torch.isnan(o.dw2[c]).all()) and bool(torch.isnan(o.db2[c]))
    assert bool(torch.isnan(dp1h_decode(o.dp1h, o.dec, P)).all())
    _report(f"NaN k of channel {c}, the other channels (e = {e})", R.check_bwd(r, None, o.dec, o.dw2, o.db2, skip))
