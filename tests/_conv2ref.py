"""fp64 references and arithmetic error bounds of the conv2 kernels (tests/test_conv2_gpu.py).

Everything here runs on the CPU in fp64 from the ops' inputs (csrc/kernels/conv2_common.h,
conv2_pack.h, docs/KERNELS.md "conv2 tests").  Layouts: activations and bounds are NCHW
[B, C, P, P]; a window axis of 4 is in the pooling scan order q = 2 * dr + dc.  A checker returns
{quantity: worst err / bound}; ok() holds every ratio to <= 1, and a NaN ratio (a value that is NaN
where the reference is finite, or the reverse) fails it."""
import math
import types

import torch
import torch.nn.functional as F

U, U11 = 2.0 ** -24, 2.0 ** -11
K101 = 1.01  # second-order terms of every worst-case accumulation bound
N_FWD = 416  # K slots of a forward accumulator: 16 ci x 26 (25 taps + the zero ky = 5 slot)
N_DGRAD = 800  # 32 co x 25 taps


def ok(ratios):
    return all(r <= 1.0 for r in ratios.values())  # (NaN <= 1 is False)


def ratio(err, bound):
    """worst err / bound; inf where the bound is 0 and the error is not, NaN on a NaN error"""
    err, bound = err.double().flatten(), bound.double().flatten()
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float("nan") if bool(torch.isnan(r).any()) else r.max().item()


def windows(t, Q):
    """[B, C, P, P] -> [B, C, Q, Q, 4], scan order, the pooled 2Q x 2Q part"""
    B, C = t.shape[:2]
    return t[:, :, :2 * Q, :2 * Q].reshape(B, C, Q, 2, Q, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Q, Q, 4)


# ------------------------------------------------------------------------------------ conv2_pack
def pow2_exp(x):
    """k of a float that must be exactly 2^k"""
    m, k = math.frexp(x)
    assert m == 0.5, f"{x!r} is no power of two"
    return k - 1


def pack_ew(w):
    """ew of conv2_pack (max |w| 2^ew in [2^14, 2^15)); the max of fp32 values is exact"""
    m = w.detach().abs().max().item()
    if not (m > 0 and math.isfinite(m)):
        return 0
    return min(100, max(-100, 15 - math.frexp(m)[1]))


def packed_weights(w, ew):
    """fp16(w 2^ew) as the packing rounds it (fp32 product exact: a power of two; one rounding to
    nearest even) [32,16,5,5] fp16, CPU"""
    return (w.detach().float().cpu() * 2.0 ** ew).half()


def w_hat(w, ew):
    """the weights the MFMAs multiply by, fp64: fp16(w 2^ew) 2^-ew"""
    return packed_weights(w, ew).double() * 2.0 ** -ew


def pack_d(w, s):
    """the y2h decode d = 2^-ew / s / 2^k of the documented choices: 1.01 L 2^ew 2^k in (1/2, 1]"""
    ew = pack_ew(w)
    L = K101 * w.detach().double().abs().sum((1, 2, 3)).max().item() * 2.0 ** ew
    k = -math.frexp(L)[1] if L > 0 and math.isfinite(L) else 0
    return 2.0 ** -ew / s / 2.0 ** k


def unpack_wp(wp):
    """forward pack wp[s 13][nt 2][g 4][co 16][j 8] (conv2_pack.h) -> ([32,16,5,5] fp16, the ky = 5
    slots [32,16] fp16): s < 10: ky = s >> 1, kx = 2 (s & 1) + (g >> 1); s = 10 + kp: ky = 2 kp +
    (g >> 1), kx = 4; ci = 8 (g & 1) + j, co = 16 nt + co16"""
    h = wp.cpu().view(torch.float16)
    e = torch.arange(13 * 2 * 4 * 16 * 8)
    j, co_in, g, nt, s = e & 7, (e >> 3) & 15, (e >> 7) & 3, (e >> 9) & 1, e >> 10
    ky = torch.where(s < 10, s >> 1, 2 * (s - 10) + (g >> 1))
    kx = torch.where(s < 10, 2 * (s & 1) + (g >> 1), torch.full_like(s, 4))
    ci, co = 8 * (g & 1) + j, nt * 16 + co_in
    full = torch.full((32, 16, 6, 5), float("nan"), dtype=torch.float16)
    full[co, ci, ky, kx] = h
    assert not torch.isnan(full[:, :, :5]).any()  # (every tap has a slot; the inputs are finite)
    return full[:, :, :5].contiguous(), full[:, :, 5, 4].contiguous()


def unpack_wd(wd):
    """dgrad pack wd[s 25][g 4][ci 16][j 8]: co = 8 g + j, the flipped tap 24 - s -> [32,16,5,5] fp16"""
    h = wd.cpu().view(torch.float16)
    f = torch.arange(25 * 4 * 16 * 8)
    j, ci, g, s = f & 7, (f >> 3) & 15, (f >> 7) & 3, f >> 9
    out = torch.full((32, 16, 25), float("nan"), dtype=torch.float16)
    out[8 * g + j, ci, 24 - s] = h
    return out.view(32, 16, 5, 5)


def check_pack_scales(m40, m41, m42, m43, w, s, slack=1e-5):
    """mag[40..43] of conv2_pack against the documented choices; -> (ew, k, kd).  L and Ld in fp64;
    `slack`: the kernel's fp32 sums."""
    ew = pack_ew(w)
    assert m40 == 2.0 ** -ew, (m40, ew)
    assert m41 == 1.0 / s, (m41, s)
    k, kd = pow2_exp(m42), pow2_exp(m43)
    wa = w.detach().double().cpu().abs()
    L, Ld = wa.sum((1, 2, 3)).max().item(), wa.sum((0, 2, 3)).max().item()
    if not (L > 0 and math.isfinite(L)):
        assert k == 0 and kd == 0, (k, kd)  # the scales fall back to 1
        return ew, k, kd
    y = K101 * L * 2.0 ** ew * 2.0 ** k
    assert 0.5 * (1 - slack) < y <= 1 + slack, f"2^k = 2^{k}: 1.01 L 2^ew 2^k = {y}"
    yd = K101 * 2.0 ** 15 * Ld * 2.0 ** ew * 2.0 ** kd / 65504.0
    assert 0.5 * (1 - slack) < yd <= 1 + slack, f"2^kd = 2^{kd}: 1.01 2^15 Ld 2^ew 2^kd / 65504 = {yd}"
    return ew, k, kd


# ------------------------------------------------------------------------------------ forward
def fwd_reference(p1h, w, ew, s, b2, g2):
    """The fp64 convolution of the kernel's exact operands: w^ = fp16(w 2^ew) 2^-ew, p = p1h / s.
    ref = w^ * p (bias-free, y2 - b2), A = |w^| * |p|, dacc = 1.01 416 u A (416 fp32 additions in any
    order).  A non-finite p1 is taken as 0 and its clipped 5 x 5 neighbourhood marked in `nan`."""
    r = types.SimpleNamespace()
    p = p1h.detach().double().cpu().permute(0, 3, 1, 2) / s
    bad = ~torch.isfinite(p)
    p = torch.where(bad, torch.zeros_like(p), p)
    r.nan = F.max_pool2d(bad.any(1, keepdim=True).double(), 5, 1, 2)[:, 0] > 0  # [B,P,P]
    wh = w_hat(w, ew)
    r.p, r.wh = p, wh
    r.ref = F.conv2d(p, wh, None, padding=2)
    r.A = F.conv2d(p.abs(), wh.abs(), None, padding=2)
    r.dacc = K101 * N_FWD * U * r.A
    r.b2, r.g2 = b2.detach().double().cpu(), g2.detach().double().cpu()
    r.B, r.P = p.shape[0], p.shape[2]
    r.n = r.B * r.P * r.P
    return r


def fwd_bound(r, d):
    """|y2h d - ref| per pixel: the accumulation, one rounding to fp16, half the smallest fp16
    subnormal step at the y2h scale"""
    return r.dacc + U11 * r.ref.abs() + 2.0 ** -25 * d


def check_fwd_values(r, y2h, d, keep=None):
    """y2h [B,P,P,32] fp16 against ref at every pixel (keep [B,P,P]: the pixels held to the bound)"""
    v = y2h.detach().double().cpu().permute(0, 3, 1, 2) * d
    err, bound = (v - r.ref).abs(), fwd_bound(r, d)
    if keep is not None:
        m = keep.unsqueeze(1).expand_as(err)
        err, bound = err[m], bound[m]
    return {"y2h": ratio(err, bound)}


def fwd_codes(r):
    """-> (the reference's first extreme per window [B,32,Q,Q], clear [B,32,Q,Q]: the fp64 top-two
    gap exceeds the two pixels' accumulation bounds; gamma2 == 0: code 0, always clear)"""
    Q = r.P // 2
    neg, zero = (r.g2 < 0).view(1, 32, 1, 1, 1), (r.g2 == 0).view(1, 32, 1, 1)
    w = windows(r.ref, Q)
    key = torch.where(neg, -w, w)
    top, idx = key.topk(2, -1)
    dw = windows(r.dacc, Q).gather(-1, idx)
    clear = (top[..., 0] - top[..., 1]) > (dw[..., 0] + dw[..., 1])
    first = (key == key.max(-1, keepdim=True).values).int().argmax(-1)
    return torch.where(zero, torch.zeros_like(first), first), clear | zero


def check_fwd_codes(want, clear, codes, cap=0.005):
    """codes [B,Q,Q,32] (a2 decoded) name `want` on every clear window; unclear <= cap"""
    got = codes.cpu().permute(0, 3, 1, 2)
    unclear = 1.0 - clear.double().mean().item() if clear.numel() else 0.0
    bad = int(((got != want) & clear).sum())
    return {"a2 wrong codes": float("inf") if bad else 0.0, "a2 unclear / cap": unclear / cap}, unclear


def sums_reference(r, n=None):
    """S, Q = sums of (y2 - b2) and its square per channel, their bounds ds, dq (the pixels' dacc
    through the sums + the kernel's fp32 tile sums of <= 16 values per lane: 16 u)"""
    yc, d = r.ref, r.dacc
    x = types.SimpleNamespace(n=r.n if n is None else n)
    x.S, x.Q = yc.sum((0, 2, 3)), (yc * yc).sum((0, 2, 3))
    x.ds = d.sum((0, 2, 3)) + 16 * U * yc.abs().sum((0, 2, 3))
    x.dq = (2 * yc.abs() * d + d * d).sum((0, 2, 3)) + 16 * U * x.Q
    return x


def check_partial(x, s):
    """s [32,2]: the workgroups' partials summed"""
    s = s.double().cpu()
    return {"partial sum": ratio((s[:, 0] - x.S).abs(), x.ds), "partial sumsq": ratio((s[:, 1] - x.Q).abs(), x.dq)}


def check_ymax(r, ymax):
    """max |y2 - b2| per channel from the fp32 accumulators: at least the reference's largest pixel
    less its bound, at most the largest |ref| + dacc of any pixel"""
    y = ymax.double().cpu()
    a = r.ref.abs().flatten(2).permute(1, 0, 2).reshape(32, -1)
    dd = r.dacc.flatten(2).permute(1, 0, 2).reshape(32, -1)
    i = a.argmax(1, keepdim=True)
    lo = (a.gather(1, i) - dd.gather(1, i)).squeeze(1)
    hi = (a + dd).max(1).values
    mid, half = (hi + lo) / 2, (hi - lo) / 2
    return {"ymax": ratio((y - mid).abs(), half)}


# ------------------------------------------------------------------------------------ BN2 finalize
def bn_reference(x, b2, g2, be2, rm0, rv0, momentum, eps, biased_running=False):
    """BN2's training outputs per channel in fp64 from the sums x (sums_reference), with bounds
    built from ds, dq.  momentum, eps: the fp32 values the op is handed."""
    n = float(x.n)
    mom, eps = float(torch.tensor(momentum, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    o = types.SimpleNamespace()
    b2, g2, be2 = (t.detach().double().cpu() for t in (b2, g2, be2))
    m0 = x.S / n
    var = (x.Q / n - m0 * m0).clamp_min(0)
    o.mean = m0 + b2
    o.dmean = x.ds / n + U * o.mean.abs()
    dvar = (x.dq + 2 * m0.abs() * x.ds) / n
    o.invstd = (var + eps).rsqrt()
    o.dinvstd = o.invstd * (0.5 * dvar / (var + eps) + 2 * U)
    o.a = g2 * o.invstd
    o.da = g2.abs() * o.dinvstd + 2 * U * o.a.abs()
    o.b = be2 - o.mean * o.a
    o.db = o.a.abs() * o.dmean + (o.mean * g2).abs() * o.dinvstd + 2 * U * (be2.abs() + (o.mean * o.a).abs())
    unb = var if biased_running or n <= 1 else var * n / (n - 1)
    o.rm = (1 - mom) * rm0.double().cpu() + mom * o.mean
    o.drm = mom * x.ds / n + U * o.rm.abs()
    o.rv = (1 - mom) * rv0.double().cpu() + mom * unb
    o.drv = mom * dvar * (1.0 if n <= 1 else n / (n - 1)) + U * o.rv.abs()
    o.zero = g2 == 0
    o.be2 = be2
    return o


def check_bn(o, stats2, aff2, rm, rv):
    st, af = stats2.double().cpu(), aff2.double().cpu()
    out = {
        "mean": ratio((st[:32] - o.mean).abs(), o.dmean),
        "invstd": ratio((st[32:] - o.invstd).abs(), o.dinvstd),
        "aff a": ratio((af[:32] - o.a).abs(), o.da),
        "aff b": ratio((af[32:] - o.b).abs(), o.db),
        "running_mean": ratio((rm.double().cpu() - o.rm).abs(), o.drm),
        "running_var": ratio((rv.double().cpu() - o.rv).abs(), o.drv),
    }
    if bool(o.zero.any()):  # gamma2 == 0: a = 0 and b = beta2 exactly
        exact = bool((af[:32][o.zero] == 0).all()) and bool((af[32:][o.zero] == o.be2[o.zero]).all())
        out["aff at gamma2 = 0"] = 0.0 if exact else float("inf")
    return out


# ------------------------------------------------------------------------------------ backward
def bwd_e(k1, k2, k3, b2, ymax, gmax):
    """the dy2 scale's exponent (conv2_bwd.hip): the largest channel bound |k1| max|g2m| + |k2|
    (max|y2 - b2| + |b2|) + |k3| put in [2^14, 2^15); -> the e of the bound 1e-6 below and above its
    fp64 value (the kernel forms it in fp32), equal unless it sits at a power of two"""
    k1, k2, k3, b2, ymax = (t.detach().double().cpu() for t in (k1, k2, k3, b2, ymax))
    bound = (k1.abs() * gmax + k2.abs() * (ymax + b2.abs()) + k3.abs()).max().item()
    if not (bound > 0 and math.isfinite(bound)):
        return 0, 0
    f = lambda v: min(60, max(-60, 15 - math.frexp(v)[1]))
    return f(bound * (1 + 1e-6)), f(bound * (1 - 1e-6))


def bwd_reference(y2h, codes, g2m, ginv, k1, k2, k3, b2, d, wh, p, e, scale):
    """dy2 = k1 dz + k2 (h d + b2) + k3 in fp64 (dz the pooled gradient g2m ginv at the window's code,
    0 on an unpooled last row / column) and the conv2 gradients of it: dp1 = convT(dy2, w^) (the
    gradient with respect to p = p1h / s), dw2 = scale sum dy2 (x) p, db2 = scale sum dy2.
    ddy: one 2^-11 rounding of dy2 2^e, three fp32 roundings of its terms (4 u M), half a subnormal."""
    r = types.SimpleNamespace()
    v = lambda t: t.detach().double().cpu().view(1, 32, 1, 1)
    h = y2h.detach().double().cpu().permute(0, 3, 1, 2)
    B, _, P, _ = h.shape
    Q = P // 2
    g = g2m.detach().double().cpu() * v(ginv)
    win = torch.zeros(B, 32, Q, Q, 4, dtype=torch.float64)
    win.scatter_(-1, codes.cpu().permute(0, 3, 1, 2).long().unsqueeze(-1), g.unsqueeze(-1))
    dz = torch.zeros(B, 32, P, P, dtype=torch.float64)
    dz[:, :, :2 * Q, :2 * Q] = win.view(B, 32, Q, Q, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, 2 * Q, 2 * Q)
    t1, t2, t3, t4 = v(k1) * dz, v(k2) * d * h, v(k2) * v(b2), v(k3)
    r.dy2 = t1 + t2 + t3 + t4
    M = t1.abs() + t2.abs() + (t3.abs() + t4.abs())
    r.ddy = U11 * r.dy2.abs() + 4 * U * M + 2.0 ** -25 * 2.0 ** -e
    r.wh, r.p, r.scale, r.e = wh, p, scale, e
    r.dp1 = F.conv_transpose2d(r.dy2, wh, None, padding=2)
    r.dp1_acc = F.conv_transpose2d(r.ddy, wh.abs(), None, padding=2) + K101 * N_DGRAD * U * F.conv_transpose2d(
        r.dy2.abs(), wh.abs(), None, padding=2)
    return r


def _wgrad(dy, p):
    """sum over images and pixels of dy[co] p[ci] at tap (ky, kx): [32,16,5,5]"""
    B = dy.shape[0]
    out = torch.zeros(32, 400, dtype=torch.float64)
    for b in range(B):  # (one image's patches at a time: 400 x P^2 doubles)
        out += dy[b].flatten(1) @ F.unfold(p[b:b + 1], 5, padding=2)[0].t()
    return out.view(32, 16, 5, 5)


def bwd_wgrad_reference(r, n_acc, p=None, scale_w=None, scale_b=None):
    """dw2 / db2 and their bounds; n_acc: the pixels one workgroup's fp32 accumulator sees"""
    p = r.p if p is None else p
    sw = r.scale if scale_w is None else scale_w
    sb = r.scale if scale_b is None else scale_b
    r.dw = sw * _wgrad(r.dy2, p)
    r.ddw = abs(sw) * (_wgrad(r.ddy, p.abs()) + K101 * n_acc * U * _wgrad(r.dy2.abs(), p.abs())) + U * r.dw.abs()
    r.db = sb * r.dy2.sum((0, 2, 3))
    r.ddb = abs(sb) * (r.ddy.sum((0, 2, 3)) + K101 * n_acc * U * r.dy2.abs().sum((0, 2, 3))) + U * r.db.abs()
    return r


def check_bwd(r, dp1, dec, dw2, db2, skip=None):
    """dp1 [B,P,P,16] decoded with dec = mag[44]; skip [32] bool: channels whose dw2 / db2 rows are
    not held to the bounds (checked by the caller)"""
    keepc = torch.ones(32, dtype=torch.bool) if skip is None else ~skip
    out = {}
    if skip is None:
        got = dp1.detach().double().cpu().permute(0, 3, 1, 2)
        bound = r.dp1_acc + U11 * r.dp1.abs() + 2.0 ** -25 * dec
        out["dp1"] = ratio((got - r.dp1).abs(), bound)
    out["dw2"] = ratio((dw2.double().cpu() - r.dw).abs()[keepc], r.ddw[keepc])
    out["db2"] = ratio((db2.double().cpu() - r.db).abs()[keepc], r.ddb[keepc])
    return out
