"""fp64 references and arithmetic error bounds of the layer-1 kernels (tests/test_layer1_gpu.py).

Everything here runs on the CPU in fp64 from the ops' inputs.  Layouts: activations and bounds are
[B, 16, H, H] (NCHW) or pooled [B, 16, P, P]; a window axis of 4 is in the pooling scan order
q = 2 * dr + dc, the order torch's max-pool (and the kernels) break ties in."""
import torch
import torch.nn.functional as F

U11, U15, U22 = 2.0 ** -11, 2.0 ** -15, 2.0 ** -22

# BN1 scale signs with a negative channel in every lane group of four (channel 4g + r), the two
# waves' patterns different, and group 2 all negative
SIGNS = torch.tensor([-1.0, 1, 1, 1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, 1], dtype=torch.float64)


def windows(t):
    """[B, C, H, W] -> [B, C, H/2, W/2, 4], scan order"""
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def conv_parts(x64, w1):
    """conv(x, w1) without the bias and |w1| * |x| (the products' magnitude), [B, 16, H, H].  A
    non-finite x is taken as 0 in the magnitude (the bound is used only where x is finite)."""
    w = w1.detach().double().cpu()
    xa = torch.where(torch.isfinite(x64), x64, torch.zeros_like(x64)).abs()
    return F.conv2d(x64, w, None, padding=2), F.conv2d(xa, w.abs(), None, padding=2)


def dz_bound(a, b, b1, yc, ya, rounded_affine=False):
    """Per-pixel bound of the kernel's z = a (conv + b1) + b against fp64, a, b, b1 [16] fp64:

      |a| 2^-15 (|w1| * |x|)              the 25 products (each <= 2^-16 relative, docs/KERNELS.md
                                          "Precision") and their fp32 accumulation
      2^-22 (|a conv| + |a b1 + b|)       the epilogue's two fp32 FMAs (a b1 + b, then a acc + that)
      2^-22 (|a (conv + b1)| + |b|)       rounded_affine: a and b themselves rounded to fp32"""
    v = lambda t: t.view(1, 16, 1, 1)
    d = v(a).abs() * U15 * ya + U22 * ((v(a) * yc).abs() + v((a * b1 + b).abs()))
    if rounded_affine:
        d = d + U22 * ((v(a) * (yc + v(b1))).abs() + v(b.abs()))
    return d


def p1_reference(a, b, b1, yc):
    """z [B,16,H,H] and relu -> max-pool of it with torch's own NaN rule [B,16,P,P]"""
    v = lambda t: t.view(1, 16, 1, 1)
    z = v(a) * (yc + v(b1)) + v(b)
    return z, F.max_pool2d(F.relu(z), 2, 2)


def p1_bound(dz, ref):
    """|p1 - ref| <= the largest z bound of the window (max and ReLU are 1-Lipschitz) + the one
    rounding to fp16 (2^-11 relative)"""
    return F.max_pool2d(dz, 2, 2) + U11 * ref.abs()


def first_max(zw):
    """index of the first maximum along the last (window) axis: torch's max-pool choice"""
    return (zw == zw.max(-1, keepdim=True).values).int().argmax(-1)


def bf16(t):
    """round to nearest even to bf16, kept in fp64 (t holds fp32 values)"""
    b = t.float().view(torch.int32)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & ~0xFFFF
    return b.view(torch.float32).double()


def bf16_split(t):
    """csrc/kernels/bf16x3.h: hi = bf16(v), lo = bf16(v - hi)"""
    hi = bf16(t)
    return hi, bf16(t - hi)


def dense_dz(idx1, dp1):
    """The dense full-resolution dz1 [B,16,H,H] of an argmax plane idx1 [B,P,P,16] (uint8: bits
    0-1 the window slot, bit 2 the ReLU mask) and the pooled gradient dp1 [B,P,P,16] fp64."""
    B, P = idx1.shape[:2]
    code = idx1.long()
    val = torch.where((code & 4) != 0, dp1, torch.zeros_like(dp1))
    w = torch.zeros(B, P, P, 16, 4, dtype=torch.float64)
    w.scatter_(-1, (code & 3).unsqueeze(-1), val.unsqueeze(-1))
    return w.view(B, P, P, 16, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, 16, 2 * P, 2 * P)


def patch_sums(dz, x64):
    """T[c][j] = sum dz1[c] xpatch_j [16,25] and sum dz1 [16]"""
    pat = F.unfold(x64, 5, padding=2)  # [B, 25, H*W]
    return torch.einsum("bcp,bjp->cj", dz.flatten(2), pat), dz.sum((0, 2, 3))


def gram(x64):
    """G[k][j] = sum xpatch_k xpatch_j [25,25] and S[j] = sum xpatch_j [25] of the zero-padded patches"""
    pat = F.unfold(x64, 5, padding=2)
    return torch.einsum("bkp,bjp->kj", pat, pat), pat.sum((0, 2))


def bn_stats(y, eps):
    """batch mean and 1 / sqrt(biased variance + eps) per channel of y [B,16,H,H]"""
    mean = y.mean((0, 2, 3))
    return mean, (y.var((0, 2, 3), unbiased=False) + eps).rsqrt()


def l1_closed_form(T, sdz, G, S, w, b1, g, mean, invstd, n):
    """The gradients of batch_norm(conv2d(x, w, b1)) (batch statistics) for an output gradient dz1
    that enters only through T = sum dz1 (x) xpatch and sdz = sum dz1 (docs/KERNELS.md "Layer 1: one
    conv pass"): y is linear in the patches, so sum dz1 y and sum y xpatch are contractions of T, G
    and S.  w [16,25].  Returns dw1 [16,25], dgamma1, dbeta1; db1 is identically 0."""
    sdzy = b1 * sdz + (w * T).sum(1)
    sdxh = sdzy - mean * sdz  # sum dz1 (y - mean)
    a1 = g * invstd
    a2 = -g * invstd ** 3 * sdxh / n
    a3 = -g * invstd * sdz / n - a2 * mean
    h = w @ G + b1.view(16, 1) * S.view(1, 25)  # sum y xpatch_j
    return a1.view(16, 1) * T + a2.view(16, 1) * h + a3.view(16, 1) * S.view(1, 25), invstd * sdxh, sdz
