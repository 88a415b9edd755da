"""The fused plan's input gradient dL/dx (csrc/kernels/l1_dgrad.hip, ops.fused_l1_input_grad):
the kernel against fp64 with a per-element bound, the model end to end, and nothing else moved."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _l1ref as R
import test_layer1_gpu as L
from _tf32ref import rel, tf32_convs
from test_fused_gpu import _ops, dp1h_encode
from test_head_wide_gpu import _Ref

pytestmark = pytest.mark.gpu

U22, U24 = 2.0 ** -22, 2.0 ** -24
RANGES = [(-2, 0), (-2, 1), (-2, 2), (-1, 2), (0, 2)]  # valid centred taps of the 5 border classes of an axis


def _classes(H):
    c = torch.full((H,), 2, dtype=torch.long)
    c[0], c[1], c[H - 2], c[H - 1] = 0, 1, 3, 4
    return c


def _reference(c, idx1, dp1, g1, stats):
    """fp64 dx of the op's own inputs and M, the sum of the absolute values of every term of dx[q]:
    dz routed by idx1, dy = A dz + B (y - b1) + C with fp64 sums, dx = conv_transpose2d(dy, w1)."""
    H, n = c.H, c.B * c.H * c.H
    mean, invstd, g = stats[:16].double().cpu(), stats[16:].double().cpu(), g1.double()
    v = lambda t: t.view(1, 16, 1, 1)
    dz = R.dense_dz(idx1, dp1)
    dgamma = (dz * (c.yc + v(c.b64) - v(mean))).sum((0, 2, 3)) * invstd
    A, Bc = g * invstd, -g * invstd ** 2 * dgamma / n
    C = -A * dz.sum((0, 2, 3)) / n + Bc * (c.b64 - mean)
    dx = F.conv_transpose2d(v(A) * dz + v(Bc) * c.yc + v(C), c.w64, padding=2)
    Ms = F.conv_transpose2d(dz.abs(), (v(A).view(16, 1, 1, 1) * c.w64).abs(), padding=2)
    # |K2| * |x| and |K0| per border class, selected per pixel
    w = c.w64.view(16, 5, 5)
    Md = torch.zeros_like(dx)
    rc, cc = _classes(H).view(H, 1).expand(H, H), _classes(H).view(1, H).expand(H, H)
    for i, (rl, rh) in enumerate(RANGES):
        for j, (cl, ch) in enumerate(RANGES):
            wm = torch.zeros_like(w)
            wm[:, rl + 2:rh + 3, cl + 2:ch + 3] = w[:, rl + 2:rh + 3, cl + 2:ch + 3]
            k2 = (Bc.view(16, 1, 1) * F.conv2d(w.unsqueeze(0), wm.unsqueeze(1), padding=4, groups=16)[0]).sum(0)
            m = F.conv2d(c.x64.abs(), k2.abs().view(1, 1, 9, 9), padding=4) + (C * wm.sum((1, 2))).sum().abs()
            Md = torch.where(((rc == i) & (cc == j)).view(1, 1, H, H), m, Md)
    return dx, Ms, Ms + Md


KERNEL_CASES = [(16, 1, "base"), (20, 3, "base"), (36, 2, "base"), (132, 3, "base"), (36, 2, "dp1_zero_channel"),
                (36, 2, "gamma_zero")]


@pytest.mark.parametrize("H,B,variant", KERNEL_CASES)
def test_kernel_against_fp64(gpu, H, B, variant):
    """fused_l1_backward, then fused_l1_input_grad, on an fp32 image, a random fp16 dp1h at a decode
    factor of 2^-9, mixed-sign gamma1 and the idx1 of the project's own layer-1 forward.

    Bound per element: |err[q]| <= 2^-22 Ms[q] + 128 * 2^-24 M[q].  Ms is the sparse term's magnitude
    sum |A_c w_c[t] dz|, M adds sum |K2| |x| and |K0|.  Counting roundings: a sparse product is dz (fp16,
    exact as stored) times A_c w_c[t] carried as an fp16 hi + lo pair, one rounding of 2^-22 (k = 1, u =
    2^-22); the rest is fp32: 16 channels summed in the MFMA and 25 taps in the shift-add (41), a K2 tap
    stored in fp32 and 81 FMAs (82), the two decode factors (powers of two, exact) and the final two adds
    with K0 (3): 126 <= 128 roundings of 2^-24 of M.  The fp32 statistics are the op's inputs and enter
    the reference as given; the layer-1 backward's sums are held to fp64 sums by this bound as well."""
    P = H // 2
    c = L._case(gpu, H, B, False)
    gen = torch.Generator().manual_seed(77 * H + B)
    g1, be1 = L._gamma("mixed", H + B)
    if variant == "gamma_zero":
        g1[5] = 0.0
    dp1 = torch.randn(B, P, P, 16, generator=gen)
    if variant == "dp1_zero_channel":
        dp1[..., 3] = 0.0
    dp1h, dec, dp1 = dp1h_encode(dp1.to(gpu), 2.0 ** -9)
    (p1, idx1, stats, gram, _), _, _, _ = L._forward(gpu, c, g1, be1)
    ops = _ops()
    bsum = torch.empty(16 * 27, dtype=torch.float64, device=gpu)
    ops.fused_l1_backward(dp1h, dec, c.xin, p1, idx1, c.w1, c.b1, g1.to(gpu), stats, gram, 1.0, None, None, None, None,
                          bsum)
    dx = ops.fused_l1_input_grad(dp1h, dec, c.xin, idx1, c.w1, c.b1, g1.to(gpu), stats, bsum)
    assert dx.shape == c.xin.shape and dx.dtype == torch.float32
    ref, Ms, M = _reference(c, idx1.cpu(), dp1.double().cpu(), g1, stats)
    got = dx.double().cpu()
    assert torch.isfinite(got).all()
    worst = L._ratio((got - ref).abs(), U22 * Ms + 128 * U24 * M).max().item()
    print(f"H={H} B={B} {variant}: dx err / bound {worst:.3f}  (max |dx| {ref.abs().max():.3e})")
    assert worst <= 1.0, f"H={H} B={B} {variant}: dx err / bound {worst:.3f}"


def _model_step(gpu, x, y, needs_grad):
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    torch.manual_seed(0)
    model = ConvNet(image_shape=(64, 64), mode="fused")
    with torch.no_grad():
        model.layer1[1].weight[::4].neg_()  # some negative BN1 and BN2 gammas: min-pooled windows
        model.layer2[1].weight[::3].neg_()
    cpu = copy.deepcopy(model)
    model = model.to(gpu)
    x = x.clone().requires_grad_(needs_grad)
    logits = model(x)
    loss = CrossEntropyLoss()(logits, y)
    loss.backward()
    return model, cpu, x, logits, loss


def test_model_input_gradient(gpu):
    """x.grad of the fused ConvNet within max(1e-3, 1.5 x the TF32-operand model's error) relative L2 of
    the fp64 model's, and torch.autograd.grad gives the same values."""
    from torch_distributed_sandbox_amd.models import fc_in_features
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    torch.manual_seed(1)
    x0, y = torch.rand(3, 1, 64, 64, device=gpu), torch.randint(0, 10, (3,), device=gpu)
    model, cpu, x, _, _ = _model_step(gpu, x0, y, True)
    assert x.grad is not None and x.grad.shape == x.shape
    ref = _Ref(fc_in_features((64, 64)), 10).double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in cpu.state_dict().items()})
    grads = []
    for m in (ref, tf32_convs(copy.deepcopy(ref))):
        x64 = x0.double().cpu().requires_grad_()
        F.cross_entropy(m(x64), y.cpu()).backward()
        grads.append(x64.grad)
    e, et = rel(x.grad.cpu(), grads[0]), rel(grads[1], grads[0])
    print(f"x.grad rel L2 err {e:.3e}  (TF32 convs: {et:.3e})")
    assert e <= max(1e-3, 1.5 * et), f"x.grad rel L2 err {e:.3e} (TF32 convs: {et:.3e})"
    (again,) = torch.autograd.grad(CrossEntropyLoss()(model(x), y), x)
    assert torch.equal(again, x.grad)


def test_nothing_else_moved(gpu):
    """The same step with and without x.requires_grad: logits, loss, every parameter gradient and the BN
    buffers bit-identical; without it the backward hands x no gradient."""
    torch.manual_seed(2)
    x0, y = torch.rand(3, 1, 64, 64, device=gpu), torch.randint(0, 10, (3,), device=gpu)
    ma, _, xa, la, lossa = _model_step(gpu, x0, y, True)
    mb, _, xb, lb, lossb = _model_step(gpu, x0, y, False)
    assert xa.grad is not None and xb.grad is None
    assert torch.equal(la, lb) and torch.equal(lossa, lossb)
    for (n, p), q in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, p), q in zip(ma.named_buffers(), mb.buffers()):
        assert torch.equal(p, q), n
