"""The affine-sampled input op (csrc/kernels/ups_affine.hip): levels against the contract's formula
in fp64 per element, the identity map against the plain upsample byte for byte, the moments exact
on the levels written, and the fused plan and the loader on augmented batches."""
import math

import pytest
import torch
import torch.nn.functional as F

from torch_distributed_sandbox_amd.ops import functional as TF

SHAPES = [(2, 28, 100, 252), (1, 28, 256, 256), (2, 20, 97, 64)]
# fp32 u, v (3 roundings each at |coordinate| < 64) move a bilinear surface of levels by < 3e-3, the
# fp32 lerps by ~1e-4: 2^-7 covers both, on top of the half level of the rounding
BOUND = 0.5 + 2.0 ** -7


def _mat(hw, H, W, deg=0.0, scale=1.0, tx=0.0, ty=0.0):
    """Output pixel centre -> source index for: rotate by deg and scale about the centre, then shift."""
    c, s, k = math.cos(math.radians(deg)) / scale, math.sin(math.radians(deg)) / scale, hw / 2
    return [c * hw / W, s * hw / H, k - c * (k + tx) - s * (k + ty) - 0.5,
            -s * hw / W, c * hw / H, k + s * (k + tx) - c * (k + ty) - 0.5]


def _case(B, hw, H, W, device, extra=()):
    """Sources and matrices: image 0 turned 20 degrees at scale 0.8 and pushed partly out of frame,
    the others shifted out of frame; then the rows of ``extra``."""
    g = torch.Generator().manual_seed(H + W)
    rows = [_mat(hw, H, W, 20.0, 0.8, 0.35 * hw, -0.2 * hw)] + [_mat(hw, H, W, tx=-0.4 * hw, ty=0.3 * hw)] * (B - 1)
    src = torch.randint(0, 256, (B + len(extra), hw, hw), dtype=torch.uint8, generator=g)
    return src.to(device), torch.tensor(rows + list(extra), dtype=torch.float32, device=device)


def _ref_fp64(src, mats, H, W):
    """The contract in fp64 from the fp32 matrices: floor, zero-padded gather, lerps."""
    (B, h, w), dev = src.shape, src.device
    m = mats.double()[:, :, None, None]
    X = torch.arange(W, dtype=torch.float64, device=dev) + 0.5
    Y = (torch.arange(H, dtype=torch.float64, device=dev) + 0.5)[:, None]
    u = (m[:, 0] * X + m[:, 1] * Y + m[:, 2]).clamp(-1, w)
    v = (m[:, 3] * X + m[:, 4] * Y + m[:, 5]).clamp(-1, h)
    i0, j0 = u.floor().long(), v.floor().long()
    ax, ay = u - i0, v - j0
    s, bi = F.pad(src.double(), (2, 2, 2, 2)), torch.arange(B, device=dev)[:, None, None]
    top = ax * s[bi, j0 + 2, i0 + 3] + (1 - ax) * s[bi, j0 + 2, i0 + 2]
    bot = ax * s[bi, j0 + 3, i0 + 3] + (1 - ax) * s[bi, j0 + 3, i0 + 2]
    return (ay * bot + (1 - ay) * top)[:, None]


def _lag_sums(x):
    """The 42 sums of the partials' columns, by torch in fp64 on the levels (exact at these sizes)."""
    xd, (H, W), out = x.double()[:, 0], x.shape[2:], []
    for dy in range(5):
        for dx in range(-4, 5) if dy else range(5):
            out.append((xd[:, :H - dy, max(0, -dx):W - max(0, dx)] * xd[:, dy:, max(0, dx):W - max(0, -dx)]).sum())
    return torch.stack(out + [xd.sum()])


def _interior(hw, H, W, device):
    """Pixels whose unclamped plain-upsample source coordinates lie in [0, hw - 1]^2."""
    def ok(n):
        f = (torch.arange(n, dtype=torch.float64, device=device) + 0.5) * float(torch.tensor(hw / n).float()) - 0.5
        return (f >= 0) & (f <= hw - 1)
    return ok(H)[:, None] & ok(W)


@pytest.mark.gpu
@pytest.mark.parametrize("B,hw,H,W", SHAPES)
def test_levels_against_fp64(gpu, B, hw, H, W):
    src, mats = _case(B, hw, H, W, gpu)
    x, _ = TF.upsample_levels_moments(src, H, W, affine=mats)
    err = (x.double() - _ref_fp64(src, mats, H, W)).abs().max().item()
    print(f"max |level - fp64| = {err:.6f}")
    assert x.dtype == torch.uint8 and x.shape == (B, 1, H, W) and err <= BOUND
    assert x.float().std() > 20  # (not a blank frame)


@pytest.mark.gpu
@pytest.mark.parametrize("B,hw,H,W", SHAPES)
def test_moments_exact_on_the_levels_written(gpu, B, hw, H, W):
    src, mats = _case(B, hw, H, W, gpu)
    x, part = TF.upsample_levels_moments(src, H, W, affine=mats)
    asum = part.view(-1, 42).sum(0)
    assert torch.equal(asum, _lag_sums(x))
    if H == W:  # the separate kernels' sums (l1_input_stats takes square batches)
        assert torch.equal(asum, torch.ops.tdsa.l1_input_stats(x)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("B,hw,H,W", SHAPES)
def test_identity_is_the_plain_upsample(gpu, B, hw, H, W):
    src, _ = _case(B, hw, H, W, gpu)
    mats = torch.tensor([_mat(hw, H, W)] * B, dtype=torch.float32, device=gpu)
    x, _ = TF.upsample_levels_moments(src, H, W, affine=mats)
    keep = _interior(hw, H, W, gpu)
    assert keep.sum() > 0.8 * H * W
    assert torch.equal(x[:, 0][:, keep], TF.upsample_bilinear_u8(src, H, W, True)[:, 0][:, keep])


@pytest.mark.gpu
def test_nan_and_huge_matrices_run_and_leave_the_rest_alone(gpu):
    B, hw, H, W = SHAPES[0]
    bad = [[float("nan")] * 6, [1e30, -1e30, 1e30, 1e30, 1e30, -1e30]]
    src, mats = _case(B, hw, H, W, gpu, extra=bad)
    x, part = TF.upsample_levels_moments(src, H, W, affine=mats)
    assert (x[:B].double() - _ref_fp64(src[:B], mats[:B], H, W)).abs().max().item() <= BOUND
    assert torch.equal(part.view(-1, 42).sum(0), _lag_sums(x))


@pytest.mark.gpu
def test_fused_plan_consumes_augmented_partials(gpu):
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused

    torch.manual_seed(0)
    H = 64
    src, mats = _case(3, 28, H, H, gpu)
    y = torch.tensor([1, 4, 7], device=gpu)
    m1 = ConvNet(image_shape=(H, H), device=gpu, mode="fused")
    m2 = ConvNet(image_shape=(H, H), device=gpu, mode="fused")
    m2.load_state_dict(m1.state_dict())
    x1, part = TF.upsample_levels_moments(src, H, H, affine=mats)
    x2 = convnet_fused.attach_input_stats(x1.clone(), (part, None))
    before = convnet_fused.STATS["precomputed_input_moments"]
    l1, l2 = F.cross_entropy(m1(x1), y), F.cross_entropy(m2(x2), y)
    assert convnet_fused.STATS["precomputed_input_moments"] == before + 1 and torch.equal(l1, l2)
    l1.backward()
    l2.backward()
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p1.grad, p2.grad)


@pytest.mark.gpu
def test_loader_augment(gpu):
    from torch_distributed_sandbox_amd.data import DeviceUpsampleLoader, RandomAffine, SyntheticMNIST
    from torch_distributed_sandbox_amd.models import convnet_fused

    ds, aug = SyntheticMNIST(size=8), RandomAffine(degrees=15.0, translate=0.1, scale=(0.8, 1.1))
    mk = lambda a, seed=3: DeviceUpsampleLoader(ds, 4, (64, 64), gpu, levels=True, seed=seed, augment=a)
    plain, keep = list(mk(None)), _interior(28, 64, 64, gpu)
    for (xa, ya), (xb, yb), (xp, _), (xz, _) in zip(mk(aug), mk(aug), plain, mk(RandomAffine())):
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and not torch.equal(xa, xp)
        assert convnet_fused._take_input_stats(xa)[0] is not None
        assert torch.equal(xz[:, 0][:, keep], xp[:, 0][:, keep])
    assert not torch.equal(next(iter(mk(aug, seed=4)))[0], next(iter(mk(aug)))[0])


def test_cpu_path_and_arguments():
    from torch_distributed_sandbox_amd.data import DeviceUpsampleLoader, RandomAffine, SyntheticMNIST

    B, hw, H, W = 2, 20, 33, 40
    src, mats = _case(B, hw, H, W, "cpu")
    x, part = TF.upsample_levels_moments(src, H, W, affine=mats)
    assert part is None and (x.double() - _ref_fp64(src, mats, H, W)).abs().max().item() <= BOUND
    ds, aug = SyntheticMNIST(size=4), RandomAffine(degrees=10.0)
    with pytest.raises(ValueError):
        DeviceUpsampleLoader(ds, 2, (32, 32), "cpu", levels=False, augment=aug)
    a, b = (list(DeviceUpsampleLoader(ds, 2, (32, 32), "cpu", levels=True, augment=aug)) for _ in range(2))
    assert all(torch.equal(p[0], q[0]) for p, q in zip(a, b)) and a[0][0].dtype == torch.uint8
