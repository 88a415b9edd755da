"""The inference plan's FP8 (E4M3) conv2 (csrc/kernels/conv2_fwd_fp8.hip on
v_mfma_scale_f32_16x16x128_f8f6f4, ConvNet(inference_precision="fp8")): the kernel against fp64 on
operands quantised at its own scales, the new ops' refusals, the model end to end on both heads, and
the default left as it was."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from _tf32ref import rel
from test_head_wide_gpu import _Ref

pytestmark = pytest.mark.gpu

MAG, SC, P1INV, KSC, P1Q = 48, 40, 41, 42, 45  # mag words (csrc/kernels/conv2_common.h, conv2_fp8.h)
CASES = [  # (P, B)
    (8, 1),    # one tile, every border
    (18, 3),   # partial tiles both ways, odd Q = 9
    (38, 2),   # more than one tile per direction plus an edge
    (64, 1),   # full tiles only
    (8, 32),   # the largest batch
]


def _ops():
    import torch_distributed_sandbox_amd as tds

    return tds._ext.ops()


def e4m3(t):
    """Round to OCP E4M3 (nearest even), kept in fp64; the callers' values are within +-448."""
    return t.float().to(torch.float8_e4m3fn).double()


def _unpool(ya, B, P):
    """ya [B, 32, PB] (pooled-blocked, csrc/kernels/pooled_layout.h) -> [B, 32, Q, Q] fp64."""
    Q = P // 2
    Q4, Q8 = (Q + 3) // 4, (Q + 7) // 8
    v = ya.double().cpu().view(B, 32, Q4, Q8, 4, 8).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, Q4 * 4, Q8 * 8)
    return v[:, :, :Q, :Q]


def fp8_conv2_ref(p1h, w2, wexp, psc, gamma):
    """fp64 conv2 (no bias) over p1h [B,16,P,P] and w2 rounded to E4M3 at the scales psc / 2^wexp, then
    each 2x2 window's extreme by gamma's sign (gamma = 0: the first position): (value, sum |terms|)."""
    B, _, P, _ = p1h.shape
    ws = torch.ldexp(torch.ones(32), wexp.cpu().float()).view(32, 1, 1, 1)
    wq = (e4m3(w2.cpu() * ws) / ws.double()).reshape(32, 400)
    cols = F.unfold(e4m3(p1h.cpu().float() * psc) / psc, 5, padding=2)  # [B, 400, P*P]
    y, s = ((m @ c).view(B, 32, P // 2, 2, P // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, P // 2, P // 2, 4)
            for m, c in ((wq, cols), (wq.abs(), cols.abs())))
    g = gamma.cpu().view(1, 32, 1, 1)
    idx = torch.where(g < 0, y.argmin(-1), y.argmax(-1))
    idx = torch.where(g == 0, torch.zeros_like(idx), idx).unsqueeze(-1)
    return y.gather(-1, idx).squeeze(-1), s.gather(-1, idx).squeeze(-1)


@functools.lru_cache(maxsize=None)
def _case(gpu, P, B):
    g = torch.Generator().manual_seed(100 * P + B)
    p1 = torch.rand(B, P, P, 16, generator=g) * 6.0
    p1 = (p1 * (torch.rand(B, P, P, 16, generator=g) > 0.45)).half()  # sparse, as after ReLU
    p1[:, : P // 3, P // 2:] = 0
    w2 = torch.randn(32, 16, 5, 5, generator=g) * 0.05
    w2[3] *= 1e-4  # near 5e-6
    w2[7] = torch.randn(16, 5, 5, generator=g)  # O(1): the per-channel scales differ by many binades
    gamma = torch.rand(32, generator=g) + 0.5
    gamma[::3] *= -1.0  # min-pooled windows
    gamma[5] = 0.0
    psc = 2.0 ** 6  # 6 * 64 <= 448
    mag = torch.zeros(MAG, dtype=torch.int32, device=gpu)
    mag.view(torch.float32)[P1INV] = 1.0
    mag.view(torch.float32)[P1Q] = psc
    ops = _ops()
    wp8, wexp = ops.conv2_pack_fp8(w2.to(gpu), mag)
    ya = ops.fused_conv2_forward_inference_fp8(p1.to(gpu), wp8, wexp, gamma.to(gpu), mag)
    return p1, w2, gamma, psc, wexp, mag.view(torch.float32).cpu(), ya


@pytest.mark.parametrize("P,B", CASES)
def test_fp8_conv2_against_fp64(gpu, P, B):
    """Products of two E4M3 values are exact in fp32, so the kernel's only errors are the fp32
    accumulation of 400 terms and ya's fp16 store: per element 2^-11 |ref| + 400 * 2^-24 * sum |terms|."""
    p1, w2, gamma, psc, wexp, magf, ya = _case(gpu, P, B)
    assert ya.shape == (B, 32, ((P // 2 + 3) // 4) * ((P // 2 + 7) // 8) * 32) and ya.dtype == torch.float16
    assert wexp.cpu().unique().numel() > 2 and int(wexp[3]) - int(wexp[7]) >= 16
    ref, sabs = fp8_conv2_ref(p1.permute(0, 3, 1, 2), w2, wexp, psc, gamma)
    # the head's decode of ya (y2 - b2 = ya * mag[40] mag[41] / mag[42]) from the words this path wrote
    d = (magf[SC] * magf[P1INV] / magf[KSC]).item()
    got = _unpool(ya, B, P) * d
    err = (got - ref).abs()
    bound = 2.0 ** -11 * ref.abs() + 400 * 2.0 ** -24 * sabs
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"P={P} B={B}: max err/bound {worst:.3f}, max |ref| {ref.abs().max().item():.3e}")
    assert torch.isfinite(got).all() and ref.abs().max() > 0
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("bad", ["dtype", "strided_p1", "pack_size"])
def test_fp8_conv2_refusals(gpu, bad):
    """Each bad argument raises before ya is allocated: the allocator's peak does not grow by a ya."""
    p1, w2, gamma, _, wexp, _, _ = _case(gpu, 64, 1)
    ops = _ops()
    mag = torch.zeros(MAG, dtype=torch.int32, device=gpu)
    mag.view(torch.float32)[P1Q] = 64.0
    wp8, _ = ops.conv2_pack_fp8(w2.to(gpu), mag)
    p1 = p1.to(gpu)
    if bad == "dtype":
        p1 = p1.float()
    elif bad == "strided_p1":
        p1 = p1.transpose(1, 2)
    else:
        wp8 = wp8[:-16]
    ya_bytes = 32 * 8 * 4 * 32 * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    with pytest.raises(RuntimeError):
        ops.fused_conv2_forward_inference_fp8(p1, wp8, wexp, gamma.to(gpu), mag)
    assert torch.cuda.max_memory_allocated(gpu) - base < ya_bytes


def _fp8_convs(model, wexp, psc, p1_scale):
    """The fp64 model with conv2's operands E4M3-rounded at the kernel's scales (as
    _tf32ref.tf32_convs builds the TF32 model)."""
    conv = model.layer2[0]
    ws = torch.ldexp(torch.ones(32), wexp.cpu().float()).view(32, 1, 1, 1)

    def fwd(x):
        wq = e4m3(conv.weight.float() * ws) / ws.double()
        # (p1 as layer 1 stores it, fp16 at p1_scale, then the FP8 scale)
        xq = e4m3((x * p1_scale).half().float() * psc) / (psc * p1_scale)
        Bx, _, Hx, Wx = x.shape
        return (wq.reshape(32, -1) @ F.unfold(xq, 5, padding=2) + conv.bias.view(1, -1, 1)).view(Bx, 32, Hx, Wx)

    conv.forward = fwd
    return model


@pytest.mark.parametrize("NC", [10, 26])
def test_fp8_model_end_to_end(gpu, NC):
    """One training step (which moves the running statistics), then eval + no_grad logits of
    inference_precision="fp8" against the fp64 model: e <= max(1e-3, 1.5 e_q), e_q the error of the
    fp64 model whose conv2 operands are E4M3-rounded at the kernel's scales."""
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused, fc_in_features
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    B, H = 3, 64
    torch.manual_seed(0)
    ours = ConvNet(num_classes=NC, image_shape=(H, H), inference_precision="fp8")
    with torch.no_grad():
        ours.layer2[1].weight[::3].neg_()
    ours = ours.to(gpu)
    x = torch.rand(B, 1, H, H, device=gpu)
    CrossEntropyLoss()(ours(x), torch.randint(0, NC, (B,), device=gpu)).backward()
    ref = _Ref(fc_in_features((H, H)), NC).double()
    ref.load_state_dict({k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in ours.state_dict().items()})
    ours.eval(), ref.eval()
    # the kernel's scales: the exponents from the pack, p1's scales from the constants launch
    ops = _ops()
    l1, l2 = ours.layer1, ours.layer2
    mag = torch.zeros(MAG, dtype=torch.int32, device=gpu)
    aff1, _ = ops.inference_constants(x, l1[0].weight, l1[0].bias, l1[1].weight, l1[1].bias, l1[1].running_mean,
                                      l1[1].running_var, float(l1[1].eps), l2[1].weight, l2[1].bias,
                                      l2[1].running_mean, l2[1].running_var, float(l2[1].eps), mag)
    _, wexp = ops.conv2_pack_fp8(l2[0].weight.detach(), mag)
    refq = _fp8_convs(copy.deepcopy(ref), wexp, mag.view(torch.float32)[P1Q].item(), aff1[32].item())
    before = convnet_fused.STATS["inference_fp8"]
    with torch.no_grad():
        got, want, wq = ours(x), ref(x.double().cpu()), refq(x.double().cpu())
    assert convnet_fused.STATS["inference_fp8"] == before + 1 and got.shape == (B, NC)
    e, eq = rel(got.cpu(), want), rel(wq, want)
    print(f"NC={NC}: rel L2 error of the logits {e:.3e}, of the E4M3-operand fp64 model {eq:.3e}")
    assert e <= max(1e-3, 1.5 * eq), (e, eq)


def test_default_precision_unchanged(gpu, monkeypatch):
    """inference_precision="tf32" and the argument omitted give equal logits without the FP8 launch;
    "fp8" counts one launch per eval forward; an unknown value raises; the environment overrides."""
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused

    monkeypatch.delenv("TDS_INFERENCE_PRECISION", raising=False)
    torch.manual_seed(1)
    a = ConvNet(image_shape=(32, 32), device=gpu).eval()
    b = ConvNet(image_shape=(32, 32), device=gpu, inference_precision="tf32").eval()
    c = ConvNet(image_shape=(32, 32), device=gpu, inference_precision="fp8").eval()
    b.load_state_dict(a.state_dict()), c.load_state_dict(a.state_dict())
    x = torch.rand(2, 1, 32, 32, device=gpu)
    before = convnet_fused.STATS["inference_fp8"]
    with torch.no_grad():
        ya, yb = a(x), b(x)
        assert torch.equal(ya, yb) and convnet_fused.STATS["inference_fp8"] == before
        yc = c(x)
        assert convnet_fused.STATS["inference_fp8"] == before + 1
        c(x)
        assert convnet_fused.STATS["inference_fp8"] == before + 2
    assert torch.isfinite(yc).all() and not torch.equal(yc, ya)
    with pytest.raises(ValueError):
        ConvNet(image_shape=(32, 32), inference_precision="fp4")
    monkeypatch.setenv("TDS_INFERENCE_PRECISION", "fp8")
    assert ConvNet(image_shape=(32, 32)).inference_precision == "fp8"
