"""The inference head on a packed fc weight (csrc/kernels/head_inf.hip on v_mfma_f32_16x16x32_f16,
ConvNet(inference_fc_precision="fp16" | "fp8")): the kernel against fp64 on operands quantised at its
own scales, the ops' refusals, the model end to end, the default left as it was, and the pack cache."""
import functools
import math

import pytest
import torch

from test_head_wide_gpu import _Ref
from test_inference_fp8_gpu import _ops, e4m3

pytestmark = pytest.mark.gpu

MAG, SC, P1INV, KSC = 48, 40, 41, 42  # ya's decode words: d = mag[40] mag[41] / mag[42]
KINDS = ["fp16", "fp8"]
CASES = [  # (P, B, NC), Q = P / 2
    (8, 1, 10),    # one block, half its columns valid: the smallest supported image
    (18, 3, 10),   # odd Q = 9: partial block rows and columns, misaligned weight rows
    (36, 5, 26),   # two class tiles, the second partial
    (24, 17, 64),  # two image tiles, four full class tiles
    (16, 32, 11),  # the largest batch
    (140, 2, 1),   # Q = 70: 18 block rows = 5 workgroups per channel, the last with 2 rows
]


def _blocked(y, fill):
    """[B, 32, Q, Q] -> pooled-blocked [B, 32, PB] (csrc/kernels/pooled_layout.h), padding = fill."""
    B, _, Q, _ = y.shape
    Q4, Q8 = (Q + 3) // 4, (Q + 7) // 8
    full = torch.full((B, 32, Q4 * 4, Q8 * 8), fill, dtype=y.dtype)
    full[:, :, :Q, :Q] = y
    return full.view(B, 32, Q4, 4, Q8, 8).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, -1).contiguous()


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


@functools.lru_cache(maxsize=None)
def _case(gpu, P, B, NC):
    g = torch.Generator().manual_seed(1000 * P + 10 * B + NC)
    Q = P // 2
    y = (torch.randn(B, 32, Q, Q, generator=g) * 40).half()
    a = torch.randn(32, generator=g)
    a[::5] = 0.0  # negative, zero and positive a
    aff2 = torch.cat([a, torch.randn(32, generator=g) * 0.5])
    b2 = torch.randn(32, generator=g) * 0.1
    scale = 10.0 ** (-4 * torch.rand(NC, generator=g))
    scale[0] = 1e-6
    scale[NC // 2] = 1.0 if NC > 1 else 1e-6
    w = torch.randn(NC, 32, Q, Q, generator=g) * scale.view(NC, 1, 1, 1)
    w[NC - 1, 5] *= 2.0 ** -16  # a channel 2^16 below its class's max (fp8: its own exponent)
    mag = torch.zeros(MAG, dtype=torch.int32)
    mag.view(torch.float32)[SC], mag.view(torch.float32)[P1INV], mag.view(torch.float32)[KSC] = 1.0, 0.5, 8.0
    return dict(y=y, ya=_blocked(y, float("nan")).to(gpu), aff2=aff2, b2=b2, w=w, mag=mag.to(gpu),
                bias=torch.randn(NC, generator=g))


def _head_ref(c, wexp, kind):
    """fp64 logits and sum |terms| on X rounded to fp16 at s_x and W rounded at 2^wexp, as head_inf.hip
    documents them."""
    a, b = c["aff2"][:32], c["aff2"][32:]
    ad, bd = a * (torch.tensor(1.0) * 0.5 / 8.0), _fma32(a, c["b2"], b)
    ex = 15 - math.frexp((ad.abs() * 65504.0 + bd.abs()).max().item())[1]  # bound * 2^ex < 2^15
    x = _fma32(ad.view(1, 32, 1, 1), c["y"], bd.view(1, 32, 1, 1)).clamp_min(0.0)
    xq = torch.ldexp(x, torch.tensor(ex)).half().double() * 2.0 ** -ex
    e = wexp.cpu()
    e = e.t().reshape(-1, 32, 1, 1) if kind == "fp8" else e.view(-1, 1, 1, 1)
    ws = torch.ldexp(c["w"], e)
    wq = (e4m3(ws) if kind == "fp8" else ws.half().double()) * torch.ldexp(torch.ones(()), -e).double()
    B, NC = x.shape[0], wq.shape[0]
    return (xq.reshape(B, -1) @ wq.reshape(NC, -1).t() + c["bias"].double(),
            xq.reshape(B, -1).abs() @ wq.reshape(NC, -1).abs().t())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P,B,NC", CASES)
def test_inference_head_against_fp64(gpu, kind, P, B, NC):
    """Both operands are fp16 values whose products are exact in fp32, so the only error is accumulation.
    A wave owns at most Q8 = ceil(Q / 8) blocks of its workgroup's band (4 block rows x Q8 blocks over 4
    waves) and each MFMA adds 32 products to the accumulator: chains of n = 32 Q8 fp32 additions; the
    waves, bands and channels are summed in fp64 and the logit is rounded once to fp32.  Per logit:
    n 2^-24 sum |terms| + 2^-24 |ref|."""
    c, ops = _case(gpu, P, B, NC), _ops()
    wpk, wexp = ops.fc_pack_inference(c["w"].reshape(NC, -1).to(gpu), P, kind)
    got = ops.fused_head_forward_inference(c["ya"], c["aff2"].to(gpu), c["b2"].to(gpu), c["mag"], wpk, wexp,
                                           c["bias"].to(gpu), P, NC, kind).double().cpu()
    assert NC == 1 or int(wexp.max()) - int(wexp.min()) >= (12 if kind == "fp16" else 16)
    ref, sabs = _head_ref(c, wexp, kind)
    n = 32 * ((P // 2 + 7) // 8)
    bound = n * 2.0 ** -24 * sabs + 2.0 ** -24 * ref.abs()
    err = (got - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{kind} P={P} B={B} NC={NC}: max err/bound {worst:.3f}, max |ref| {ref.abs().max().item():.3e}")
    assert got.shape == (B, NC) and torch.isfinite(got).all() and ref.abs().min() > 0
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("bad", ["ya_dtype", "pack_short", "P", "batch_33"])
def test_inference_head_refusals(gpu, bad):
    """Each bad argument raises before anything is allocated: the allocator's peak does not move."""
    P, B, NC = 18, 3, 10
    c, ops = _case(gpu, P, B, NC), _ops()
    wpk, wexp = ops.fc_pack_inference(c["w"].reshape(NC, -1).to(gpu), P, "fp16")
    ya = c["ya"]
    if bad == "ya_dtype":
        ya = ya.float()
    elif bad == "pack_short":
        wpk = wpk[:-8]
    elif bad == "P":
        P = 34  # (Q = 17: another block count than Q = 9, in ya and in the pack)
    else:
        ya = torch.zeros(33, 32, ya.shape[2], dtype=torch.float16, device=gpu)
    args = (c["aff2"].to(gpu), c["b2"].to(gpu), c["mag"], wpk, wexp, c["bias"].to(gpu), P, NC, "fp16")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    with pytest.raises(RuntimeError):
        ops.fused_head_forward_inference(ya, *args)
    assert torch.cuda.max_memory_allocated(gpu) == base


@functools.lru_cache(maxsize=None)
def _model_case(gpu, kind, NC, B):
    """One fused training step at batch 3 (it moves the running statistics), then the eval forward of
    batch B with the option: (logits, the fp64 model's, its sum |X W|, the default plan's logits or None
    where that plan does not take the shape, packs and head launches counted)."""
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused, fc_in_features
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    H = 64
    torch.manual_seed(0)
    ours = ConvNet(num_classes=NC, image_shape=(H, H), inference_fc_precision=kind)
    with torch.no_grad():
        ours.layer2[1].weight[::3].neg_()
    ours = ours.to(gpu)
    x = torch.rand(B, 1, H, H, device=gpu)
    CrossEntropyLoss()(ours(x[:3]), torch.randint(0, NC, (3,), device=gpu)).backward()
    ref = _Ref(fc_in_features((H, H)), NC).double()
    ref.load_state_dict({k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in ours.state_dict().items()})
    ours.eval(), ref.eval()
    before = dict(convnet_fused.STATS)
    with torch.no_grad():
        got = ours(x).double().cpu()
        counts = tuple(convnet_fused.STATS[k] - before[k] for k in ("inference_fc_packs", "inference_fc_head"))
        feat = ref.layer2(ref.layer1(x.double().cpu())).reshape(B, -1)
        want, sabs = ref.fc(feat), feat.abs() @ ref.fc.weight.abs().t()
        ours.inference_fc_precision = "fp32"
        base = ours(x).double().cpu() if convnet_fused.supported_inference(ours, x) else None
    return got, want, sabs, base, counts


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("NC,B", [(10, 3), (26, 3), (26, 20)])
def test_inference_fc_model(gpu, kind, NC, B):
    """Per logit: the default plan's own distance from the fp64 model (measured here; for (26, 20), which
    the default plan does not take, the (26, 3) case's largest distance per sum |X W|) plus the fc
    quantisation u sum |X W|, u = 2^-10 for fp16 (both operands rounded once) and 2^-4 + 2^-11 for fp8."""
    got, want, sabs, base, counts = _model_case(gpu, kind, NC, B)
    assert counts == (1, 1) and got.shape == (B, NC) and (base is None) == (B > 16)
    if base is None:
        _, want3, sabs3, base3, _ = _model_case(gpu, kind, NC, 3)
        allow = ((base3 - want3).abs() / sabs3).max() * sabs
    else:
        allow = (base - want).abs()
    u = 2.0 ** -10 if kind == "fp16" else 2.0 ** -4 + 2.0 ** -11
    err, bound = (got - want).abs(), allow + u * sabs
    print(f"{kind} NC={NC} B={B}: max err/bound {(err / bound).max().item():.3f}, allowance share "
          f"{(allow / bound).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all()


def test_default_fc_precision_unchanged(gpu, monkeypatch):
    """inference_fc_precision="fp32" and the argument omitted give equal logits and pack nothing; an
    unknown value raises; the environment overrides."""
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused

    monkeypatch.delenv("TDS_INFERENCE_FC_PRECISION", raising=False)
    torch.manual_seed(1)
    a = ConvNet(image_shape=(32, 32), device=gpu).eval()
    b = ConvNet(image_shape=(32, 32), device=gpu, inference_fc_precision="fp32").eval()
    b.load_state_dict(a.state_dict())
    x = torch.rand(2, 1, 32, 32, device=gpu)
    before = dict(convnet_fused.STATS)
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    assert convnet_fused.STATS == before and a.inference_fc_precision == "fp32"
    with pytest.raises(ValueError):
        ConvNet(image_shape=(32, 32), inference_fc_precision="fp4")
    monkeypatch.setenv("TDS_INFERENCE_FC_PRECISION", "fp8")
    assert ConvNet(image_shape=(32, 32)).inference_fc_precision == "fp8"


def test_fc_pack_cache(gpu):
    """The pack is made once for many eval batches, and again after a training step that moved
    fc.weight inside the head backward (no version bump): the logits then equal a fresh model's that
    loaded the trained state."""
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    H = 256  # (fc.weight of 2^20 elements and more: DDP steps it inside the head backward)
    torch.manual_seed(2)
    m = ConvNet(image_shape=(H, H), device=gpu, mode="fused", inference_fc_precision="fp16")
    d = DistributedDataParallel(m, overlap_optimizer=True)  # the fc step runs inside the head backward
    o = d.attach_optimizer(SGD(m.parameters(), 0.1))
    x, y = torch.rand(3, 1, H, H, device=gpu), torch.randint(0, 10, (3,), device=gpu)
    packs = convnet_fused.STATS["inference_fc_packs"]
    m.eval()
    with torch.no_grad():
        g1, g2 = m(x), m(x)
    assert convnet_fused.STATS["inference_fc_packs"] == packs + 1 and torch.equal(g1, g2)
    m.train()
    w0 = m.fc.weight.detach().clone()
    loss = CrossEntropyLoss()(d(x), y)
    o.zero_grad()
    loss.backward()
    assert not torch.equal(m.fc.weight, w0)  # stepped inside the head backward
    o.step()
    m.eval()
    with torch.no_grad():
        g3 = m(x)
    assert convnet_fused.STATS["inference_fc_packs"] == packs + 2 and not torch.equal(g3, g1)
    fresh = ConvNet(image_shape=(H, H), device=gpu, inference_fc_precision="fp16")
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh.eval()(x), g3)
