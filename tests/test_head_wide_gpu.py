"""The fused head for 11 .. 64 classes (csrc/kernels/head_wide.hip: fc products on v_mfma_f32_16x16x4_f32,
exact fp32) against fp64: the kernels alone, the weight forms of the fused step, the model end to end
on the fused plan, and the new ops' refusals."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _tf32ref import rel, tf32_convs
from test_fused_gpu import _check, _head_case, _ops, mag_floats, new_mag, set_ya_scale, ypart

pytestmark = pytest.mark.gpu

CASES = [  # (P, B, NC)
    (8, 1, 11),     # Q = 4, one block, one image, the first class of a second tile
    (18, 5, 16),    # Q = 9: all four row-alignment classes, partial blocks both ways, a full class tile
    (20, 8, 17),    # Q = 10: alignment classes 0 and 2, a tile + 1 class
    (38, 16, 33),   # the image tile full (two workgroups per channel in the backward)
    (64, 3, 64),    # every class tile full
    (150, 2, 11),   # Q = 75 = the 64-column span of a wave iteration + 11: a second, partial span
]
STEP_CASES = [c for c in CASES if c[1] <= 8]  # (Q = 9 and 75 odd)


@functools.lru_cache(maxsize=None)
def _case(gpu, P, B, NC):
    """Inputs of test_fused_gpu._head_case with an NC-row fc, the wide forward's outputs and the fp64
    autograd results of BN2 (batch statistics) -> ReLU -> pool -> fc.  Computed once; nothing in it is
    written afterwards."""
    ops = _ops()
    y2, b2, g2, be2, _, _, partial2, ya = _head_case(gpu, P, B, P + B + NC)
    Q = P // 2
    wfc = torch.randn(NC, 32 * Q * Q, device=gpu) * 0.01
    bfc = torch.randn(NC, device=gpu)
    dl = torch.randn(B, NC, device=gpu)
    logits, stats2, aff2, wmax = ops.fused_head_wide_forward(ya, partial2, b2, g2, be2, None, None, None, 0.1, 1e-5,
                                                             wfc, bfc, P)
    yr = y2.permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    gr, ber, wr = (t.double().cpu().requires_grad_(True) for t in (g2, be2, wfc))
    pz = F.max_pool2d(F.relu(F.batch_norm(yr, None, None, gr, ber, True, 0.1, 1e-5)), 2, 2)
    pz.retain_grad()
    ref = F.linear(pz.reshape(B, -1), wr, bfc.double().cpu())
    ref.backward(dl.double().cpu())
    return {"ya": ya, "b2": b2, "g2": g2, "wfc": wfc, "bfc": bfc, "dl": dl, "logits": logits, "stats2": stats2,
            "aff2": aff2, "wmax": wmax, "ref_logits": ref.detach(), "ref_dW": wr.grad, "ref_dg": gr.grad,
            "ref_dbe": ber.grad, "ref_g": (pz.grad * (pz > 0)).detach()}


def _backward(c, P, wfc, dw_out=None, lr=0.0, **kw):
    return _ops().fused_head_wide_backward(c["dl"], c["ya"], c["stats2"], c["aff2"], c["b2"], c["g2"], wfc, c["wmax"],
                                           P, dw_out, 1.0, lr, **kw)


@pytest.mark.parametrize("P,B,NC", CASES)
def test_wide_head_forward_backward(gpu, P, B, NC):
    """Logits, dW, dbfc, dgamma2, dbeta2 and g2m against fp64 at test_head_forward_backward's bounds."""
    c = _case(gpu, P, B, NC)
    Q = P // 2
    _check(c["logits"], c["ref_logits"], 1e-5, "logits")
    mag = set_ya_scale(new_mag(gpu, B, P))
    ypart(mag).zero_()
    dW, dbfc, dg2, dbe2, g2m, kbuf = _backward(c, P, c["wfc"], mag=mag)
    assert g2m.shape == (B, 32, Q, Q) and g2m.dtype == torch.float16 and kbuf.shape == (128,)
    ginv = kbuf[96:]
    assert torch.equal(torch.frexp(ginv).mantissa, torch.full_like(ginv, 0.5))  # powers of two
    assert g2m.float().abs().max().item() < 2.0 ** 14
    g2f = g2m.float() * ginv.view(1, 32, 1, 1)
    gm32 = mag_floats(mag)[32].item()  # max |g2m| before rounding: the conv2 backward's bound
    assert abs(gm32 - g2f.abs().max().item()) <= 2.0 ** -11 * gm32
    _check(dW, c["ref_dW"], 1e-5, "dW")
    _check(dbfc, c["dl"].double().sum(0), 1e-6, "dbfc")
    _check(dg2, c["ref_dg"], 1e-5, "dgamma2")
    _check(dbe2, c["ref_dbe"], 1e-5, "dbeta2")
    _check(g2f, c["ref_g"], 2.0 ** -11 + 1e-5, "g2m (fp16, 2^-11 relative)")
    # the forward on the finished affine with labels: the same logits, torch's loss and its gradient
    labels = torch.randint(0, NC, (B,), device=gpu)
    lg, _, loss, dlg = _ops().fused_head_wide_forward_aff(c["ya"], c["aff2"], c["b2"], None, c["wfc"], c["bfc"], P, labels)
    assert torch.equal(lg, c["logits"])
    z = lg.double().requires_grad_(True)
    want = F.cross_entropy(z, labels)
    want.backward()
    _check(loss, want, 1e-6, "loss")
    _check(dlg, z.grad, 1e-6, "dlogits")


@pytest.mark.parametrize("P,B,NC", STEP_CASES)
def test_wide_head_fused_step(gpu, P, B, NC):
    """The weight forms: dW written + plain SGD, the momentum rule over two steps against
    torch.optim.SGD in fp64 on the same gradients, and the update-only forms bit for bit."""
    c = _case(gpu, P, B, NC)
    w0 = c["wfc"]
    dW = _backward(c, P, w0)[0]
    lr = 0.5
    w1, dW2 = w0.clone(), torch.empty_like(w0)
    _backward(c, P, w1, dW2, lr)
    assert torch.equal(dW2, dW)
    assert torch.allclose(w1, w0 - lr * dW, rtol=0, atol=1e-6)
    w1u = w0.clone()
    assert _backward(c, P, w1u, None, lr, keep_dw=False)[0] is None
    assert torch.equal(w1u, w1)
    # momentum + weight decay + nesterov, two steps (dW = dl^T X does not depend on W: the same both steps)
    rule = dict(weight_decay=0.01, momentum=0.9, dampening=0.0, nesterov=True)
    wk, wu = w0.clone(), w0.clone()
    bk, bu = torch.full_like(w0, float("nan")), torch.full_like(w0, float("nan"))  # (created by the first step)
    for first in (True, False):
        _backward(c, P, wk, dW2, lr, mom_buf=bk, first_step=first, **rule)
        assert torch.equal(dW2, dW)
        _backward(c, P, wu, None, lr, keep_dw=False, mom_buf=bu, first_step=first, **rule)
    assert torch.equal(wu, wk) and torch.equal(bu, bk)
    p = w0.double().cpu().requires_grad_(True)
    opt = torch.optim.SGD([p], lr=lr, **rule)
    for _ in range(2):
        p.grad = dW.double().cpu()
        opt.step()
    bref = opt.state[p]["momentum_buffer"]
    # fp32 roundings per element and step (common.h sgd_rule_step): 4 into the buffer, counted as 5 for
    # the momentum's own fp32 rounding, and 2 more into the weight, each 2^-24 of its value; the
    # buffer's error enters the weight times lr (1 + momentum) < 2 lr
    eb = 2 * 5 * 2.0 ** -24 * bref.abs().max().item()
    ew = 2 * 2 * 2.0 ** -24 * p.detach().abs().max().item() + 2 * 2 * lr * eb
    assert (bk.double().cpu() - bref).abs().max().item() <= eb
    assert (wk.double().cpu() - p.detach()).abs().max().item() <= ew


class _Ref(nn.Module):
    """The fp64 reference module of test_fused_gpu._fused_vs_ref with NC classes."""

    def __init__(self, inf, nc):
        super().__init__()
        self.layer1 = nn.Sequential(nn.Conv2d(1, 16, 5, 1, 2), nn.BatchNorm2d(16), nn.ReLU(), nn.MaxPool2d(2, 2))
        self.layer2 = nn.Sequential(nn.Conv2d(16, 32, 5, 1, 2), nn.BatchNorm2d(32), nn.ReLU(), nn.MaxPool2d(2, 2))
        self.fc = nn.Linear(inf, nc)

    def forward(self, x):
        o = self.layer2(self.layer1(x))
        return self.fc(o.reshape(o.size(0), -1))


def test_wide_head_model_end_to_end(gpu):
    """ConvNet(num_classes=26, mode="fused"): one training step and the eval forward against the fp64
    model, at the fused-model test's bounds (1e-3, or 1.5x what TF32-operand convolutions make).
    Without the wide head both raise RuntimeError (mode="fused" refuses more than ten classes)."""
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused, fc_in_features
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    B, H, NC = 3, 64, 26
    torch.manual_seed(0)
    ours = ConvNet(num_classes=NC, image_shape=(H, H), mode="fused")
    with torch.no_grad():
        ours.layer2[1].weight[::3].neg_()  # some negative BN2 gammas: min-pooled windows
    ref = _Ref(fc_in_features((H, H)), NC).double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in ours.state_dict().items()})
    reft = tf32_convs(copy.deepcopy(ref))
    ours = ours.to(gpu)
    x = torch.rand(B, 1, H, H, device=gpu)
    y = torch.randint(0, NC, (B,), device=gpu)
    before = convnet_fused.STATS["head_wide"]
    logits = ours(x)
    loss = CrossEntropyLoss()(logits, y)
    loss.backward()
    assert convnet_fused.STATS["head_wide"] == before + 1
    x64 = x.double().cpu()
    rlog, tlog = ref(x64), reft(x64)
    rl, tl = F.cross_entropy(rlog, y.cpu()), F.cross_entropy(tlog, y.cpu())
    rl.backward()
    tl.backward()
    e, et = rel(logits.detach().cpu(), rlog.detach()), rel(tlog.detach(), rlog.detach())
    assert e <= max(1e-3, 1.5 * et), (e, et)
    assert abs(loss.item() - rl.item()) <= max(2e-4 * max(1.0, abs(rl.item())), 1.5 * abs(tl.item() - rl.item()))
    rp, rt = dict(ref.named_parameters()), dict(reft.named_parameters())
    for n, p in ours.named_parameters():
        g, rg = p.grad.double().cpu(), rp[n].grad
        if n.endswith("0.bias"):  # analytically zero (bias before BN): rounding noise both sides
            wsc = rp[n.replace("bias", "weight")].grad.abs().max().item()
            assert (g - rg).abs().max().item() <= 1e-3 * wsc + 1e-6, n
            continue
        e, et = rel(g, rg), rel(rt[n].grad, rg)
        assert e <= max(1e-3, 1.5 * et), f"{n}: rel L2 err {e:.3e} (TF32 convs: {et:.3e})"
    # eval under no_grad: the inference plan on the running statistics that step left
    ours.eval(), ref.eval(), reft.eval()
    with torch.no_grad():
        got, want, wt = ours(x), ref(x64), reft(x64)
    assert got.shape == (B, NC)
    e, et = rel(got.cpu(), want), rel(wt, want)
    assert e <= max(1e-3, 1.5 * et), (e, et)


@pytest.mark.parametrize("B,NC", [(1, 65), (17, 11)])
def test_wide_head_refusals(gpu, B, NC):
    """More than 64 classes or 16 images: both forwards and the backward raise before any launch -- the
    weight and dw_out keep their bits."""
    ops = _ops()
    P, Q = 8, 4
    ya = torch.zeros(B, 32, 32, device=gpu, dtype=torch.float16)
    wfc = torch.full((NC, 32 * Q * Q), 3.0, device=gpu)
    dw = torch.full_like(wfc, 7.0)
    f32 = functools.partial(torch.zeros, device=gpu)
    aff2, b2, dl = f32(64), f32(32), f32(B, NC)
    wmax = torch.zeros(32, 64, device=gpu, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.fused_head_wide_forward_aff(ya, aff2, b2, None, wfc, None, P)
    with pytest.raises(RuntimeError):
        ops.fused_head_wide_forward(ya, torch.zeros(64, device=gpu, dtype=torch.float64), b2, None, None, None, None,
                                    None, 0.1, 1e-5, wfc, None, P)
    with pytest.raises(RuntimeError):
        ops.fused_head_wide_backward(dl, ya, aff2, aff2, b2, None, wfc, wmax, P, dw, 1.0, 0.5)
    assert bool((wfc == 3.0).all()) and bool((dw == 7.0).all())


def test_more_than_64_classes_train_on_the_layers_path(gpu):
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused

    model = ConvNet(num_classes=65, image_shape=(16, 16), mode="auto").to(gpu)
    before = convnet_fused.STATS["head_wide"]
    logits = model(torch.rand(2, 1, 16, 16, device=gpu))
    logits.sum().backward()
    assert logits.shape == (2, 65) and convnet_fused.STATS["head_wide"] == before
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
