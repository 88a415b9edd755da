"""Momentum SGD inside the pooled fc exchange's update kernels (ops.head_update_pooled_step) and the plan
that reaches them.  Reference: torch's rule in fp64 on the fp32 dW of head_update_pooled's mode 1, with
tests/test_sgd_momentum_gpu.py's per-element bounds; and, bit for bit, that dW and the flat sweep."""
import functools

import pytest
import torch

from test_fused_gpu import _ops
from test_head_ranges_gpu import SENTINEL, _guarded, _guards_kept
from test_head_wide_exchange_gpu import _case
from test_sgd_momentum_gpu import (HP_SETS, _batch, _margins, _one_flat_buffer, _plan_step, _rule_ref, _twins, _within,
                                   pg)  # noqa: F401  (pg: the world-1 process group fixture)

pytestmark = pytest.mark.gpu

GUARD, LR = 64, 0.01
# ten classes: odd Q off the 16-B grid; aligned, two ranks; NB = 8, partial 8-column block, several chunks.
# Wide: NT = 1, 3, 4; a K step of two ranks' images; 16 images; odd Q
TEN = [(38, 5, 10, 1), (64, 3, 10, 2), (130, 8, 10, 3)]
WIDE = [(18, 5, 11, 1), (38, 16, 33, 2), (18, 3, 64, 3)]
CASES = [c + (hp,) for c in TEN for hp in HP_SETS] + [c + (list(HP_SETS)[i + 1],) for i, c in enumerate(WIDE)]


@pytest.mark.parametrize("P,B,NC,W,hp", CASES)
def test_pooled_update_momentum_step(gpu, P, B, NC, W, hp):
    """Two consecutive steps (the first creates the buffer, ignoring the sentinels in it), guarded."""
    ops = _ops()
    ya_all, rec_all, x_all = _case(gpu, P, B, NC, W)  # each rank its own BN2 affine and ya scale
    K, scale = x_all.shape[1], 1.0 / W
    mom, wd, damp, nest = HP_SETS[hp]
    g = torch.Generator(device=gpu).manual_seed(P + NC)
    w_cur = torch.randn(NC, K, device=gpu, generator=g) * 0.01
    b_cur = torch.full_like(w_cur, SENTINEL)
    for step in range(2):
        first, where = step == 0, (P, B, NC, W, hp, step)
        dl = torch.randn(W * B, NC, device=gpu, generator=g)
        dW = torch.empty_like(w_cur)
        ops.head_update_pooled(dl, ya_all, rec_all, w_cur, dW, P, scale, 0.0, 1)
        b_ref, w_ref, bound_b, bound_w, terms = _rule_ref(w_cur, dW, b_cur, LR, HP_SETS[hp], first)
        _margins(terms, bound_w, where)
        (wbuf, w), (bbuf, b) = _guarded(gpu, NC, K, GUARD), _guarded(gpu, NC, K, GUARD)
        w.copy_(w_cur), b.copy_(b_cur)
        ops.head_update_pooled_step(dl, ya_all, rec_all, w, b, P, scale, LR, wd, mom, damp, nest, first)
        assert _guards_kept(wbuf, GUARD) and _guards_kept(bbuf, GUARD), where
        _within(b, b_ref, bound_b, where + ("buf",))
        _within(w, w_ref, bound_w, where + ("w",))
        ops.sgd_step_([w_cur.view(-1)], [dW.view(-1)], [b_cur.view(-1)], LR, wd, mom, damp, nest, first)
        assert torch.equal(w, w_cur) and torch.equal(b, b_cur), where  # mode 1's dW + the flat sweep: the same bits


def _call(c, w, b, P, mom=0.9):
    ya_all, rec_all, _ = c
    dl = torch.ones(ya_all.shape[0] * ya_all.shape[1], w.shape[0], device=w.device)
    _ops().head_update_pooled_step(dl, ya_all, rec_all, w, b, P, 1.0, LR, 0.0, mom, 0.0, False, False)


def test_wide_rule_form_is_one_launch(gpu):
    """144 images: more than one launch holds, refused with weight and buffer untouched."""
    c = _case(gpu, 8, 16, 11, 9)
    w, b = torch.full((11, c[2].shape[1]), 0.25, device=gpu), torch.full((11, c[2].shape[1]), 0.5, device=gpu)
    with pytest.raises(RuntimeError):
        _call(c, w, b, 8)
    assert bool((w == 0.25).all()) and bool((b == 0.5).all())


def test_pooled_step_refusals(gpu):
    """What the op refuses before any launch: weight and buffer stay as they were."""
    P, NC, c = 38, 10, _case(gpu, 38, 5, 10, 1)
    K = c[2].shape[1]
    w, good = torch.full((NC, K), 0.25, device=gpu), torch.full((NC, K), 0.5, device=gpu)
    bad = {
        "shape": dict(b=torch.full((NC, K + 4), 0.5, device=gpu)),
        "dtype": dict(b=torch.full((NC, K), 0.5, device=gpu, dtype=torch.float64)),
        "device": dict(b=torch.full((NC, K), 0.5)),
        "misaligned": dict(b=torch.full((NC * K + 1,), 0.5, device=gpu)[1:].view(NC, K)),
        "alias": dict(b=w),
        "momentum 0": dict(b=good, mom=0.0),
    }
    for name, kw in bad.items():
        with pytest.raises(RuntimeError):
            _call(c, w, P=P, **kw)
        assert bool((w == 0.25).all()) and bool((good == 0.5).all()), name
        assert kw["b"] is w or bool((kw["b"] == 0.5).all()), name
    _call(c, w, good, P)  # the call they all vary is a good one
    assert not bool((w == 0.25).all()) and not bool((good == 0.5).all())


@pytest.mark.parametrize("classes", [10, 26])
def test_plan_forced_exchange_steps_in_update_kernel(pg, gpu, monkeypatch, classes):  # noqa: F811
    """Forced exchange at world size 1, momentum + weight decay + nesterov, overlap on: no fc gradient, its
    bucket slot never allocated; the trajectory is the sequential twin's bit for bit."""
    from torch_distributed_sandbox_amd import models

    monkeypatch.setattr(models, "ConvNet", functools.partial(models.ConvNet, num_classes=classes))
    m1, m2, d1, d2, o1, o2 = _twins(gpu, grad_exchange="activations")
    fc, g = m1.fc.weight, torch.Generator(device=gpu).manual_seed(7)
    for step in range(3):
        x, y = _batch(gpu, g)
        _plan_step(d1, o1, x, y)
        o1.step()
        assert fc.grad is None and d1.grad_storage_bytes() < fc.numel() * 4, step
        _plan_step(d2, o2, x, y)
        o2.step()
    d1.wait_pending_updates()
    torch.cuda.synchronize()
    assert d1.exchanges[0].steps_exchanged == 3
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), n
        assert torch.equal(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"]), n
    _one_flat_buffer(o1, d1.flat_param, list(m1.parameters()))
    w0, b0 = fc.detach().clone(), o1.state[fc]["momentum_buffer"].clone()
    with d1.no_sync():
        _plan_step(d1, o1, *_batch(gpu, g))
    d1.wait_pending_updates()
    assert fc.grad is not None and torch.equal(fc, w0) and torch.equal(o1.state[fc]["momentum_buffer"], b0)
