"""SGD with momentum / weight decay on the fast paths: the head backward's in-kernel momentum step
(kernels/head_pb.hip MOM), the flat sweep's 16-byte momentum path (kernels/elementwise.hip), and the
plan under DistributedDataParallel(overlap_optimizer=True) with ops.optim.SGD's flat momentum buffer.

Reference for the update arithmetic: torch's rule

    d = g + wd w;  b' = first ? d : mom b + (1 - damp) d;  d = nesterov ? d + mom b' : b';  w' = w - lr d

in fp64 on the fp32 values the kernel gets: w, b, the fp32 gradient g (for the head kernel the dW the
same kernel stores with keep_dw=True) and the hyperparameters as the op rounds them to fp32.  Per
element the kernels may differ from it by K * 2^-24 * S, S the sum of the absolute values of the
terms entering b' (w'), K the number of fp32 roundings of the kernels' chain (common.h
sgd_rule_step, one fused multiply-add per line there), counted in _rule_ref beside each line.
"""
import copy
import os

import numpy as np
import pytest
import torch

from test_fused_gpu import _head_case, _ops
from test_head_ranges_gpu import SENTINEL, _guarded, _guards_kept

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24

# (momentum, weight_decay, dampening, nesterov): the term each flag carries is >= 100 x the bound on
# the median element for the data below (asserted by _margins on the steps where the flag acts)
HP_SETS = {
    "mom": (0.9, 0.0, 0.0, False),
    "mom_wd": (0.9, 0.05, 0.0, False),
    "mom_damp": (0.9, 0.0, 0.25, False),
    "nesterov_wd": (0.9, 0.05, 0.0, True),
}


def _f32(v):
    return float(np.float32(v))


def _rule_ref(w, g, b, lr, hp, first):
    """fp64 rule on fp32 tensors -> (b', w', bound on b', bound on w', {flag: its term in w'})."""
    mom, wd, damp, nest = hp
    lr, mom, wd, damp = _f32(lr), _f32(mom), _f32(wd), _f32(damp)
    w, g = w.double(), g.double()
    d = g + wd * w
    s_d = g.abs() + (wd * w).abs()
    k_d = 1 if wd != 0.0 else 0              # (1) d = fma(wd, w, g)
    if first:
        bn, s_b, k_b = d, s_d, k_d           # b' = d: no further rounding
    else:
        b = b.double()
        bn = mom * b + (1.0 - damp) * d
        s_b = (mom * b).abs() + (1.0 - damp) * s_d
        # (3) fma(mom, b, omd d); with dampening also omd = 1.f - damp and (2) omd * d (without: omd is
        # exactly 1 and the product exact)
        k_b = k_d + (3 if damp != 0.0 else 1)
    if nest:
        dn = d + mom * bn
        s_n = s_d + mom * s_b
        k_n = k_b + 1                        # (4) fma(mom, b', d)
    else:
        dn, s_n, k_n = bn, s_b, k_b
    wn = w - lr * dn
    s_w = w.abs() + lr * s_n
    k_w = k_n + 1                            # (5) fma(-lr, d, w)
    assert k_w <= 8
    terms = {"momentum": None if first and not nest else lr * mom * ((bn if nest else b).abs()),
             "weight_decay": lr * (wd * w).abs() if wd != 0.0 else None,
             "dampening": lr * damp * d.abs() if damp != 0.0 and not first else None,
             "nesterov": lr * mom * bn.abs() if nest else None}
    return bn, wn, k_b * EPS * s_b, k_w * EPS * s_w, terms


def _margins(terms, bound_w, where):
    """Every flag's term in w' is >= 100 x the bound on the median element: a dropped flag fails."""
    med_bound = bound_w.median().item()
    for flag, t in terms.items():
        if t is not None:
            assert t.median().item() >= 100.0 * med_bound, (where, flag, t.median().item(), med_bound)


def _within(got, ref, bound, where):
    err = (got.double() - ref).abs()
    worst = (err - bound).max().item()
    assert worst <= 0.0, (where, "worst excess", worst, "max err", err.max().item(), "max bound", bound.max().item())


# ---------------------------------------------------------------- head backward kernel
def _head_setup(gpu, P, B):
    ops = _ops()
    y2, b2, g2, be2, wfc, bfc, partial2, ya = _head_case(gpu, P, B, 7 * P + B)
    _, stats2, aff2 = ops.fused_head_forward(ya, partial2, b2, g2, be2, None, None, None, 0.1, 1e-5, wfc, bfc, P)
    dl = torch.randn(B, wfc.shape[0], device=gpu)
    return {"ya": ya, "b2": b2, "g2": g2, "wfc": wfc, "bfc": bfc, "stats2": stats2, "aff2": aff2, "dl": dl}


_HEAD = {}


def _head(gpu, P, B):
    if (P, B) not in _HEAD:
        _HEAD[(P, B)] = _head_setup(gpu, P, B)
    return _HEAD[(P, B)]


GUARD = 64
LR_HEAD = 0.01


@pytest.mark.parametrize("hp", list(HP_SETS))
@pytest.mark.parametrize("P,B", [(38, 3), (38, 8), (130, 3), (130, 8)])
def test_head_backward_momentum_step(gpu, P, B, hp):
    """Two consecutive in-kernel momentum steps (the first creates the buffer, pre-filled with a
    sentinel it must ignore), with keep_dw True and False, weight and buffer in guarded allocations."""
    ops = _ops()
    c = _head(gpu, P, B)
    mom, wd, damp, nest = HP_SETS[hp]
    ya, stats2, aff2, b2, g2, dl = (c[k] for k in ("ya", "stats2", "aff2", "b2", "g2", "dl"))
    NC, K = c["wfc"].shape
    w_cur, b_cur = c["wfc"].clone(), torch.full_like(c["wfc"], SENTINEL)
    for step in range(2):
        first = step == 0
        where = (P, B, hp, step)
        ops.fused_head_forward_aff(ya, aff2, b2, None, w_cur, c["bfc"], P)  # (the backward's g2m scale: this weight's maxima)
        # no update at all: dW stored, everything else as the momentum calls must leave it
        plain = ops.fused_head_backward(dl, ya, stats2, aff2, b2, g2, w_cur.clone(), P, None, 1.0, True)
        dWp = plain[0]
        b_ref, w_ref, bound_b, bound_w, terms = _rule_ref(w_cur, dWp, b_cur, LR_HEAD, HP_SETS[hp], first)
        _margins(terms, bound_w, where)
        got = {}
        for keep in (True, False):
            wbuf, w = _guarded(gpu, NC, K, GUARD)
            bbuf, b = _guarded(gpu, NC, K, GUARD)
            w.copy_(w_cur)
            b.copy_(b_cur)
            res = ops.fused_head_backward(dl, ya, stats2, aff2, b2, g2, w, P, None, 1.0, True, LR_HEAD, None, None,
                                          None, keep, 0, 32, True, None, None, None, False, b, wd, mom, damp, nest,
                                          first)
            assert _guards_kept(wbuf, GUARD) and _guards_kept(bbuf, GUARD), (where, keep)
            _within(b, b_ref, bound_b, where + (keep, "buf"))
            _within(w, w_ref, bound_w, where + (keep, "w"))
            if keep:
                assert torch.equal(res[0], dWp), where  # the stored dW: the plain call's
            else:
                assert res[0] is None or res[0].numel() == 0, where
            for i in (1, 2, 3, 4, 5):  # dbfc, dgamma2, dbeta2, g2m, kbuf
                assert torch.equal(res[i], plain[i]), (where, keep, i)
            got[keep] = (w.clone(), b.clone())
        assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1]), where
        w_cur, b_cur = got[True]


def test_head_backward_momentum_refusals(gpu):
    """What the op refuses with a buffer, before any launch: weight and buffer stay as they were."""
    ops = _ops()
    P = 38
    c = _head(gpu, P, 3)
    c9 = _head(gpu, P, 9)
    NC, K = c["wfc"].shape

    def call(c, w, buf, lr=0.01, c0=0, c1=32, finalize=True, mom=0.9, g2m_o=None, part_o=None):
        return ops.fused_head_backward(c["dl"], c["ya"], c["stats2"], c["aff2"], c["b2"], c["g2"], w, P, None, 1.0, True,
                                       lr, None, None, None, True, c0, c1, finalize, g2m_o, part_o, None, False, buf,
                                       0.0, mom, 0.0, False, False)

    w = c["wfc"].clone()
    ops.fused_head_forward_aff(c["ya"], c["aff2"], c["b2"], None, w, c["bfc"], P)
    good = torch.full_like(w, 0.5)
    Q = P // 2
    g2m_o = torch.empty(3 * 32 * Q * Q + 32, device=gpu, dtype=torch.float16)[:3 * 32 * Q * Q].view(3, 32, Q, Q)
    part_o = torch.empty(ops.head_bwd_workspace(3, P), device=gpu, dtype=torch.float64)
    bad = {
        "shape": dict(buf=torch.full((NC, K + 4), 0.5, device=gpu)),
        "dtype": dict(buf=torch.full((NC, K), 0.5, device=gpu, dtype=torch.float64)),
        "device": dict(buf=torch.full((NC, K), 0.5)),
        "alias": dict(buf=w),
        "no update_lr": dict(buf=good, lr=0.0),
        "momentum without a buffer": dict(buf=None),
        "chunk": dict(buf=good, c0=0, c1=11, finalize=False, g2m_o=g2m_o, part_o=part_o),
    }
    w0 = w.clone()
    for name, kw in bad.items():
        with pytest.raises(RuntimeError):
            call(c, w, **kw)
        assert torch.equal(w, w0), name
        assert bool((good == 0.5).all()), name
        if kw.get("buf") is not None and kw["buf"] is not w:
            assert bool((kw["buf"] == 0.5).all()), name
    # two image passes (B = 9) with a buffer
    w9 = c9["wfc"].clone()
    ops.fused_head_forward_aff(c9["ya"], c9["aff2"], c9["b2"], None, w9, c9["bfc"], P)
    w90 = w9.clone()
    with pytest.raises(RuntimeError):
        call(c9, w9, good)
    assert torch.equal(w9, w90) and bool((good == 0.5).all())
    ops.fused_head_forward_aff(c["ya"], c["aff2"], c["b2"], None, w, c["bfc"], P)
    call(c, w, good)  # the call they all vary is a good one
    assert not torch.equal(w, w0) and not bool((good == 0.5).all())


# ---------------------------------------------------------------- flat sweep
LR_FLAT = 0.125  # a power of two: lr * g is exact, so fma(-lr, g, p) and torch's p - lr * g agree bit for bit


def _one_flat_buffer(opt, flat_param, params):
    """state[p]["momentum_buffer"] of every parameter: views of one buffer, laid out like flat_param."""
    mbs = [opt.state[p]["momentum_buffer"] for p in params]
    base = mbs[0].untyped_storage().data_ptr()
    for p, mb in zip(params, mbs):
        assert mb.shape == p.shape and mb.untyped_storage().data_ptr() == base
        assert mb.data_ptr() - base == p.data_ptr() - flat_param.data_ptr()


def _flat_tensors(gpu, seed):
    """Tensors of 7, 33, 1000 and 4099 elements at 16-byte-aligned addresses, and a 1000-element
    view starting one element into an allocation (the scalar loop)."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    sizes = (7, 33, 1000, 4099)
    ts = [torch.randn(n, device=gpu, generator=g) for n in sizes]
    ts.append(torch.randn(1001, device=gpu, generator=g)[1:])
    assert all(t.data_ptr() % 16 == 0 for t in ts[:-1]) and ts[-1].data_ptr() % 16 == 4
    return ts


@pytest.mark.parametrize("hp", list(HP_SETS))
def test_flat_sweep_momentum(gpu, hp):
    ops = _ops()
    mom, wd, damp, nest = HP_SETS[hp]
    ps = _flat_tensors(gpu, 1)
    bs = [torch.full_like(p, SENTINEL) for p in ps[:-1]] + [torch.full((1001,), SENTINEL, device=gpu)[1:]]
    for step in range(2):
        first = step == 0
        gs = _flat_tensors(gpu, 10 + step)
        refs = [_rule_ref(p, g, b, LR_FLAT, HP_SETS[hp], first) for p, g, b in zip(ps, gs, bs)]
        ops.sgd_step_(ps, gs, bs, LR_FLAT, wd, mom, damp, nest, first)
        for i, (p, b, (b_ref, w_ref, bound_b, bound_w, terms)) in enumerate(zip(ps, bs, refs)):
            if p.numel() >= 1000:
                _margins(terms, bound_w, (hp, step, i))
            _within(b, b_ref, bound_b, (hp, step, i, "buf"))
            _within(p, w_ref, bound_w, (hp, step, i, "w"))


def test_flat_sweep_weight_decay_only_and_plain(gpu):
    """Weight decay without momentum (no buffer) takes the 16-byte path too; the plain step on the
    same inputs is p - lr * g bit for bit, as test_kernels_gpu.py::test_sgd forms it.

    What the bit comparison shows and what it does not: the kernel's plain step is one fused
    multiply-add, torch's p - lr * g rounds twice, so the two agree in every bit only where lr * g is
    exact -- hence lr = 2^-3 here, not test_sgd's 0.1, at which the last bit may differ (and differed
    before this path existed).  The check catches anything leaking into the plain step (weight decay,
    a buffer, another operand order); it does not show "the same bits as before" at a general lr.
    That evidence is the benchmark's dumped outputs after 25 plain steps at lr = 1e-4, bit-identical
    to the parent commit's (profiles/momentum_fused_ab.md), and the unchanged plain 16-byte code."""
    ops = _ops()
    ps, gs = _flat_tensors(gpu, 1), _flat_tensors(gpu, 10)
    refs = [_rule_ref(p, g, None, LR_FLAT, (0.0, 0.05, 0.0, False), True) for p, g in zip(ps, gs)]
    ops.sgd_step_(ps, gs, [], LR_FLAT, 0.05, 0.0, 0.0, False, False)
    for i, (p, (_, w_ref, _, bound_w, terms)) in enumerate(zip(ps, refs)):
        _within(p, w_ref, bound_w, ("wd only", i))
    ps = _flat_tensors(gpu, 1)
    ref = [p - LR_FLAT * g for p, g in zip(ps, gs)]
    ops.sgd_step_(ps, gs, [], LR_FLAT, 0.0, 0.0, 0.0, False, False)
    for p, r in zip(ps, ref):
        assert torch.equal(p, r)


# ---------------------------------------------------------------- the plan, world size 1
H_PLAN, B_PLAN, LR_PLAN = 256, 3, 1e-2
PLAN_HP = dict(momentum=0.9, weight_decay=1e-4, nesterov=True)


def _twins(gpu, keep=False, **ddp_kw):
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    m1 = ConvNet(image_shape=(H_PLAN, H_PLAN), device=gpu, mode="fused")
    m2 = copy.deepcopy(m1)
    d1 = DistributedDataParallel(m1, overlap_optimizer=True, keep_fused_grads=keep, **ddp_kw)
    d2 = DistributedDataParallel(m2, fuse_update_in_backward=False, **ddp_kw)
    assert d1.overlap_optimizer and len(d1._deferred) == 1 and not d2._deferred
    o1 = d1.attach_optimizer(SGD(m1.parameters(), LR_PLAN, **PLAN_HP))
    o2 = d2.attach_optimizer(SGD(m2.parameters(), LR_PLAN, **PLAN_HP))
    return m1, m2, d1, d2, o1, o2


def _batch(gpu, g):
    x = torch.rand(B_PLAN, 1, H_PLAN, H_PLAN, device=gpu, generator=g)
    y = torch.randint(0, 10, (B_PLAN,), device=gpu, generator=g)
    return x, y


def _plan_step(d, o, x, y):
    from torch_distributed_sandbox_amd.ops import CrossEntropyLoss

    loss = CrossEntropyLoss()(d(x), y)
    o.zero_grad()
    loss.backward()
    return loss


def _check_plan_step(m1, m2, o1, o2, w0, b0, first, where):
    """After both twins stepped: the fc weight and its buffer within the bound of the fp64 rule on
    the twin's dW, everything else bit for bit."""
    hp = (PLAN_HP["momentum"], PLAN_HP["weight_decay"], 0.0, PLAN_HP["nesterov"])
    dW = m2.fc.weight.grad
    b_ref, w_ref, bound_b, bound_w, terms = _rule_ref(w0, dW, b0, LR_PLAN, hp, first)
    _within(o1.state[m1.fc.weight]["momentum_buffer"], b_ref, bound_b, where + ("fc buf",))
    _within(m1.fc.weight, w_ref, bound_w, where + ("fc w",))
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        if n == "fc.weight":
            continue
        assert torch.equal(p, q), where + (n,)
        assert torch.equal(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"]), where + (n, "buf")


def test_plan_momentum_in_head_backward(gpu):
    """DDP(overlap_optimizer=True) with momentum, weight decay and nesterov at world size 1: the fc
    weight's step runs inside the head backward with no gradient materialised; three single-step
    comparisons against an unfused, non-overlapped twin."""
    m1, m2, d1, d2, o1, o2 = _twins(gpu)
    g = torch.Generator(device=gpu).manual_seed(5)
    fc_bytes = m1.fc.weight.numel() * 4
    for step in range(3):
        x, y = _batch(gpu, g)
        w0 = m1.fc.weight.detach().clone()
        b0 = None if step == 0 else o1.state[m1.fc.weight]["momentum_buffer"].clone()
        _plan_step(d1, o1, x, y)
        assert m1.fc.weight.grad is None, step
        assert not torch.equal(m1.fc.weight, w0), step  # stepped inside the backward
        _plan_step(d2, o2, x, y)
        assert torch.equal(m2.fc.weight, w0), step
        o1.step()
        o2.step()
        assert d1.last_deferred_inline, step
        assert d1.grad_storage_bytes() < fc_bytes, step
        _one_flat_buffer(o1, d1.flat_param, list(m1.parameters()))  # torch's state layout, as views
        _check_plan_step(m1, m2, o1, o2, w0, b0, step == 0, (step,))
        with torch.no_grad():  # every step a single-step comparison
            for p, q in zip(m1.parameters(), m2.parameters()):
                p.copy_(q)
                o1.state[p]["momentum_buffer"].copy_(o2.state[q]["momentum_buffer"])
            for a, b in zip(m1.buffers(), m2.buffers()):
                a.copy_(b)
    # no_sync(): the gradient is materialised, the in-kernel step skipped
    x, y = _batch(gpu, g)
    w0 = m1.fc.weight.detach().clone()
    b0 = o1.state[m1.fc.weight]["momentum_buffer"].clone()
    with d1.no_sync():
        _plan_step(d1, o1, x, y)
    _plan_step(d2, o2, x, y)
    assert m1.fc.weight.grad is not None and torch.equal(m1.fc.weight.grad, m2.fc.weight.grad)
    assert torch.equal(m1.fc.weight, w0) and torch.equal(o1.state[m1.fc.weight]["momentum_buffer"], b0)


def test_plan_momentum_keep_fused_grads(gpu):
    m1, m2, d1, d2, o1, o2 = _twins(gpu, keep=True)
    g = torch.Generator(device=gpu).manual_seed(6)
    x, y = _batch(gpu, g)
    w0 = m1.fc.weight.detach().clone()
    _plan_step(d1, o1, x, y)
    _plan_step(d2, o2, x, y)
    assert torch.equal(m1.fc.weight.grad, m2.fc.weight.grad)  # also written, by the same arithmetic
    assert not torch.equal(m1.fc.weight, w0)
    o1.step()
    o2.step()
    _check_plan_step(m1, m2, o1, o2, w0, None, True, ("keep",))


# ---------------------------------------------------------------- forced exchange at world size 1
@pytest.fixture(scope="module")
def pg(gpu):
    from torch_distributed_sandbox_amd.parallel import distributed as dist
    from torch_distributed_sandbox_amd.parallel import launch

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = launch.find_free_port()
    dist.init_process_group("rccl-native", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


def test_forced_exchange_momentum_matches_sequential(pg, gpu):
    """grad_exchange="activations" forced at world size 1, overlap on, with momentum: the exchange
    writes dW to the bucket (its in-place step is plain-SGD only), the deferred runner applies the
    momentum step on the side stream and fences the parameters; the trajectory is the sequential
    twin's bit for bit."""
    from torch_distributed_sandbox_amd.ops import param_fence

    m1, m2, d1, d2, o1, o2 = _twins(gpu, grad_exchange="activations")
    assert len(d1.exchanges) == 1
    g = torch.Generator(device=gpu).manual_seed(7)
    for step in range(3):
        x, y = _batch(gpu, g)
        for d, o in ((d1, o1), (d2, o2)):
            _plan_step(d, o, x, y)
            o.step()
        assert param_fence.pending(m1.fc.weight) and not d1.last_deferred_inline, step
    d1.wait_pending_updates()
    torch.cuda.synchronize()
    assert d1.exchanges[0].steps_exchanged == 3
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), n
        assert torch.equal(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"]), n


# ---------------------------------------------------------------- checkpoint
def test_checkpoint_carries_momentum(gpu, tmp_path):
    """Two steps, save; a fresh model / wrapper / optimizer loads and takes the third step: the
    uninterrupted run's parameters and buffers bit for bit, the loaded buffers views of the flat one."""
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel
    from torch_distributed_sandbox_amd.utils import checkpoint

    def fresh(seed):
        torch.manual_seed(seed)
        m = ConvNet(image_shape=(H_PLAN, H_PLAN), device=gpu, mode="fused")
        d = DistributedDataParallel(m, overlap_optimizer=True)
        return m, d, d.attach_optimizer(SGD(m.parameters(), LR_PLAN, **PLAN_HP))

    g = torch.Generator(device=gpu).manual_seed(8)
    batches = [_batch(gpu, g) for _ in range(3)]
    m1, d1, o1 = fresh(0)
    for x, y in batches[:2]:
        _plan_step(d1, o1, x, y)
        o1.step()
    path = str(tmp_path / "ck.pt")
    checkpoint.save(path, d1, o1, step=2)
    m2, d2, o2 = fresh(1)
    checkpoint.load(path, d2, o2, map_location=gpu)
    _one_flat_buffer(o2, d2.flat_param, list(m2.parameters()))
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(o2.state[q]["momentum_buffer"], o1.state[p]["momentum_buffer"])
    for d, o in ((d1, o1), (d2, o2)):
        _plan_step(d, o, *batches[2])
        o.step()
    assert m2.fc.weight.grad is None and d2.last_deferred_inline
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), n
        assert torch.equal(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"]), n


# ---------------------------------------------------------------- two gloo ranks sharing cuda:0
MR_B, MR_STEPS = 2, 2


def _mr_worker(rank, world, port, overlap, out):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    m = ConvNet(image_shape=(H_PLAN, H_PLAN), device=dev, mode="fused")
    ddp = DistributedDataParallel(m, grad_exchange="allreduce", overlap_optimizer=overlap)
    opt = ddp.attach_optimizer(SGD(m.parameters(), LR_PLAN, **PLAN_HP))
    g = torch.Generator().manual_seed(21)
    xs = torch.rand(MR_STEPS, world, MR_B, 1, H_PLAN, H_PLAN, generator=g)
    ys = torch.randint(0, 10, (MR_STEPS, world, MR_B), generator=g)
    for s in range(MR_STEPS):
        loss = CrossEntropyLoss()(ddp(xs[s, rank].to(dev)), ys[s, rank].to(dev))
        opt.zero_grad()
        loss.backward()
        opt.step()
    ddp.wait_pending_updates()
    torch.cuda.synchronize()
    rec = {"params": {n: p.detach().cpu().clone() for n, p in m.named_parameters()},
           "bufs": {n: opt.state[p]["momentum_buffer"].detach().cpu().clone() for n, p in m.named_parameters()},
           "fc_grad": ddp.fc_grad_path()}
    torch.save(rec, os.path.join(out, f"o{int(overlap)}_r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_momentum_overlap_matches_sequential(gpu, tmp_path):
    """With momentum the overlapped optimizer's runner (collective waited for on the side stream,
    then the momentum step of parameter, gradient and buffer slices) leaves what the sequential
    step leaves, bit for bit, on both ranks."""
    from torch_distributed_sandbox_amd.parallel import launch

    world = 2
    for overlap in (True, False):
        launch.spawn(_mr_worker, args=(world, launch.find_free_port(), overlap, str(tmp_path)), nprocs=world,
                     timeout=240)
    recs = {(o, r): torch.load(tmp_path / f"o{o}_r{r}.pt", weights_only=True) for o in (0, 1) for r in range(world)}
    assert recs[(1, 0)]["fc_grad"] == "allreduce"
    for r in range(world):
        for kind in ("params", "bufs"):
            for n, t in recs[(1, r)][kind].items():
                assert torch.equal(t, recs[(0, r)][kind][n]), (r, kind, n)
                assert torch.equal(t, recs[(1, 0)][kind][n]), (r, kind, n)
