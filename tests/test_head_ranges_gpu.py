"""The fused head in channel-range launches (kernels/head_pb.hip): ops.fused_head_forward_range over
channels [c0, c1) -- the grouped activation exchange's column groups -- and ops.fused_head_backward(...,
c_begin, c_end, finalize, g2m_out, partial_out) -- the K-chunked fc all-reduce's chunks.  A sequence of
range launches over a partition of [0, 32) must reproduce the whole launch bit for bit (the same
partial rows, the same finalizers), write nothing outside its own columns and planes, finish nothing
before its last launch, and match the fp64 chain BN2 -> ReLU -> pool -> fc within the bounds of
test_fused_gpu.py::test_head_forward_backward.  Then both forms end to end under DDP at an odd
pooled edge, with 3 groups / 3 chunks (parallel/factored.py column_groups, column_chunks)."""
import copy
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from test_fused_gpu import _check, _head_case, _ops, mag_floats, new_mag, set_ya_scale, ypart
from test_kernels_gpu import _close

pytestmark = pytest.mark.gpu

SENTINEL = 7.0

# partitions of [0, 32)
QUARTERS = ((0, 8), (8, 16), (16, 24), (24, 32))
UNEVEN = ((0, 11), (11, 21), (21, 32))  # round(i * 32 / 3): column_chunks' 3 chunks
SINGLES = ((0, 1), (1, 2), (2, 31), (31, 32))
ODD_A = ((0, 4), (4, 16), (16, 28), (28, 32))  # cuts at multiples of 4 channels: what an odd Q takes
ODD_B = ((0, 12), (12, 20), (20, 32))

# P = 38: Q = 19, odd, rows off the 16-B grid, 2 forward / 3 backward bands per channel; P = 64: Q = 32;
# P = 130: Q = 65, a partial 8-column block and a partial last band; P = 520 / 518: Q = 260 / 259, Q8 = 33,
# the second 32-block chunk of a block row and its idle lanes (B = 1: a 10 x 2.16 M weight)
FWD_CASES = [(P, B) for P in (38, 64, 130) for B in (1, 3, 8)] + [(520, 1), (518, 1)]
BWD_CASES = [(P, B) for P in (38, 64, 130) for B in (3, 8, 9)] + [(520, 1), (518, 1)]  # B = 9: two image passes


@pytest.fixture(autouse=True)
def _clean_counters(gpu):
    """A test that fails in the middle of a range sequence must not hand the tests after it a stale
    channels counter: opening a sequence (of any shape) resets the stream's counters."""
    yield
    _ops().head_forward_range_ws(torch.empty(1, 32, 32, device=gpu, dtype=torch.float16),
                                 torch.empty(1, 32 * 16, device=gpu), 8)


def _fwd_partitions(P):
    Q = P // 2
    if P >= 500:
        return (UNEVEN,) if Q % 2 == 0 else (ODD_B,)
    return (QUARTERS, UNEVEN, SINGLES) if Q % 2 == 0 else (ODD_A, ODD_B)


def _bwd_partitions(P):
    Q = P // 2
    if P >= 500:
        return (UNEVEN,)  # (the backward takes any range at any Q)
    return (QUARTERS, UNEVEN, SINGLES) if Q % 2 == 0 else (ODD_A, ODD_B, UNEVEN)


def _permuted(part):
    """Another launch order (completion is by count, not by position): odd positions, then even."""
    return part[1::2] + part[0::2]


@functools.lru_cache(maxsize=None)
def _case(gpu, P, B):
    """One head problem, its BN2 statistics / affine from the whole ops.fused_head_forward (as
    test_head_forward_backward builds them) and the fp64 chain BN2 -> ReLU -> pool -> fc with its
    gradients for a fixed dlogits.  Computed once per shape and left unchanged."""
    ops = _ops()
    y2, b2, g2, be2, wfc, bfc, partial2, ya = _head_case(gpu, P, B, 100 * P + B)
    Q, NC = P // 2, wfc.shape[0]
    _, stats2, aff2 = ops.fused_head_forward(ya, partial2, b2, g2, be2, None, None, None, 0.1, 1e-5, wfc, bfc, P)
    dl = torch.randn(B, NC, device=gpu)
    labels = torch.randint(0, NC, (B,), device=gpu)
    if B > 1:
        labels[1] = -100  # an ignored row
    yr = y2.permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    gr = g2.double().cpu().requires_grad_(True)
    ber = be2.double().cpu().requires_grad_(True)
    wr = wfc.double().cpu().requires_grad_(True)
    z = F.batch_norm(yr, None, None, gr, ber, True, 0.1, 1e-5)
    pz = F.max_pool2d(F.relu(z), 2, 2)
    pz.retain_grad()
    logits = F.linear(pz.reshape(B, -1), wr, bfc.double().cpu())
    logits.backward(dl.double().cpu())
    ref = {"logits": logits.detach(), "x": pz.detach().reshape(B, -1), "dW": wr.grad, "dg2": gr.grad,
           "dbe2": ber.grad, "g2m": pz.grad * (pz.detach() > 0).double()}
    return {"ya": ya, "b2": b2, "g2": g2, "wfc": wfc, "bfc": bfc, "stats2": stats2, "aff2": aff2, "dl": dl,
            "labels": labels, "Q": Q, "NC": NC, "ref": ref}


def _guarded(gpu, rows, cols, guard):
    """A [rows, cols] fp32 tensor of sentinels inside a larger buffer of sentinels (``guard``
    elements on either side, a multiple of 4: the view keeps the buffer's 16-B alignment)."""
    buf = torch.full((guard + rows * cols + guard,), SENTINEL, device=gpu)
    return buf, buf[guard:guard + rows * cols].view(rows, cols)


def _guards_kept(buf, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[buf.numel() - guard:] == SENTINEL).all())


def _new_ws(c, P):
    """A range sequence's workspace with sentinels in everything the last launch's finalizer writes."""
    ws = _ops().head_forward_range_ws(c["ya"], c["wfc"], P)
    for t in ws[1:]:
        t.fill_(SENTINEL)
    return ws


def _unfinished(ws):
    return all(bool((t == SENTINEL).all()) for t in ws[1:])


def _run_ranges(gpu, c, P, order, ws, mag, labels=None):
    """The range launches of ``order`` over ``ws``: every range's rows must come out as its columns
    of the whole launch's X, nothing may be written around them, and nothing is finished before the
    last launch.  Returns {(c0, c1): rows}."""
    ops = _ops()
    QQ = c["Q"] * c["Q"]
    B = c["ya"].shape[0]
    guard = (QQ + 3) // 4 * 4
    rows = {}
    for i, (c0, c1) in enumerate(order):
        buf, xg = _guarded(gpu, B, (c1 - c0) * QQ, guard)
        ops.fused_head_forward_range(c["ya"], c["aff2"], c["b2"], mag, c["wfc"], c["bfc"], P, c0, c1, *ws, labels, xg)
        assert _guards_kept(buf, guard), (c0, c1)
        if i < len(order) - 1:
            assert _unfinished(ws), f"finished after {order[:i + 1]}"
        rows[(c0, c1)] = xg
    return rows


def _whole_forward(gpu, c, P, mag, labels):
    """The whole launch: ops.fused_head_forward_aff(_ce) for the logits, X, the loss and dlogits;
    the fp64 sums, which those ops keep to themselves, from the same launch over a workspace of our
    own (fused_head_forward_range with [0, 32) is the whole launch)."""
    ops = _ops()
    B, K = c["ya"].shape[0], c["wfc"].shape[1]
    xw = torch.full((B, K), SENTINEL, device=gpu)
    logits = ops.fused_head_forward_aff(c["ya"], c["aff2"], c["b2"], mag, c["wfc"], c["bfc"], P, xw)
    ws = _new_ws(c, P)
    ops.fused_head_forward_range(c["ya"], c["aff2"], c["b2"], mag, c["wfc"], c["bfc"], P, 0, 32, *ws, labels, None)
    assert torch.equal(ws[2], logits)
    out = {"logits": logits, "x": xw, "sums": ws[1].clone()}
    if labels is not None:
        lg, loss, dlogits = ops.fused_head_forward_aff_ce(c["ya"], c["aff2"], c["b2"], mag, c["wfc"], c["bfc"], P,
                                                          labels)
        assert torch.equal(lg, logits) and torch.equal(ws[3], dlogits) and torch.equal(ws[4], loss)
        out.update(loss=loss, dlogits=dlogits)
    return out


def _same_as_whole(c, rows, ws, whole, labels):
    QQ = c["Q"] * c["Q"]
    for (c0, c1), xg in rows.items():
        assert torch.equal(xg, whole["x"][:, c0 * QQ:c1 * QQ]), (c0, c1)
    assert torch.equal(ws[2], whole["logits"]) and torch.equal(ws[1], whole["sums"])
    if labels is not None:
        assert torch.equal(ws[4], whole["loss"]) and torch.equal(ws[3], whole["dlogits"])


@pytest.mark.parametrize("P,B", FWD_CASES)
def test_forward_ranges_equal_the_whole_launch(gpu, P, B):
    ops = _ops()
    c = _case(gpu, P, B)
    mag = set_ya_scale(new_mag(gpu, B, P))
    labels = c["labels"]
    whole = _whole_forward(gpu, c, P, mag, labels)
    whole_nolab = _whole_forward(gpu, c, P, mag, None)
    assert torch.equal(whole_nolab["logits"], whole["logits"]) and torch.equal(whole_nolab["sums"], whole["sums"])
    # the whole launch against fp64, at test_head_forward_backward's bound
    _check(whole["logits"], c["ref"]["logits"], 1e-5, "logits (whole)")
    first = True
    for part in _fwd_partitions(P):
        for order in (part, _permuted(part)):
            for lab in ((None, labels) if first else (labels,)):
                ws = _new_ws(c, P)
                rows = _run_ranges(gpu, c, P, order, ws, mag, lab)
                _same_as_whole(c, rows, ws, whole, lab)
                if lab is None:  # no labels: the loss and dlogits are left alone
                    assert bool((ws[3] == SENTINEL).all()) and bool((ws[4] == SENTINEL).all())
            if first:
                first = False
                # against fp64: the logits and the concatenated rows at 1e-5, the loss and dlogits against
                # the cross-entropy of the kernel's own logits in fp64 at test_cross_entropy's 1e-6 / 1e-6
                _check(ws[2], c["ref"]["logits"], 1e-5, "logits")
                _check(torch.cat([rows[r] for r in sorted(rows)], dim=1), c["ref"]["x"], 1e-5, "X rows")
                zr = ws[2].double().cpu().requires_grad_(True)
                ce = F.cross_entropy(zr, labels.cpu())
                ce.backward()
                _close(ws[4], ce, 1e-6, 1e-6)
                _close(ws[3], zr.grad, 1e-6, 1e-6)
                # ... and bit for bit the separate CE launch on those logits
                loss2, dl2 = ops.cross_entropy(ws[2], labels, -100, 0.0)
                assert torch.equal(ws[4], loss2) and torch.equal(ws[3], dl2)


@pytest.mark.parametrize("P,B", [(38, 3), (64, 8)])
def test_forward_counters_reset(gpu, P, B):
    """The same sequence twice over one workspace (no new head_forward_range_ws in between: the
    finalizing launch itself leaves the counters at 0), then a whole launch: three equal results.
    The range launches also leave the whole launch's max |W| rows, from which the next head backward
    on the stream picks g2m's fp16 scales (kbuf[96:])."""
    c = _case(gpu, P, B)
    mag = set_ya_scale(new_mag(gpu, B, P))
    labels = c["labels"]
    whole = _whole_forward(gpu, c, P, mag, labels)
    part = _fwd_partitions(P)[0]

    def g2m_scales():  # kbuf[96:]: picked by the backward from the max |W| rows the last forward left
        return _ops().fused_head_backward(c["dl"], c["ya"], c["stats2"], c["aff2"], c["b2"], c["g2"], c["wfc"], P, None,
                                          1.0, False)[5][96:]

    scales = g2m_scales()
    _ops().fused_head_forward_aff(c["ya"], c["aff2"], c["b2"], mag, c["wfc"] * 64.0, c["bfc"], P)  # other maxima
    assert not torch.equal(g2m_scales(), scales)
    ws = _new_ws(c, P)
    for _ in range(2):
        for t in ws[1:]:
            t.fill_(SENTINEL)
        rows = _run_ranges(gpu, c, P, part, ws, mag, labels)
        _same_as_whole(c, rows, ws, whole, labels)
        assert torch.equal(g2m_scales(), scales)  # the range launches leave the whole launch's maxima
    again = _whole_forward(gpu, c, P, mag, labels)
    for k in whole:
        assert torch.equal(again[k], whole[k]), k


def test_forward_refusals_launch_nothing(gpu):
    """A refused range raises before any launch: an odd Q with a range off the multiples of 4
    channels, an empty or reversed range, a batch above one pass.  The sequence they interrupt still
    comes out bit for bit."""
    ops = _ops()
    P, B = 38, 3
    c = _case(gpu, P, B)
    QQ = c["Q"] * c["Q"]
    mag = set_ya_scale(new_mag(gpu, B, P))
    labels = c["labels"]
    whole = _whole_forward(gpu, c, P, mag, labels)
    # (before the sequence below is opened: head_forward_range_ws resets the stream's counters)
    c9 = _case(gpu, P, 9)  # two image passes: the range form has one
    ws9 = _new_ws(c9, P)
    with pytest.raises(RuntimeError):
        ops.fused_head_forward_range(c9["ya"], c9["aff2"], c9["b2"], None, c9["wfc"], c9["bfc"], P, 0, 4, *ws9, None,
                                     None)
    assert _unfinished(ws9)
    ws = _new_ws(c, P)
    rows = _run_ranges(gpu, c, P, ODD_A[:1], ws, mag, labels)
    for c0, c1 in ((2, 3), (4, 15), (3, 7), (5, 5), (6, 3), (28, 33), (-4, 4)):
        xg = torch.full((B, max(c1 - c0, 0) * QQ), SENTINEL, device=gpu)
        with pytest.raises(RuntimeError):
            ops.fused_head_forward_range(c["ya"], c["aff2"], c["b2"], mag, c["wfc"], c["bfc"], P, c0, c1, *ws, labels,
                                         xg)
        assert bool((xg == SENTINEL).all()) and _unfinished(ws), (c0, c1)
    rows.update(_run_ranges(gpu, c, P, ODD_A[1:], ws, mag, labels))
    _same_as_whole(c, rows, ws, whole, labels)


def test_forward_abandoned_sequence(gpu):
    """A sequence that stops after channels [0, 16) leaves the channels counter at 16; the next
    sequence opens with head_forward_range_ws, which resets the counters, and must come out as the
    whole launch (without the reset its logits would be finished after 16 channels)."""
    P, B = 64, 3
    c = _case(gpu, P, B)
    mag = set_ya_scale(new_mag(gpu, B, P))
    labels = c["labels"]
    whole = _whole_forward(gpu, c, P, mag, labels)
    ws = _new_ws(c, P)
    _run_ranges(gpu, c, P, ((0, 16),), ws, mag, labels)
    assert _unfinished(ws)
    ws = _new_ws(c, P)
    rows = _run_ranges(gpu, c, P, QUARTERS, ws, mag, labels)
    _same_as_whole(c, rows, ws, whole, labels)


def _bwd_mag(gpu, B, P):
    """The step's magnitude workspace as test_head_forward_backward prepares it: garbage, ya's
    scale, and one forward part that the finalize must reduce into mag[5]."""
    mag = set_ya_scale(new_mag(gpu, B, P))
    ypart(mag).zero_()
    ypart(mag)[5, 3] = torch.tensor(2.5).view(torch.int32)
    return mag


def _g2m_buffer(gpu, B, Q):
    """g2m [B, 32, Q, Q] fp16 of sentinels, with the slack the conv2 backward wants after it."""
    n = B * 32 * Q * Q
    return torch.full((n + 32,), SENTINEL, device=gpu, dtype=torch.float16)[:n].view(B, 32, Q, Q)


@pytest.mark.parametrize("P,B", BWD_CASES)
def test_backward_chunks_equal_the_whole_call(gpu, P, B):
    ops = _ops()
    c = _case(gpu, P, B)
    Q, NC, QQ = c["Q"], c["NC"], c["Q"] * c["Q"]
    ya, stats2, aff2, b2, g2, wfc, dl = (c[k] for k in ("ya", "stats2", "aff2", "b2", "g2", "wfc", "dl"))
    # the forward of this weight on this stream: it leaves max |W| per class and workgroup, from which
    # the backward picks g2m's fp16 scales
    ops.fused_head_forward_aff(ya, aff2, b2, None, wfc, c["bfc"], P)
    mag_w = _bwd_mag(gpu, B, P)
    # the whole call in its separate-finalize form (ypart_done=False): the chunks' finalizer
    dW, dbfc, dg2, dbe2, g2m, kbuf = ops.fused_head_backward(dl, ya, stats2, aff2, b2, g2, wfc, P, None, 1.0, True,
                                                             mag=mag_w, ypart_done=False)
    # against fp64, with the numbers of test_head_forward_backward
    ref = c["ref"]
    _check(dW, ref["dW"], 1e-5, "dW")
    _check(dbfc, dl.double().sum(0), 1e-6, "dbfc")
    _check(dg2, ref["dg2"], 1e-5, "dgamma2")
    _check(dbe2, ref["dbe2"], 1e-5, "dbeta2")
    g2f = g2m.float() * kbuf[96:].view(1, 32, 1, 1)
    _check(g2f, ref["g2m"].view(B, 32, Q, Q), 2.0 ** -11 + 1e-5, "g2m (fp16, 2^-11 relative)")
    nrow = ops.head_bwd_workspace(B, P) - 16  # doubles of the BN2 partial rows, [32][npass * nblk][4]
    for part in _bwd_partitions(P):
        dw_o = torch.full_like(wfc, SENTINEL)
        g2m_o = _g2m_buffer(gpu, B, Q)
        part_o = torch.full((nrow + 16,), SENTINEL, device=gpu, dtype=torch.float64)
        part_0 = part_o.clone()
        rows_v = part_o[:nrow].view(32, -1)  # a channel's partial rows
        tail_v = part_o[nrow:].view(torch.float32)  # g2m's per-channel scales on their way to kbuf[96:]
        rows_0, tail_0 = part_0[:nrow].view(32, -1), part_0[nrow:].view(torch.float32)
        mag_c = _bwd_mag(gpu, B, P)
        done = []  # (c0, c1, the chunk's columns / planes / rows / scales right after its call)
        for i, (c0, c1) in enumerate(part):
            last = i == len(part) - 1
            res = ops.fused_head_backward(dl, ya, stats2, aff2, b2, g2, wfc, P, dw_o, 1.0, True, 0.0, None, None, None,
                                          True, c0, c1, last, g2m_o, part_o, mag_c)
            assert res[0].data_ptr() == dw_o.data_ptr() and res[4].data_ptr() == g2m_o.data_ptr()
            if not last:  # nothing is finalized before the last call
                assert all(res[k].numel() == 0 for k in (1, 2, 3, 5)), (c0, c1)
            done.append((c0, c1, dw_o[:, c0 * QQ:c1 * QQ].clone(), g2m_o[:, c0:c1].clone(), rows_v[c0:c1].clone(),
                         tail_v[c0:c1].clone()))
            ran = torch.zeros(32, dtype=torch.bool, device=gpu)
            for a, e, dw_s, g_s, r_s, t_s in done:  # the chunks already run: unchanged
                ran[a:e] = True
                assert torch.equal(dw_o[:, a * QQ:e * QQ], dw_s) and torch.equal(g2m_o[:, a:e], g_s), (c0, c1, a, e)
                assert torch.equal(rows_v[a:e], r_s) and torch.equal(tail_v[a:e], t_s), (c0, c1, a, e)
            # the chunks not yet run: their columns, planes, partial rows and scales untouched
            assert bool((dw_o.view(NC, 32, QQ)[:, ~ran] == SENTINEL).all()), (c0, c1)
            assert bool((g2m_o[:, ~ran] == SENTINEL).all()), (c0, c1)
            assert torch.equal(rows_v[~ran], rows_0[~ran]) and torch.equal(tail_v[~ran], tail_0[~ran]), (c0, c1)
        _, dbfc_c, dg2_c, dbe2_c, g2m_c, kbuf_c = res
        assert torch.equal(dw_o, dW), part
        assert torch.equal(g2m_c, g2m), part
        assert torch.equal(dbfc_c, dbfc) and torch.equal(dg2_c, dg2) and torch.equal(dbe2_c, dbe2), part
        assert kbuf_c.shape == (128,) and torch.equal(kbuf_c, kbuf), part  # (kbuf[96:]: from the workspace tail)
        assert torch.equal(kbuf_c[96:], tail_v), part
        assert torch.equal(mag_c[:33], mag_w[:33]), part  # max |y2 - b2| per channel and max |g2m|
        want = torch.zeros(32, device=gpu)
        want[5] = 2.5
        assert torch.equal(mag_floats(mag_c)[:32], want)


def test_backward_chunk_refusals(gpu):
    """A channel chunk writes into the caller's dw_out / g2m_out / partial_out, and the fused SGD
    step runs on the whole weight only: anything else raises, before a launch."""
    ops = _ops()
    P, B = 38, 3
    c = _case(gpu, P, B)
    Q = c["Q"]
    ya, stats2, aff2, b2, g2, dl = (c[k] for k in ("ya", "stats2", "aff2", "b2", "g2", "dl"))
    wfc = c["wfc"].clone()
    w0 = wfc.clone()
    ops.fused_head_forward_aff(ya, aff2, b2, None, wfc, c["bfc"], P)

    def bufs():
        return (torch.full_like(wfc, SENTINEL), _g2m_buffer(gpu, B, Q),
                torch.full((ops.head_bwd_workspace(B, P),), SENTINEL, device=gpu, dtype=torch.float64))

    def call(dw_o, g2m_o, part_o, lr=0.0, c0=0, c1=11):
        return ops.fused_head_backward(dl, ya, stats2, aff2, b2, g2, wfc, P, dw_o, 1.0, True, lr, None, None, None,
                                       True, c0, c1, False, g2m_o, part_o, None)

    for drop, lr, rng in ((None, 0.5, (0, 11)), (0, 0.0, (0, 11)), (1, 0.0, (0, 11)), (2, 0.0, (0, 11)),
                          (None, 0.0, (11, 11)), (None, 0.0, (21, 33))):
        b = list(bufs())
        keep = [t.clone() for t in b]
        args = [None if k == drop else t for k, t in enumerate(b)]
        with pytest.raises(RuntimeError):
            call(*args, lr=lr, c0=rng[0], c1=rng[1])
        assert all(torch.equal(t, k) for t, k in zip(b, keep)), (drop, lr, rng)
        assert torch.equal(wfc, w0), (drop, lr, rng)
    res = call(*bufs())  # the call they all vary is a good one
    assert res[1].numel() == 0


# ---------------------------------------------------------------- end to end, world 1 forced (rccl-native)
@pytest.fixture(scope="module")
def pg(gpu):
    from torch_distributed_sandbox_amd.parallel import distributed as dist
    from torch_distributed_sandbox_amd.parallel import launch

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = launch.find_free_port()
    dist.init_process_group("rccl-native", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


@pytest.mark.parametrize("kw,ranges", [
    (dict(grad_exchange="activations", exchange_source="rows", exchange_groups=3), 3),
    (dict(grad_exchange="chunked", allreduce_chunks=3), 0),
])
def test_three_ranges_end_to_end_at_odd_q(pg, gpu, kw, ranges):
    """H = 260 (Q = 65, odd) with 3 column groups of the zero-suppressed activation exchange (the
    head forward in range launches; plain thirds (0,11),(11,21),(21,32) are ranges the launch refuses
    at an odd Q: column_groups cuts at multiples of 4 channels there) and with 3 chunks of the
    K-chunked all-reduce (the head backward in chunks, which takes the plain thirds): the gradients
    of the plain fused model, at test_comm_gpu.py::test_activation_exchange_fused_convnet's bound."""
    from torch_distributed_sandbox_amd.models import ConvNet, convnet_fused
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    H, B = 260, 3
    m = ConvNet(image_shape=(H, H), device=gpu, mode="fused")
    ref = copy.deepcopy(m)
    ddp = DistributedDataParallel(m, **kw)
    assert len(ddp.exchanges) == 1
    ex = ddp.exchanges[0]
    QQ = (H // 4) ** 2
    if ranges:
        groups = ex.column_groups(32 * QQ, planes=32)
        assert len(groups) == ranges and all(k0 % (4 * QQ) == 0 and k1 % (4 * QQ) == 0 for k0, k1 in groups)
    else:
        assert ex.column_chunks(32 * QQ, planes=32) == [(a * QQ, e * QQ) for a, e in UNEVEN]
    opt = ddp.attach_optimizer(SGD(m.parameters(), 0.01))
    x = torch.rand(B, 1, H, H, device=gpu)
    y = torch.tensor([1, 2, 3], device=gpu)
    for step in range(2):
        before = convnet_fused.STATS["head_range_launches"]
        loss = CrossEntropyLoss()(ddp(x), y)
        assert convnet_fused.STATS["head_range_launches"] == before + ranges
        opt.zero_grad()
        loss.backward()
        ref.zero_grad()
        CrossEntropyLoss()(ref(x), y).backward()
        for (n, p), q in zip(m.named_parameters(), ref.parameters()):
            if n.endswith("0.bias"):
                continue
            rel = ((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30)).item()
            assert rel < 1e-5, (step, n, rel)
        opt.step()
        with torch.no_grad():
            for p, q in zip(m.parameters(), ref.parameters()):
                q.copy_(p)
    assert ex.steps_exchanged == 2
    if ranges:
        assert ddp.fc_grad_path() == "activation-exchange(zs)"
