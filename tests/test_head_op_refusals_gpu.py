"""The argument checks of the fused head's ops (csrc/fused_ops.cpp): the four forwards, the two pooled
updates and the backward.  Each case passes one bad argument to an otherwise good call at the smallest
shape the ops take (P = 8: Q = 4; B = 1, or B = 9 where the refusal is "at most 8 images"; NC = 2),
expects a RuntimeError, and then finds every buffer the op could have written -- fc.weight, out / dw_out,
x_out, the momentum buffer, the workspaces -- bit for bit as it was: the check came before any launch
or memset.  The call each group of cases varies is run at the end and does write.

Not repeated here: the channel ranges and the batch of the range forward
(test_head_ranges_gpu.py::test_forward_refusals_launch_nothing), the backward's chunk arguments
(::test_backward_chunk_refusals), the momentum buffer's shape / dtype / device and its chunked call
(test_sgd_momentum_gpu.py::test_head_backward_momentum_refusals)."""
import functools

import pytest
import torch

from test_fused_gpu import _head_case, _ops
from test_head_ranges_gpu import SENTINEL

pytestmark = pytest.mark.gpu

P, Q, NC = 8, 4, 2
QQ = Q * Q
K = 32 * QQ
W = 2  # ranks of the pooled updates


@functools.lru_cache(maxsize=None)
def _case(gpu, B):
    ops = _ops()
    y2, b2, g2, be2, wfc, bfc, partial2, ya = _head_case(gpu, P, B, 8000 + B)
    wfc, bfc = wfc[:NC].contiguous(), bfc[:NC].contiguous()
    _, stats2, aff2 = ops.fused_head_forward(ya, partial2, b2, g2, be2, None, None, None, 0.1, 1e-5, wfc, bfc, P)
    return {"ya": ya, "partial2": partial2, "b2": b2, "g2": g2, "be2": be2, "wfc": wfc, "bfc": bfc, "stats2": stats2,
            "aff2": aff2, "dl": torch.randn(B, NC, device=gpu), "labels": torch.randint(0, NC, (B,), device=gpu),
            "plane": ya.shape[2]}


def _full(gpu, shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, device=gpu, dtype=dtype)


def _kept(*tensors):
    return all(bool((t == SENTINEL).all()) for t in tensors)


# ---------------------------------------------------------------- the four forwards
RANGE = (0, 8)  # the range form's channels in every case here


def _fwd_call(op, c, a, ws):
    """One forward op on the arguments a (the good ones, one of them replaced)."""
    ops = _ops()
    if op == "fused_head_forward":
        return ops.fused_head_forward(a["ya"], c["partial2"], c["b2"], c["g2"], c["be2"], None, None, None, 0.1, 1e-5,
                                      a["wfc"], a["bfc"], P, a["x_out"])
    if op == "fused_head_forward_aff":
        return ops.fused_head_forward_aff(a["ya"], a["aff2"], c["b2"], None, a["wfc"], a["bfc"], P, a["x_out"])
    if op == "fused_head_forward_aff_ce":
        return ops.fused_head_forward_aff_ce(a["ya"], a["aff2"], c["b2"], None, a["wfc"], a["bfc"], P, a["labels"],
                                             a["x_out"])
    return ops.fused_head_forward_range(a["ya"], a["aff2"], c["b2"], None, a["wfc"], a["bfc"], P, *RANGE, *ws,
                                        a["labels"], a["x_out"])


FWD_OPS = {  # op -> the arguments it takes
    "fused_head_forward": ("ya", "wfc", "x_out"),
    "fused_head_forward_aff": ("ya", "aff2", "wfc", "x_out"),
    "fused_head_forward_aff_ce": ("ya", "aff2", "wfc", "x_out", "labels"),
    "fused_head_forward_range": ("ya", "aff2", "wfc", "x_out", "labels"),
}


def _fwd_bad(gpu, c, cols):
    """(name, argument, bad value[, further replacements that keep the rest consistent with it])."""
    B, plane = c["ya"].shape[0], c["plane"]
    return [
        ("ya dtype", "ya", c["ya"].float()),
        ("ya plane length", "ya", torch.zeros(B, 32, plane + 8, device=gpu, dtype=torch.float16)),
        ("ya second dimension", "ya", torch.zeros(B, 31, plane, device=gpu, dtype=torch.float16)),
        ("fc.weight columns", "wfc", torch.zeros(NC, K + 4, device=gpu)),
        ("fc.weight 11 rows", "wfc", torch.zeros(11, K, device=gpu), {"bfc": None}),
        ("aff2 of 63 floats", "aff2", c["aff2"][:63].clone()),
        ("x_out shape", "x_out", _full(gpu, (B, cols + 4))),
        ("labels int32", "labels", c["labels"].int()),
        ("labels of length B + 1", "labels", torch.zeros(B + 1, device=gpu, dtype=torch.long)),
        ("labels on the CPU", "labels", c["labels"].cpu()),
    ]


@pytest.mark.parametrize("op", list(FWD_OPS))
def test_forward_refusals(gpu, op):
    ops = _ops()
    c = _case(gpu, 1)
    B = 1
    cols = (RANGE[1] - RANGE[0]) * QQ if op == "fused_head_forward_range" else K
    wfc0 = c["wfc"].clone()

    def args():
        return {"ya": c["ya"], "aff2": c["aff2"], "wfc": c["wfc"], "bfc": c["bfc"], "labels": c["labels"],
                "x_out": _full(gpu, (B, cols))}

    def workspace(wfc):
        if op != "fused_head_forward_range":
            return ()
        ws = ops.head_forward_range_ws(c["ya"], wfc, P)  # (sized by fc.weight's rows)
        for t in ws:
            t.fill_(SENTINEL)
        return ws

    ran = 0
    for name, key, bad, *more in _fwd_bad(gpu, c, cols):
        if key not in FWD_OPS[op]:
            continue
        a = args()
        a.update({key: bad}, **(more[0] if more else {}))
        ws = workspace(a["wfc"])
        with pytest.raises(RuntimeError):
            _fwd_call(op, c, a, ws)
        assert _kept(a["x_out"], *ws), (op, name)
        assert torch.equal(c["wfc"], wfc0), (op, name)
        ran += 1
    assert ran == {3: 6, 4: 7, 5: 10}[len(FWD_OPS[op])]
    a = args()  # the call they all vary is a good one
    ws = workspace(a["wfc"])
    _fwd_call(op, c, a, ws)
    assert not _kept(a["x_out"])
    workspace(a["wfc"])  # (the range left unfinished: opening a sequence resets the stream's channel counter)


# ---------------------------------------------------------------- the pooled updates
SHARD = (4, 12)


def _pooled_args(gpu, B, shard):
    ops = _ops()
    c = _case(gpu, B)
    ya_all = torch.stack([c["ya"], c["ya"].flip(0)]).contiguous()  # [W, B, 32, plane]
    if shard:
        ya_all = ya_all[:, :, SHARD[0]:SHARD[1]].contiguous()
    rec = ops.head_pooled_record(c["aff2"], c["b2"], None)
    return {"dl": torch.randn(W * B, NC, device=gpu), "ya": ya_all, "rec": torch.stack([rec, rec]).contiguous(),
            "wfc": c["wfc"].clone(), "out": _full(gpu, (NC, K)), "lr": 0.5, "mode": 1, "c0": SHARD[0], "c1": SHARD[1]}


def _pooled_call(a, shard):
    ops = _ops()
    if shard:
        return ops.head_update_pooled_shard(a["dl"], a["ya"], a["rec"], a["wfc"], a["out"], P, a["c0"], a["c1"], 1.0,
                                            a["lr"], a["mode"])
    return ops.head_update_pooled(a["dl"], a["ya"], a["rec"], a["wfc"], a["out"], P, 1.0, a["lr"], a["mode"])


@pytest.mark.parametrize("shard", [False, True], ids=["head_update_pooled", "head_update_pooled_shard"])
def test_pooled_update_refusals(gpu, shard):
    good = _pooled_args(gpu, 1, shard)
    nine = _pooled_args(gpu, 9, shard)
    # a contiguous [NC, K] view one float off the 16-B grid
    off = _full(gpu, (NC * K + 4,))
    bad = {
        "mode 3": (good, {"mode": 3}),
        "mode 1 without out": (good, {"out": None}),
        "mode 2 without out": (good, {"out": None, "mode": 2}),
        "mode 0 with lr = 0": (good, {"mode": 0, "lr": 0.0}),
        "out off 16-B alignment": (good, {"out": off[1:1 + NC * K].view(NC, K)}),
        "rec_all of 127 columns": (good, {"rec": good["rec"][:, :127].contiguous()}),
        "dl_all with W B + 1 rows": (good, {"dl": torch.randn(W + 1, NC, device=gpu)}),
        "9 images per rank": (nine, {}),
    }
    if shard:
        bad.update({
            "c0 == c1": (good, {"c1": SHARD[0]}),
            "c1 = 33": (good, {"c0": 25, "c1": 33}),
            "ya_sh channels != c1 - c0": (good, {"ya": good["ya"][:, :, :7].contiguous()}),
        })
    for name, (base, kw) in bad.items():
        a = dict(base, **kw)
        w0 = a["wfc"].clone()
        with pytest.raises(RuntimeError):
            _pooled_call(a, shard)
        assert torch.equal(a["wfc"], w0) and _kept(good["out"], nine["out"], off), name
    for mode in (1, 0):  # the call they all vary is a good one, and so is its mode 0
        a = dict(good, mode=mode, out=_full(gpu, (NC, K)))
        w0 = a["wfc"].clone()
        _pooled_call(a, shard)
        assert _kept(a["out"]) == (mode == 0) and torch.equal(a["wfc"], w0) == (mode == 1), mode


# ---------------------------------------------------------------- the backward
def _bwd_args(gpu, B):
    ops = _ops()
    c = _case(gpu, B)
    return {"c": c, "wfc": c["wfc"].clone(), "dw_out": _full(gpu, (NC, K)), "mom_buf": _full(gpu, (NC, K)),
            "g2m_out": _full(gpu, (B * K + 32,), torch.float16)[:B * K].view(B, 32, Q, Q),
            "partial_out": _full(gpu, (ops.head_bwd_workspace(B, P),), torch.float64)}


def _bwd_call(a, lr=0.0, keep_dw=True, mom_buf=None, weight_decay=0.0, momentum=0.0):
    c = a["c"]
    # the forward of this weight on this stream (the backward's g2m scales come from its maxima)
    _ops().fused_head_forward_aff(c["ya"], c["aff2"], c["b2"], None, a["wfc"], c["bfc"], P)
    return _ops().fused_head_backward(c["dl"], c["ya"], c["stats2"], c["aff2"], c["b2"], c["g2"], a["wfc"], P,
                                      a["dw_out"], 1.0, True, lr, keep_dw=keep_dw, g2m_out=a["g2m_out"],
                                      partial_out=a["partial_out"], mom_buf=mom_buf, weight_decay=weight_decay,
                                      momentum=momentum)


def test_backward_refusals(gpu):
    one, nine = _bwd_args(gpu, 1), _bwd_args(gpu, 9)
    bad = {
        "keep_dw=False with update_lr = 0": (one, dict(keep_dw=False)),
        "weight_decay without mom_buf": (one, dict(lr=0.01, weight_decay=1e-4)),
        "mom_buf is fc.weight": (one, dict(lr=0.01, momentum=0.9, mom_buf=one["wfc"])),
        "mom_buf with 9 images": (nine, dict(lr=0.01, momentum=0.9, mom_buf=nine["mom_buf"])),
    }
    for name, (a, kw) in bad.items():
        w0 = a["wfc"].clone()
        with pytest.raises(RuntimeError):
            _bwd_call(a, **kw)
        assert torch.equal(a["wfc"], w0), name
        assert _kept(a["dw_out"], a["mom_buf"], a["g2m_out"], a["partial_out"]), name
    # the calls they vary are good ones: the momentum step at one image, the plain backward at nine
    w0 = one["wfc"].clone()
    _bwd_call(one, lr=0.01, momentum=0.9, mom_buf=one["mom_buf"])
    assert not torch.equal(one["wfc"], w0)
    assert not _kept(one["dw_out"]) and not _kept(one["mom_buf"]) and not _kept(one["g2m_out"])
    _bwd_call(nine)
    assert not _kept(nine["dw_out"]) and _kept(nine["mom_buf"])
