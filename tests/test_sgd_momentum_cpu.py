"""SGD momentum / weight decay off the GPU: ops.optim.SGD's flat-branch bookkeeping with the native
ops stubbed, the whole-step query of ops/fused_update.py and what it refuses, and the trainer's
--momentum / --weight-decay / --dampening / --nesterov flags with --checkpoint / --resume."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from torch_distributed_sandbox_amd.ops import SGD, fused_update
from torch_distributed_sandbox_amd.ops import optim as optim_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _OnDevice(torch.Tensor):
    """A CPU tensor that reports is_cuda: the optimizer's flat branches run with the ops stubbed."""
    is_cuda = property(lambda self: True)


class _Owner:
    """Stands for DistributedDataParallel behind the deferred runner (runner.__self__)."""

    def __init__(self, inline):
        self.inline, self.inline_calls, self.runner_calls, self.update_fn = inline, 0, 0, None

    def take_inline_deferred(self):
        self.inline_calls += 1
        return list(self.inline)

    def run(self, update_fn):
        self.runner_calls += 1
        self.update_fn = update_fn


def _flat_optimizer(monkeypatch, **hp):
    """Three parameters as views of a 100-element flat buffer: a [0, 50), w [50, 90) (deferred,
    stepped inside its backward: no gradient), bias [90, 100) (deferred, stepped inline)."""
    calls = []

    class _Ops:
        def sgd_step_(self, ps, gs, bs, lr, wd, mom, damp, nest, first):
            assert len(ps) == len(gs) and (not bs or len(bs) == len(ps))
            calls.append({"p": [(p.data_ptr(), p.numel()) for p in ps], "g": [(g.data_ptr(), g.numel()) for g in gs],
                          "b": [(b.data_ptr(), b.numel()) for b in bs], "args": (lr, wd, mom, damp, nest), "first": first})

    monkeypatch.setattr(optim_mod._ext, "ops", lambda: _Ops())
    base, fg = torch.zeros(100), torch.zeros(100)
    params = []
    for off, n in ((0, 50), (50, 40), (90, 10)):
        p = nn.Parameter(torch.zeros(n))
        p.data = base[off:off + n]
        params.append(p)
    a, w, bias = params
    a.grad, bias.grad = fg[0:50], fg[90:100]
    opt = SGD(params, 0.1, **hp)
    opt.set_flat_buffers(base.as_subclass(_OnDevice), fg, params)
    owner = _Owner([(90, 10)])
    opt.set_deferred([(50, 50)], owner.run, stepped=lambda p: p is w)
    return opt, owner, calls, base, fg, params


def test_flat_momentum_branch_bookkeeping(monkeypatch):
    opt, owner, calls, base, fg, (a, w, bias) = _flat_optimizer(monkeypatch, momentum=0.9, weight_decay=1e-4,
                                                                 nesterov=True)
    # the backward kernel's query creates the flat buffer: the creating step
    st = opt.fused_step(w)
    fb = opt._flat_mom
    assert st["first_step"] and st["buf"].data_ptr() == fb.data_ptr() + 50 * 4 and st["buf"].shape == w.shape
    assert (st["lr"], st["momentum"], st["weight_decay"], st["dampening"], st["nesterov"]) == (0.1, 0.9, 1e-4, 0.0, True)
    assert opt.fused_step(w)["first_step"]  # still this step
    for step in range(3):
        calls.clear()
        opt.step()
        assert owner.runner_calls == step + 1 and owner.inline_calls == step + 1  # once per step, inline ranges taken
        assert len(calls) == 1  # one launch: the non-deferred range and the inline leftovers
        c = calls[0]
        assert c["p"] == [(base.data_ptr(), 50), (base.data_ptr() + 360, 10)]
        assert c["g"] == [(fg.data_ptr(), 50), (fg.data_ptr() + 360, 10)]
        assert c["b"] == [(fb.data_ptr(), 50), (fb.data_ptr() + 360, 10)]
        assert c["args"] == (0.1, 1e-4, 0.9, 0.0, True)
        assert c["first"] == (step == 0)
        # the runner's update_fn steps parameter, gradient and momentum slices, with this step's flag
        owner.update_fn(50, 40)
        u = calls[1]
        assert u["p"] == [(base.data_ptr() + 200, 40)] and u["g"] == [(fg.data_ptr() + 200, 40)]
        assert u["b"] == [(fb.data_ptr() + 200, 40)] and u["first"] == (step == 0)
        assert not opt.fused_step(w)["first_step"]  # the next backward's query
    # torch's state layout: one buffer per parameter, views of the flat one
    sd = opt.state_dict()
    assert [tuple(s["momentum_buffer"].shape) for s in sd["state"].values()] == [(50,), (40,), (10,)]
    for p in (a, w, bias):
        assert opt.state[p]["momentum_buffer"].untyped_storage().data_ptr() == fb.untyped_storage().data_ptr()


def test_flat_weight_decay_only_has_no_buffer(monkeypatch):
    opt, owner, calls, base, fg, (a, w, bias) = _flat_optimizer(monkeypatch, weight_decay=1e-4)
    st = opt.fused_step(w)
    assert st["buf"] is None and not st["first_step"] and opt._flat_mom is None
    opt.step()
    assert owner.runner_calls == 1 and len(calls) == 1
    assert calls[0]["b"] == [] and calls[0]["args"] == (0.1, 1e-4, 0.0, 0.0, False) and not calls[0]["first"]
    assert "momentum_buffer" not in opt.state[a]


def test_load_state_dict_fills_flat_buffer_and_is_not_first(monkeypatch):
    opt, owner, calls, base, fg, params = _flat_optimizer(monkeypatch, momentum=0.9)
    opt.fused_step(params[1])
    opt.step()
    for i, p in enumerate(params):
        opt.state[p]["momentum_buffer"].fill_(float(i + 1))
    sd = {"state": {k: {"momentum_buffer": v["momentum_buffer"].clone()} for k, v in opt.state_dict()["state"].items()},
          "param_groups": opt.state_dict()["param_groups"]}
    opt2, owner2, calls2, _, _, params2 = _flat_optimizer(monkeypatch, momentum=0.9)
    opt2.load_state_dict(sd)
    fb = opt2._flat_mom
    assert fb is not None and not opt2._mom_fresh
    assert torch.equal(fb[:50], torch.full((50,), 1.0)) and torch.equal(fb[50:90], torch.full((40,), 2.0))
    assert torch.equal(fb[90:], torch.full((10,), 3.0))
    for p in params2:
        assert opt2.state[p]["momentum_buffer"].untyped_storage().data_ptr() == fb.untyped_storage().data_ptr()
    assert not opt2.fused_step(params2[1])["first_step"]
    opt2.step()
    assert calls2[0]["first"] is False


def test_partial_state_is_zero_filled_or_refused(monkeypatch):
    """Only some parameters hold a buffer (an entry of None counts as none): without dampening the
    missing ones are zeros -- torch's buf = d on their first step is mom * 0 + d -- and the step still
    takes the flat branch and calls the runner; with dampening the state is refused."""
    opt, owner, calls, base, fg, (a, w, bias) = _flat_optimizer(monkeypatch, momentum=0.9)
    opt.state[a]["momentum_buffer"] = torch.full((50,), 2.0)
    opt.state[w]["momentum_buffer"] = None
    st = opt.fused_step(w)
    assert not st["first_step"] and torch.equal(st["buf"], torch.zeros(40))
    assert torch.equal(opt.state[a]["momentum_buffer"], torch.full((50,), 2.0))
    assert opt.state[a]["momentum_buffer"].untyped_storage().data_ptr() == st["buf"].untyped_storage().data_ptr()
    opt.step()
    assert owner.runner_calls == 1 and len(calls) == 1 and calls[0]["first"] is False
    opt, owner, calls, base, fg, (a, w, bias) = _flat_optimizer(monkeypatch, momentum=0.9, dampening=0.5)
    opt.state[a]["momentum_buffer"] = torch.full((50,), 2.0)
    with pytest.raises(RuntimeError):
        opt.step()
    # entries of None only: no buffer yet, the creating step
    opt, owner, calls, base, fg, params = _flat_optimizer(monkeypatch, momentum=0.9, dampening=0.5)
    for p in params:
        opt.state[p]["momentum_buffer"] = None
    opt.step()
    assert owner.runner_calls == 1 and calls[0]["first"] is True


# ---------------------------------------------------------------- the query's refusals
def _cpu_ddp(monkeypatch, world_size=1):
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    m = ConvNet(image_shape=(256, 256))  # fc 10 x 131072: a deferred (exchange-candidate) layer
    ddp = DistributedDataParallel(m)
    ddp._deferred = [ddp._layer_bucket[id(m.fc)]]
    ddp.world_size = world_size
    return m, ddp


def test_whole_step_query_and_refusals(monkeypatch):
    m, ddp = _cpu_ddp(monkeypatch)
    opt = ddp.attach_optimizer(SGD(m.parameters(), 0.1, momentum=0.9, nesterov=True, weight_decay=1e-4))
    w = m.fc.weight
    st = fused_update.take_step(w)
    assert st is not None and st["momentum"] == 0.9 and st["nesterov"] and st["first_step"]
    assert st["buf"].shape == w.shape and st["buf"].data_ptr() == opt.state[w]["momentum_buffer"].data_ptr()
    # the plain-SGD queries answer None for this group: the exchanged paths keep writing dW
    assert fused_update.take(w) is None and fused_update.take(w, exchanged=True) is None
    # already done this step / a gradient is there / grad sync off
    fused_update.applied(w, grad_written=True)
    assert fused_update.take_step(w) is None
    ddp._fused_done.clear()
    with ddp.no_sync():
        assert fused_update.take_step(w) is None
    w.grad = torch.zeros_like(w)
    assert fused_update.take_step(w) is None
    w.grad = None
    assert fused_update.take_step(w) is not None
    # maximize
    opt.param_groups[0]["maximize"] = True
    assert fused_update.take_step(w) is None
    opt.param_groups[0]["maximize"] = False
    # the local query at world size > 1
    ddp.world_size = 2
    assert fused_update.take_step(w) is None and fused_update.take(w) is None
    ddp.world_size = 1
    # two groups
    opt.param_groups.append(dict(opt.param_groups[0], params=[]))
    assert fused_update.take_step(w) is None
    opt.param_groups.pop()
    assert fused_update.take_step(w) is not None
    assert fused_update.take_step(None) is None and fused_update.take_step(m.layer1[0].weight) is None


def test_plain_group_answers_both_queries(monkeypatch):
    m, ddp = _cpu_ddp(monkeypatch)
    ddp.attach_optimizer(SGD(m.parameters(), 0.1))
    w = m.fc.weight
    st = fused_update.take_step(w)
    assert st["lr"] == 0.1 and st["buf"] is None and st["momentum"] == 0.0
    assert fused_update.take(w) == 0.1
    m2, ddp2 = _cpu_ddp(monkeypatch)
    ddp2.attach_optimizer(SGD(m2.parameters(), 0.1, weight_decay=1e-4))
    # weight decay without momentum: no buffer for the kernel's momentum form, the optimizer's sweep steps it
    assert fused_update.take_step(m2.fc.weight) is None and fused_update.take(m2.fc.weight) is None


# ---------------------------------------------------------------- trainer flags, checkpoint / resume
def _train(args):
    e = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "mnist_onegpu.py", "--device", "cpu", "--image-size", "32", "--max-steps", "6",
                        "--log-interval", "1", "--lr", "0.05", "--dataset-size", "200", "--momentum", "0.9",
                        "--weight-decay", "1e-4", "--nesterov", "--json"] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stderr
    summ = json.loads(p.stdout.strip().splitlines()[-1])
    losses = {int(ep): [] for ep in re.findall(r"Epoch \[(\d+)/", p.stdout)}
    for ep, v in re.findall(r"Epoch \[(\d+)/\d+\], Step \[\d+/\d+\], Loss: ([\d.]+)", p.stdout):
        losses[int(ep)].append(float(v))
    return summ, losses


def test_trainer_momentum_flags_checkpoint_resume(tmp_path):
    ck = str(tmp_path / "ck.pt")
    s1, l1 = _train(["--epochs", "1", "--checkpoint", ck])
    for s in (s1,):
        assert (s["momentum"], s["weight_decay"], s["dampening"], s["nesterov"], s["lr"]) == (0.9, 1e-4, 0.0, True, 0.05)
    sd = torch.load(ck, weights_only=True)
    bufs = [st["momentum_buffer"] for st in sd["optimizer"]["state"].values()]
    assert len(bufs) == 10 and all(float(b.abs().max()) > 0 for b in bufs)
    s2, l2 = _train(["--epochs", "2", "--resume", ck])
    s3, l3 = _train(["--epochs", "2"])  # uninterrupted
    assert len(l3[1]) == 6 and l3[1] == l1[1]
    assert len(l2[2]) == 6 and l2[2] == l3[2]  # the second epoch continues as the uninterrupted run's
    assert s2["final_loss"] == s3["final_loss"]
    assert s2["momentum"] == 0.9 and s2["nesterov"] is True
