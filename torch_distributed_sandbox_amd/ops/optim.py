"""SGD with a multi-tensor gfx950 kernel (``torch.optim.SGD(params, lr)``, mnist_onegpu.py:49).

One launch updates every parameter (tensor table in the kernel arguments,
SURVEY.md §2.4 K26).  When the parameters live in one flat buffer (as laid
out by ``parallel.ddp.DistributedDataParallel``), the update is a single
contiguous sweep over that buffer and its flat gradient bucket.  Momentum and weight decay
take the same flat paths: the momentum buffers are views of one flat buffer laid out like the
flat parameters, and a backward kernel that steps a parameter itself gets the whole rule and
the parameter's buffer from ``fused_step`` (ops/fused_update.py ``take_step``).
"""
from __future__ import annotations

import torch

from .. import _ext


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)
        self._flat = None  # (flat_param, flat_grad) when installed by DDP
        self._deferred = None  # ([(offset, numel)], runner) when DDP overlaps part of the update
        self._stepped = None  # predicate: parameter already stepped inside its backward (no .grad)
        # momentum with flat buffers: one buffer laid out like flat_param, created on first use;
        # state[p]["momentum_buffer"] are views of it.  _mom_fresh: created and not yet stepped
        # (torch's first step, buf = d: its contents are ignored)
        self._flat_mom = None
        self._mom_fresh = False

    def set_flat_buffers(self, flat_param: torch.Tensor, flat_grad, params):
        """Declare that ``params`` are views of ``flat_param`` with grads in ``flat_grad`` (a tensor,
        or a callable returning the buffer as it is at step time: DDP allocates the big layers'
        gradient slots at the buffer's end on first use, parallel/ddp.py ``_lazy_from``)."""
        ids = {id(p) for g in self.param_groups for p in g["params"]}
        if ids == {id(p) for p in params} and len(self.param_groups) == 1:
            self._flat = (flat_param, flat_grad, list(params))
        else:
            self._flat = None

    def set_deferred(self, ranges, runner, stepped=None):
        """DDP(overlap_optimizer=True): the flat ranges in ``ranges`` are updated by
        ``runner(update_fn)`` on DDP's side stream; the rest here, on the current stream.
        ``stepped(p)``: True for a parameter whose update already ran inside its backward
        kernel without a gradient (ops/fused_update.py); the runner skips it."""
        self._deferred = (sorted(ranges), runner) if ranges else None
        self._stepped = stepped

    def _ensure_flat_mom(self):
        """The flat momentum buffer.  Buffers the state already holds -- from the per-parameter
        path or ``load_state_dict`` -- are copied in and re-pointed, and the buffer then does not
        count as fresh.  A state in which only some parameters hold a buffer (an entry of None
        counts as none): torch would create the missing ones with ``buf = d`` on their first step,
        which a zero buffer reproduces exactly when dampening is 0 (``mom * 0 + d``), so they are
        zero-filled then; with dampening it cannot be reproduced by one flag for the whole flat
        buffer and the state is refused."""
        fp, _, params = self._flat
        buf = self._flat_mom
        if buf is not None and buf.numel() == fp.numel() and buf.device == fp.device:
            return buf
        have = [p for p in params if self.state.get(p, {}).get("momentum_buffer") is not None]
        if have and len(have) != len(params) and self.param_groups[0]["dampening"] != 0.0:
            raise RuntimeError("SGD: only some parameters hold a momentum buffer; with dampening != 0 the flat "
                               "momentum buffer cannot continue such a state")
        buf = torch.zeros_like(fp)
        for p in params:
            off = (p.data_ptr() - fp.data_ptr()) // fp.element_size()
            view = buf[off:off + p.numel()].view_as(p)
            old = self.state[p].get("momentum_buffer")
            if old is not None:
                view.copy_(old)
            self.state[p]["momentum_buffer"] = view
        self._flat_mom = buf
        self._mom_fresh = not have
        return buf

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # loaded momentum buffers go into the flat buffer, the state's entries become its views
        self._flat_mom = None
        self._mom_fresh = False
        if self._flat is not None and any(st.get("momentum_buffer") is not None for st in self.state.values()):
            with torch.no_grad():
                self._ensure_flat_mom()

    def fused_step(self, p):
        """The whole step of ``p`` for a kernel that applies it inside the backward
        (ops/fused_update.py ``take_step``): lr, momentum, dampening, weight_decay, nesterov, the
        momentum buffer (a view of the flat one; None without momentum) and whether this step
        creates it.  None when the optimizer cannot hand the step out (several groups, maximize,
        no flat buffers)."""
        if len(self.param_groups) != 1 or self._flat is None:
            return None
        g = self.param_groups[0]
        if g.get("maximize", False):
            return None
        step = {"lr": float(g["lr"]), "momentum": float(g["momentum"]), "dampening": float(g["dampening"]),
                "weight_decay": float(g["weight_decay"]), "nesterov": bool(g["nesterov"]), "buf": None,
                "first_step": False}
        if step["momentum"] != 0.0:
            with torch.no_grad():
                self._ensure_flat_mom()
            step["buf"] = self.state[p]["momentum_buffer"]
            step["first_step"] = self._mom_fresh
        return step

    def _flat_grad(self):
        fg = self._flat[1]
        return fg() if callable(fg) else fg

    def _flat_ok(self):
        if self._flat is None:
            return False
        fp, _, params = self._flat
        fg = self._flat_grad()
        if self._deferred is None and fg.numel() != fp.numel():
            return False  # (a gradient slot never allocated: no single sweep)
        for p in params:
            if p.grad is None:
                if self._deferred is not None and self._stepped is not None and self._stepped(p):
                    continue
                return False
            # grads must still be views of the flat bucket
            if p.grad.untyped_storage().data_ptr() != fg.untyped_storage().data_ptr():
                return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, mom, damp = group["lr"], group["momentum"], group["dampening"]
            wd, nest = group["weight_decay"], group["nesterov"]
            if self._flat is not None and self._flat[0].is_cuda and self._flat_ok():
                # one sweep over the flat buffers and, under DDP's overlap, the deferred ranges on its
                # side stream.  With momentum the flat momentum buffer's slices go beside the
                # parameter's; the plain step passes no buffers and a rule of zeros
                plain = mom == 0.0 and wd == 0.0
                fp, fg = self._flat[0], self._flat_grad()
                fb = self._ensure_flat_mom() if mom != 0.0 else None
                rule = (lr, 0.0, 0.0, 0.0, False, False) if plain else (lr, wd, mom, damp, nest,
                                                                        mom != 0.0 and self._mom_fresh)
                sl = (lambda off, n: [fb[off:off + n]]) if fb is not None else (lambda off, n: [])

                def sweep(ps, gs, bs, _rule=rule):
                    _ext.ops().sgd_step_(ps, gs, bs, *_rule)

                if self._deferred is None:
                    sweep([fp], [fg], [fb] if fb is not None else [])
                else:
                    ranges, runner = self._deferred
                    ps, gs, bs, pos = [], [], [], 0
                    for off, n in ranges + [(fp.numel(), 0)]:
                        if off > pos:
                            ps.append(fp[pos:off])
                            gs.append(fg[pos:off])
                            bs += sl(pos, off - pos)
                        pos = off + n
                    # small leftovers of the deferred ranges the owner wants stepped here, in this sweep
                    owner = getattr(runner, "__self__", None)
                    for off, n in (owner.take_inline_deferred() if hasattr(owner, "take_inline_deferred") else []):
                        ps.append(fp[off:off + n])
                        gs.append(fg[off:off + n])
                        bs += sl(off, n)
                    if ps:
                        sweep(ps, gs, bs)
                    # (always: the runner waits for the bucket's collective and fences the parameters)
                    runner(lambda off, n: sweep([fp[off:off + n]], [self._flat_grad()[off:off + n]], sl(off, n)))
                if not plain:  # (a plain step leaves a buffer created by a backward kernel's query fresh)
                    self._mom_fresh = False
                continue
            params, grads, bufs, first = [], [], [], False
            for p in group["params"]:
                if p.grad is None:
                    continue
                params.append(p)
                grads.append(p.grad)
                if mom != 0.0:
                    st = self.state[p]
                    if st.get("momentum_buffer") is None:
                        st["momentum_buffer"] = torch.zeros_like(p)
                        first = True
                    bufs.append(st["momentum_buffer"])
            # (a flat buffer created this step, by a backward kernel's query: still its first step)
            first = first or (bool(bufs) and self._mom_fresh)
            self._mom_fresh = False
            if not params:
                continue
            if params[0].is_cuda:
                ok = all(p.is_contiguous() and g.is_contiguous() and p.dtype == torch.float32 for p, g in
                         zip(params, grads))
                if ok:
                    _ext.ops().sgd_step_(params, grads, bufs, lr, wd, mom, damp, nest, first)
                    continue
            # CPU / non-contiguous reference path (torch.optim.SGD semantics)
            for i, p in enumerate(params):
                d = grads[i]
                if wd != 0.0:
                    d = d.add(p, alpha=wd)
                if mom != 0.0:
                    b = bufs[i]
                    if first:
                        b.copy_(d)
                    else:
                        b.mul_(mom).add_(d, alpha=1.0 - damp)
                    d = d.add(b, alpha=mom) if nest else b
                p.add_(d, alpha=-lr)
        return loss
