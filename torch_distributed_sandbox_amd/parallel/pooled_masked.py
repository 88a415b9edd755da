"""Sign-masked encoding of the fused head's pooled input ya for the activation exchange
(``source="pooled-masked"``, parallel/factored.py).

The pooled source all-gathers every rank's ya (fp16, pooled-blocked: csrc/kernels/pooled_layout.h)
and every rank recomputes ``X = relu(a*ya + b)`` from it.  About half of X is exactly zero, and which
half is known as soon as the rank's head record exists (``ops.head_pooled_record``: BN2's affine and
ya's decode), before the gather leaves.  This source sends the values whose X is not +0, one bit per
position and one value offset per page; the update kernels read a dropped position as +0.f, which is
what the dense kernels compute there, so the exchanged step is bitwise the pooled source's.

Format of one rank's ya ``[B, 32, Q4*Q8*32]`` (Q4 = ceil(Q/4), Q8 = ceil(Q/8) blocks of 4 pooled rows
x 8 pooled columns):

* a page is one chunk of the head kernels' walk: 32 consecutive blocks (1024 values) of one (image,
  channel, block row); a block row has ``ceil(Q8/32)`` pages, the last may hold fewer real blocks --
  the missing ones count as all-dropped.  Pages are ordered (image, channel, block row, chunk);
* ``meta`` int32 ``[npages * 33]``: per page its value offset (the exclusive prefix sum of the kept
  counts over this rank's pages) followed by 32 mask words; bit i of word k <-> value
  ``i = (py % 4)*8 + px % 8`` of block k of the chunk;
* ``values`` fp16 ``[cap]``: the kept values in (page, block, i) order;
* a value is kept iff ``relu(z)`` has any bit set (z > 0, or z is NaN), with ``z = fma(a*d, h, a*b2 + b)``
  formed from the rank's record as the head kernels form it, and the position lies inside the
  Q x Q image.

``meta`` is 132 B per 2048 dense bytes: bytes sent = 0.064 * dense + 2 * cap (+ the 512-B record).

GPU: ``ops.head_pooled_encode`` and ``ops.head_update_pooled_masked[_step]`` (csrc/kernels/
head_pb.hip).  The torch reference below serves the tests and CPU rehearsals; it forms z in fp64 and
rounds once, which is the kernels' fused multiply-add up to double rounding.
"""
from __future__ import annotations

from typing import Tuple

import torch

BLOCKS = 32          # blocks per page
META = 1 + BLOCKS    # int32 per page
REC = 128            # floats per head record


def geom(Q: int) -> Tuple[int, int, int]:
    """(Q4, Q8, pages per block row) of pooled size Q."""
    q8 = (Q + 7) // 8
    return (Q + 3) // 4, q8, (q8 + BLOCKS - 1) // BLOCKS


def npages(B: int, Q: int) -> int:
    q4, _, nch = geom(Q)
    return B * 32 * q4 * nch


def meta_numel(B: int, Q: int) -> int:
    return npages(B, Q) * META


def payload_bytes(B: int, Q: int, cap: int) -> int:
    """Bytes one rank sends per link under this source: meta, ``cap`` fp16 values, the record."""
    return 4 * META * npages(B, Q) + 2 * int(cap) + 4 * REC


def rank_x(ya: torch.Tensor, rec: torch.Tensor, Q: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(X, keep) of one rank's ya ``[B, 32, plane]`` and record, both ``[B, 32, Q4, Q8, 32]`` in ya's
    layout: X = relu(z) in fp32 with +0 outside the image, keep = X has a bit set."""
    q4, q8, _ = geom(Q)
    B = ya.shape[0]
    rec = rec.reshape(-1).float()
    a, b, ysc, b2 = rec[:32], rec[32:64], rec[64:67], rec[68:100]
    ad = a * (ysc[0] * ysc[1] / ysc[2])                                  # fp32, as hp_ydec
    bd = (a.double() * b2.double() + b.double()).float()                 # fmaf(a, b2, b)
    h = ya.reshape(B, 32, q4, q8, 32).double()
    z = (ad.double().view(1, 32, 1, 1, 1) * h + bd.double().view(1, 32, 1, 1, 1)).float()
    i = torch.arange(32, device=ya.device)
    py = 4 * torch.arange(q4, device=ya.device).view(q4, 1, 1) + (i // 8).view(1, 1, 32)
    px = 8 * torch.arange(q8, device=ya.device).view(1, q8, 1) + (i % 8).view(1, 1, 32)
    keep = ((z > 0) | torch.isnan(z)) & ((py < Q) & (px < Q)).view(1, 1, q4, q8, 32)
    return torch.where(keep, z, torch.zeros_like(z)), keep


def _paged(t: torch.Tensor, Q: int) -> torch.Tensor:
    """[B, 32, Q4, Q8, 32] -> [npages, 32 blocks, 32], block rows padded to whole pages."""
    q4, q8, nch = geom(Q)
    pad = nch * BLOCKS - q8
    if pad:
        t = torch.cat([t, t.new_zeros(t.shape[0], 32, q4, pad, 32)], dim=3)
    return t.reshape(-1, BLOCKS, 32)


def encode_ref(ya: torch.Tensor, rec: torch.Tensor, Q: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(meta, values, nnz) of one rank's ya -- the torch reference of ``ops.head_pooled_encode``."""
    _, keep = rank_x(ya, rec, Q)
    kp = _paged(keep, Q)
    counts = kp.sum((1, 2), dtype=torch.int64)
    offs = torch.cumsum(counts, 0) - counts
    words = (kp.to(torch.int64) << torch.arange(32, device=ya.device, dtype=torch.int64)).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)  # uint32 bits as int32
    meta = torch.cat([offs.to(torch.int32).view(-1, 1), words], dim=1).reshape(-1)
    vals = _paged(ya.reshape(keep.shape), Q)[kp]
    return meta, vals, int(vals.numel())


def decode_ref(meta: torch.Tensor, values: torch.Tensor, rec: torch.Tensor, B: int, Q: int) -> torch.Tensor:
    """X ``[B, 32*Q*Q]`` (the fc's flatten order) of one rank's payload -- torch reference: the kept
    values back in their places, X formed from them as the head forward does, +0 elsewhere."""
    q4, q8, nch = geom(Q)
    m = meta.view(-1, META)
    words = m[:, 1:].to(torch.int64) & 0xFFFFFFFF
    kp = ((words.unsqueeze(-1) >> torch.arange(32, device=meta.device, dtype=torch.int64)) & 1).bool()
    hp = torch.zeros(kp.shape, dtype=torch.float16, device=meta.device)
    hp[kp] = values.reshape(-1)[:int(kp.sum())]
    unpage = lambda t: t.reshape(B, 32, q4, nch * BLOCKS, 32)[:, :, :, :q8]
    x, _ = rank_x(unpage(hp).reshape(B, 32, -1), rec, Q)
    x = torch.where(unpage(kp), x, torch.zeros_like(x))
    # blocks [Q4, Q8, 4, 8] -> rows and columns, cut to the image
    x = x.view(B, 32, q4, q8, 4, 8).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, 4 * q4, 8 * q8)
    return x[:, :, :Q, :Q].reshape(B, -1)


def encode(ya: torch.Tensor, rec: torch.Tensor, P: int, meta_out: torch.Tensor, values_out: torch.Tensor):
    """Encode into meta_out ``[meta_numel]`` and values_out ``[cap]``; returns the 0-d int64 kept count
    (a device tensor, no host sync).  Values past cap are dropped; the consumer checks the count."""
    if ya.is_cuda:
        from .. import _ext

        return _ext.ops().head_pooled_encode(ya, rec, int(P), meta_out, values_out)
    meta, vals, nnz = encode_ref(ya, rec, P // 2)
    meta_out.copy_(meta)
    k = min(nnz, values_out.numel())
    values_out[:k].copy_(vals[:k])
    return torch.tensor(nnz, dtype=torch.int64)
