"""The layer-1 kernels' per-tile paths (csrc/kernels/convnet_fused.hip): the division-free tile walk
(l1_tiles.h), the addresses formed from a scalar tile base and a per-thread offset on tiles inside
the image and with per-lane bounds on border tiles, the forward's two alternating LDS buffers and the
backward's operand reads one K-step ahead.  References and bounds are tests/test_layer1_gpu.py's
(fp64, per element); nothing here is taken from a kernel's output.

Forward tiles are 16 x 64 pixels with a 20 x 72 window (the level input's pair words reach 4 columns
further: a tile is "inside" when c0 + 72 <= W, an fp32 image's when c0 + 68 <= W).  Square images, B = 3:
  H =  12  one tile per image, smaller than the tile (all four borders at once);
  H =  68  5 x 2 tiles: every tile a corner or a left / right edge, last tile row 4 high, last column 4 wide;
  H = 132  9 x 3 tiles: the middle column is inside for an fp32 image and a border tile for levels
           (64 + 72 > 132), top / bottom edge tiles, a 4-wide last column;
  H = 196  13 x 4 tiles: column 1 inside for both inputs, column 2 inside for fp32 only; 156 tiles;
  H = 260  17 x 5 tiles, 255 tiles.
On the full grid every tile of these images has a workgroup of its own.  The small grid is 64
workgroups (8 CUs x 8, SMALL_CUS): 156 tiles give each 2 or 3, 255 tiles 3 or 4 -- both LDS buffers
reused, lists that step over tile rows and from one image into the next (step 64 = 1 image + 12 tiles
at H = 196, 64 = 12 tile rows + 4 at H = 260).
Backward tiles are 8 x 32 pooled; P = 6, 34, 66, 98 on the full grid and on 32-40 workgroups (8 CUs x
4-5): P = 98 is 13 x 4 tiles x 3 images = 156, about 4 per workgroup, walked last to first."""
import pytest
import torch

from test_layer1_gpu import (INPUTS, KINDS, _aff33, _affine, _backward_inputs, _case, _check_backward, _check_p1,
                             _check_training_forward, _forward, _gamma, _ops, small_grid)  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [12, 68, 132, 196, 260]


def _bits(p1):
    return p1.view(torch.int16)


@INPUTS
@pytest.mark.parametrize("H", SIZES)
def test_training_forward_small_and_full_grid(gpu, small_grid, H, levels):
    """ops.fused_l1_forward on 64 workgroups: p1 within the per-element bound and the argmax byte exact
    on every clear window (test_layer1_gpu._check_training_forward, its bounds), for positive, mixed and
    zero gamma1; the full grid's p1 and idx1 are the same bytes (a tile's bytes do not depend on the list
    that reached it), and so is the p1 of the inference launch on the very affine the training launch
    used (the op returns its element 32; the 33 floats are one buffer)."""
    c = _case(gpu, H, 3, levels)
    ops = _ops()
    name = f"H={H} {'levels' if levels else 'image'}"
    for kind in ("positive", "mixed", "zero"):
        small_grid(True)
        p1, idx1 = _check_training_forward(gpu, c, kind, 3 * H, f"{name} {kind} 64 workgroups")
        small_grid(False)
        g1, be1 = _gamma(kind, 3 * H)
        (q1, qidx, _, _, p1s), _, _, _ = _forward(gpu, c, g1, be1)
        assert torch.equal(_bits(p1), _bits(q1)), f"{name} {kind}: p1 depends on the workgroup count"
        assert torch.equal(idx1, qidx), f"{name} {kind}: idx1 depends on the workgroup count"
        assert p1s.storage_offset() == 32 and p1s.untyped_storage().nbytes() >= 33 * 4
        aff = p1s.as_strided((33,), (1,), 0)
        for small in (False, True):
            small_grid(small)
            inf = ops.fused_l1_forward_inference(c.xin, c.w1, c.b1, aff)
            small_grid(False)
            assert torch.equal(_bits(inf), _bits(q1)), f"{name} {kind}: the inference launch's p1 differs (small grid: {small})"


@INPUTS
@pytest.mark.parametrize("H", SIZES)
def test_conv_epilogue_small_and_full_grid(gpu, small_grid, H, levels):
    """ops.fused_l1_forward_inference on a hand-built affine of every kind (test_layer1_gpu._affine):
    p1 within the bound on 64 workgroups, the same bytes on the full grid."""
    c = _case(gpu, H, 3, levels)
    ops = _ops()
    for k, kind in enumerate(KINDS):
        a, b = _affine(kind, 7 * H + 3 + k)
        aff = _aff33(gpu, a, b)
        small_grid(True)
        few = ops.fused_l1_forward_inference(c.xin, c.w1, c.b1, aff)
        small_grid(False)
        full = ops.fused_l1_forward_inference(c.xin, c.w1, c.b1, aff)
        assert torch.equal(_bits(few), _bits(full)), f"H={H} {kind}: p1 depends on the workgroup count"
        _check_p1(few, c, a, b, f"H={H} 64 workgroups {'levels' if levels else 'image'} {kind}")


@INPUTS
@pytest.mark.parametrize("own", [False, True], ids=["random_idx", "own_idx"])
@pytest.mark.parametrize("P", [6, 34, 66, 98])
def test_backward_small_and_full_grid(gpu, small_grid, P, own, levels):
    """ops.fused_l1_backward against test_layer1_gpu's fp64 reference and per-element bounds on the
    full grid and on 32-40 workgroups (the partial rows group the tiles differently, so each launch is
    held to the reference, not to the other); two calls on one grid are bit-identical."""
    dp1h, dec, args, refs = _backward_inputs(gpu, P, 3, levels, own_idx=own)
    ops = _ops()
    for small in (False, True):
        small_grid(small)
        out = ops.fused_l1_backward(dp1h, dec, *args, 1.0)
        again = ops.fused_l1_backward(dp1h, dec, *args, 1.0)
        small_grid(False)
        tag = f"P={P} {'levels' if levels else 'image'}{' own idx1' if own else ''} {'small' if small else 'full'} grid"
        _check_backward(out, refs, tag)
        for u, v, nm in zip(out, again, ("dw1", "db1", "dgamma1", "dbeta1")):
            assert torch.equal(u, v), f"{tag}: {nm} differs between two calls"
