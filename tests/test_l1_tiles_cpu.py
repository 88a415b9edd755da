"""The layer-1 kernels' tile walk (csrc/kernels/l1_tiles.h), run on the host through
ops.l1_tile_walk, against the division form it replaces: entry k of a workgroup's list is tile
t = t0 + k * grid, b = t // (tiles_r * tiles_c), tile row = t % (tiles_r * tiles_c) // tiles_c,
tile column = t % tiles_c; past the list only b >= B is promised."""
import pytest

from torch_distributed_sandbox_amd import _ext

# (B, tiles_r, tiles_c, grid): the bench shape's forward and backward lists on 2048 and 1280
# workgroups, one tile column, one tile row, one tile, grid = 1, grid > tiles, grid a multiple of an
# image's tiles, of a tile row's, and one short of / one past them
SWEEP = [(5, 188, 47, 2048), (5, 188, 47, 1280), (3, 9, 3, 64), (3, 17, 5, 64), (3, 17, 5, 40), (3, 9, 1, 4),
         (3, 1, 7, 4), (1, 1, 1, 1), (1, 1, 1, 8), (2, 3, 4, 1), (2, 3, 4, 100), (4, 3, 4, 12), (4, 3, 4, 24),
         (4, 3, 4, 4), (4, 3, 4, 8), (4, 3, 4, 11), (4, 3, 4, 13), (4, 3, 4, 3), (4, 3, 4, 5), (32, 2, 1, 64)]


@pytest.mark.parametrize("B,tr,tc,grid", SWEEP)
def test_walk_matches_the_division_form(B, tr, tc, grid):
    ops = _ext.ops()
    total = B * tr * tc
    seen = []
    firsts = range(grid) if grid <= 128 else list(range(3)) + list(range(grid // 2, grid // 2 + 3)) + [grid - 1]
    for t0 in firsts:
        n = max(0, -(-(total - t0) // grid))  # tiles of this list
        rows = ops.l1_tile_walk(t0, grid, tr, tc, n + 2).tolist()
        for k, (b, r, c) in enumerate(rows):
            t = t0 + k * grid
            if k < n:
                assert (b, r, c) == (t // (tr * tc), t % (tr * tc) // tc, t % tc), (t0, k)
                seen.append(t)
            else:
                assert b >= B, (t0, k)
    if grid <= 128:
        assert sorted(seen) == list(range(total))
