// Tile walk of the persistent layer-1 kernels (convnet_fused.hip): a workgroup takes the tiles
// t = t0, t0 + grid, t0 + 2 grid, ... of the list t = (b * tiles_r + tr) * tiles_c + tc.  The step
// is decomposed once, grid = (sb * tiles_r + sr) * tiles_c + sc, and a tile's coordinates follow
// from the previous tile's by two carries -- no division per tile (two divisions by run-time
// values per tile before, each through v_rcp_iflag_f32).  Host-callable: tests/test_l1_tiles_cpu.py
// holds it to the division form.
#pragma once

#if defined(__HIP__)
#define TDS_L1T_FN __host__ __device__ __forceinline__
#else
#define TDS_L1T_FN inline
#endif

namespace tds {

struct L1Walk {
  int b, tr, tc;   // the current tile; past the list when b >= B
  int sb, sr, sc;  // the step
};

TDS_L1T_FN L1Walk l1_walk_begin(int t0, int grid, int tiles_r, int tiles_c) {
  const int per_img = tiles_r * tiles_c;
  L1Walk w;
  w.b = t0 / per_img;
  int rem = t0 - w.b * per_img;
  w.tr = rem / tiles_c;
  w.tc = rem - w.tr * tiles_c;
  w.sb = grid / per_img;
  rem = grid - w.sb * per_img;
  w.sr = rem / tiles_c;
  w.sc = rem - w.sr * tiles_c;
  return w;
}

// tc, sc < tiles_c and tr, sr < tiles_r: one conditional subtraction per digit
TDS_L1T_FN void l1_walk_next(L1Walk& w, int tiles_r, int tiles_c) {
  w.tc += w.sc;
  const int cr = w.tc >= tiles_c ? 1 : 0;
  w.tc -= cr ? tiles_c : 0;
  w.tr += w.sr + cr;
  const int cb = w.tr >= tiles_r ? 1 : 0;
  w.tr -= cb ? tiles_r : 0;
  w.b += w.sb + cb;
}

}  // namespace tds
