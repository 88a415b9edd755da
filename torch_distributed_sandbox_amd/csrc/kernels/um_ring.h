// The moments half of the input kernels (ups_moments.hip's plain upsample, ups_affine.hip's affine
// sampling): the work split (one wave = a band of rows x up to 62 quads, lane l owning quad
// q0 + l - 1, lanes 0 and qpw + 1 the halo), the wave-wide DPP shifts that hand a row's edge quads
// to the neighbours, the five-row ring of nine byte windows, the 41 + 1 v_dot4_u32_u8 per quad and
// row.  A kernel computes a row's four levels per lane (`cur`) its own way, hands them to um_row
// and ends with the 42 wave sums as its partial row.
#pragma once
#include "common.h"
#include "xmom_u8.h"

namespace tds {

// (isolated op, r5_s35: 32 rows 48.1 - 48.6 us, 40: 47.0 - 48.6, 48: 45.8 - 46.2, 64: 45.3 - 46.7)
constexpr int UM_RB = 48;         // output rows per wave
constexpr int UM_QPW = 62;        // quads per wave at most (lanes 1..62 own them)
// a lane's sums: UM_RB rows x 4 products <= 255^2 each; the wave's: 62 lanes
static_assert((unsigned long long)UM_RB * 4ull * 62ull * 65025ull < (1ull << 32), "u32 wave sums would wrap");
static_assert(UM_RB + 4 <= 64, "one lane per row of the band");

struct UmGeo {
  int nqg, qpw, nband;
};
static inline UmGeo um_geo(int H, int W, int rb = UM_RB) {
  UmGeo g;
  const int nq = W / 4;
  g.nqg = (nq + UM_QPW - 1) / UM_QPW;
  g.qpw = (nq + g.nqg - 1) / g.nqg;
  g.nband = (H + rb - 1) / rb;
  return g;
}

__device__ __forceinline__ uint32_t um_shr1(uint32_t v) {  // lane l <- lane l - 1 (lane 0 <- 0)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t um_shl1(uint32_t v) {  // lane l <- lane l + 1 (lane 63 <- 0)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true);
}

typedef float um_f2 __attribute__((ext_vector_type(2)));

// Row i of the band (ring slot j = i % 5, static in the caller's loop unrolled by 5), its four
// levels in `cur` (0 in lanes without a quad and for rows past the image): the row's 9 byte
// windows go into the ring, and from i = 4 on the band's row i - 4 meets rows i - 4 .. i (ring
// slots j+1 .. j+5 mod 5).
__device__ __forceinline__ void um_row(uint32_t (&ring)[5][9], uint32_t (&acc)[42], int i, int j, uint32_t cur,
                                       bool own) {
  const uint32_t left = um_shr1(cur), right = um_shl1(cur);
#pragma unroll
  for (int s9 = 0; s9 < 9; ++s9) ring[j][s9] = xm_win(left, cur, right, s9);
  if (i >= 4) {
    const uint32_t u = own ? ring[(j + 1) % 5][4] : 0u;
    int k = 0;
#pragma unroll
    for (int dx = 0; dx <= 4; ++dx, ++k) acc[k] = __builtin_amdgcn_udot4(u, ring[(j + 1) % 5][4 + dx], acc[k], false);
#pragma unroll
    for (int dy = 1; dy <= 4; ++dy)
#pragma unroll
      for (int dx = -4; dx <= 4; ++dx, ++k)
        acc[k] = __builtin_amdgcn_udot4(u, ring[(j + 1 + dy) % 5][4 + dx], acc[k], false);
    acc[41] = __builtin_amdgcn_udot4(u, 0x01010101u, acc[41], false);
  }
}

}  // namespace tds
