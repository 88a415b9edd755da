// Shared pieces of the FP8 (E4M3) inference conv2 (conv2_fwd_fp8.hip) and its weight pack
// (conv2_pack.hip conv2_pack_fp8_kernel): the K order of v_mfma_scale_f32_16x16x128_f8f6f4's operands,
// the power-of-two scale choice and the hardware conversion.
//
// K order.  One MFMA multiplies K = 128: lane l (i = l & 15, g = l >> 4) holds 32 operand bytes, K
// slots 32 g .. 32 g + 31 of row i (A) or column i (B).  conv2's K = 25 taps x 16 channels = 400 is
// padded to 512 = 4 MFMAs (s = 0 .. 3), K index = tap slot x 16 + channel.  A lane's 32 bytes are one
// tap PAIR q = 4 s + g: taps (ky, kx) and (ky, kx + 1), ky = q / 3, kx = 2 (q % 3), which are 32
// contiguous bytes of the staged tile (two neighbouring 16-B pixel records).  kx = 5 (the second tap
// of every third pair) and the pair q = 15 do not exist: their weight bytes are zero.
#pragma once

#include "conv2_common.h"

namespace tds {

constexpr int F8_KSTEPS = 4;
constexpr int F8_WFRAG_BYTES = 2 * F8_KSTEPS * 2 * 64 * 16;  // [nt 2][s 4][tap of the pair 2][lane 64][ci 16]
constexpr int kMagP1Fp8 = kMagScales + 5;  // mag[45] = 2^ep: p1h * 2^ep <= 448 (inference.hip writes it)
constexpr float F8_E4M3_MAX = 448.f;       // OCP e4m3fn

__host__ __device__ constexpr int f8_pair_ky(int q) { return q < 15 ? q / 3 : 0; }
__host__ __device__ constexpr int f8_pair_kx(int q) { return q < 15 ? 2 * (q % 3) : 0; }  // the pair's first tap

// the largest e with m * 2^e <= 448 (0 for m = 0 or a non-finite m), within +-100
__device__ __forceinline__ int f8_scale_exp(double m) {
  if (!(m > 0.0) || !__builtin_isfinite(m)) return 0;
  int x;
  const double f = frexp(m, &x);  // m = f 2^x, 0.5 <= f < 1; 448 = 0.875 * 2^9
  return min(100, max(-100, (f <= 0.875 ? 9 : 8) - x));
}

// four fp32 values -> four E4M3 bytes (a in the low byte), round to nearest even (v_cvt_pk_fp8_f32;
// the callers' scales keep every value within +-448, so no saturation mode is relied on)
__device__ __forceinline__ uint32_t f8_pack4(float a, float b, float c, float d) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

}  // namespace tds
