// Geometry of the inference head's packed fc weight (head_inf.hip): shared by the pack kernel, the
// forward kernel and the host checks (csrc/fused_ops.cpp).
//
// The pack follows ya's pooled-blocked layout (pooled_layout.h): one block = 4 pooled rows x 8 pooled
// columns = the K = 32 of one v_mfma_f32_16x16x32_f16.  A lane's 8 K values are one block row (K group
// g = row of the block), a "piece": 8 fp16 = 16 B ("fp16" kind) or 8 E4M3 bytes ("fp8" kind).  Pieces
// are ordered
//
//   piece(c, R, bx, g, j) = (((c * Q4 + R) * Q8 + bx) * 4 + g) * NC + j,   element e = column 8 bx + e
//
// so the B fragment of (channel, block, K group) is one contiguous run of NC pieces -- no padding
// classes are stored -- and a (channel, band of block rows) is one contiguous run of the pack, as it
// is of every image's ya.  Positions outside the Q x Q image hold zeros.
#pragma once

#include <stdint.h>

#include "pooled_layout.h"

namespace tds {

enum HeadInfKind { kHeadInfF16 = 0, kHeadInfF8 = 1 };

constexpr int HI_BAND = 4;      // block rows per workgroup
constexpr int HI_MAX_B = 32;    // two 16-image M tiles
constexpr int HI_MAX_NC = 64;   // four 16-class N tiles
constexpr int HI_F16_TOP = 15;  // fp16 values are stored below 2^15 (the weight at 2^e_j, X at s_x)
constexpr int HI_EXP_LIM = 120; // |exponent| limit of the power-of-two scales (no fp32 weight can overflow at it)

// pieces of the whole pack; bytes = pieces * (16 or 8)
__host__ __device__ inline int64_t hi_pack_pieces(int Q, int NC) {
  const PBGeom g = pb_geom(Q);
  return (int64_t)32 * g.Q4 * g.Q8 * 4 * NC;
}
__host__ __device__ inline int hi_piece_bytes(int kind) { return kind == kHeadInfF8 ? 8 : 16; }
// scale exponents: one per class (fp16), one per (channel, class) (fp8: wexp[c * NC + j])
__host__ __device__ inline int64_t hi_exp_count(int NC, int kind) { return kind == kHeadInfF8 ? (int64_t)32 * NC : NC; }
__host__ __device__ inline int hi_nband(int Q) { return (pb_geom(Q).Q4 + HI_BAND - 1) / HI_BAND; }

}  // namespace tds
