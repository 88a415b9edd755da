// conv2 forward of the inference plan in FP8 (models/convnet_fused.py forward_inference with
// inference_precision="fp8"): ya = the conv2 output at each 2x2 pooling window's extreme, in the format
// conv2_fwd2.hip writes (pooled_layout.h, fp16, the extreme chosen by the sign of gamma2, gamma2 = 0
// pooling the first position), on the block-scaled v_mfma_scale_f32_16x16x128_f8f6f4: both operands
// OCP E4M3, K = 128 per instruction, fp32 accumulation.  A 16-pixel x 16-channel output tile takes 4
// MFMAs (K = 25 taps x 16 channels = 400, padded to 512; conv2_fp8.h) where the TF32-class kernel
// takes 13 on v_mfma_f32_16x16x32_f16.  Only inference can afford 4 significant bits: opt-in.
//
// Quantisation, all scales exact powers of two:
//   * p1 arrives as layer 1 writes it (NHWC fp16 at p1_scale).  inference_constants bounds it and
//     stores 2^ep with bound * 2^ep <= 448 in mag[kMagP1Fp8]; the staging converts p1h * 2^ep to E4M3
//     (fp16 -> fp32 and the scaling are exact, v_cvt_pk_fp8_f32 rounds to nearest even).
//   * the weights carry one scale per output channel, max |w_c| * 2^ew_c in (224, 448]
//     (conv2_pack.hip conv2_pack_fp8_kernel: the fragments and the 32 exponents).
//   * the scales are taken out ONCE IN THE EPILOGUE, not through the MFMA's E8M0 operands (both are
//     0x7f = 2^0): a lane's accumulators all belong to one output channel per N tile, so 2^-ew_c 2^-ep
//     folds into the factor the ya store multiplies by anyway (one v_mul per pooled value, as in
//     conv2_fwd2.hip); the scale operands would cost two more VGPRs per MFMA and buy nothing.
//   * ya = fp16(acc * 2^-ew_c * 2^-ep * 2^k), 2^k = mag[kMagScales + 2] from the pack (1.14 * 448 * 2^-ep
//     * max_c sum |w_c| * 2^k < 2^15: p1 at its bound cannot overflow it, 1.14 > (1 + 2^-4)^2 covers
//     both roundings), and mag[kMagScales] = 1: the head's decode d = mag[40] mag[41] / mag[42]
//     (launchers.h TdsYaDec) gives y2 = ya d + b2 with no change to the head.
//
// Work split.  Persistent workgroups of 4 waves walk conv2_fwd2's 8 x 16 tile table (one tile pools to
// one 4 x 8 block of ya).  Wave w owns output rows 2w, 2w + 1 of the tile -- whole pooling windows --
// and BOTH 16-channel N tiles, so an A fragment read from LDS feeds two MFMAs: 2 rows x 4 K-steps x 2
// N = 16 MFMAs and 16 ds_read_b128 per wave and tile.
//   * weights in registers: 2 N x 4 K-steps x 8 VGPRs = 64, loaded once per workgroup;
//   * p1 staged through registers: every thread loads two 16-B half records (8 channels) of the next
//     tile's 12 x 20 window before this tile's MFMAs, converts them after (8 v_cvt_f32_f16, 8 v_mul, 4
//     v_cvt_pk_fp8_f32 per chunk) and writes 8 B into the other LDS plane: one barrier per tile, the
//     global latency under the MFMAs.  (An LDS-DMA of the fp16 records needs a second LDS pass to
//     convert; the conversion in registers costs the VALU work once and halves the LDS traffic.)
//   * operand-to-lane map (conv2_fp8.h): lane (i = l & 15, g = l >> 4) of K-step s holds the tap pair
//     q = 4s + g of pixel column i: 32 contiguous bytes of the staged row r + ky at column i + kx.
//     C: row (pixel column) 4g + r, column (channel) i, as every 16x16 MFMA.
//   * LDS: two planes of 12 rows x 21 records of 16 B (column 20 stays zero: the nonexistent tap kx = 5
//     reads it), 4032 B each; a 16-lane group reads 256 contiguous bytes, conflict-free, and the
//     staging writes consecutive 8-B pieces.  The pooled block is staged as [32 co] x 17 words (16
//     words of 4 x 8 halves + 1 pad: lane (i, g) writes word 17 i + 4w + g, all 64 banks distinct) and
//     stored by the workgroup as 64-B runs per channel, double-buffered so the stores of tile t drain
//     under tile t + 1.  12.4 KiB per workgroup.
//   * registers: 64 weights + 16 accumulators + 16 A fragments in flight + 8 prefetched p1 + addresses:
//     under the 168 of 3 workgroups per CU.
// Edges: records outside the image are staged as zeros (padding 2 and partial tiles alike), loads are
// clamped to a valid address and masked; a partial tile's windows beyond the image land in ya's block
// padding (pooled_layout.h), nothing outside ya is written.
#include "conv2_fp8.h"
#include "launchers.h"
#include "pooled_layout.h"

namespace tds {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int F8_TH = 8, F8_TC = 16;
constexpr int F8_SR = F8_TH + 4, F8_SC = F8_TC + 4;  // 12 x 20 staged records
constexpr int F8_ROWB = (F8_SC + 1) * 16;            // + the zero column: 336 B per staged row
constexpr int F8_PLANE = F8_SR * F8_ROWB;            // 4032 B
constexpr int F8_CHUNKS = F8_SR * F8_SC * 2;         // 480 half records of 8 channels
constexpr int F8_THREADS = 256, F8_WG = 3;
constexpr int F8_YCO = 17;                           // words per channel of the staged pooled block
constexpr int F8_YSTAGE = 32 * F8_YCO * 4;           // 2176 B
constexpr int F8_OFF_Y = 2 * F8_PLANE;
constexpr int F8_LDS = F8_OFF_Y + 2 * F8_YSTAGE;
static_assert(F8_PLANE % 16 == 0 && F8_OFF_Y % 16 == 0, "LDS carve");
static_assert(F8_CHUNKS <= 2 * F8_THREADS, "two chunks per thread");

struct F8Tile {
  int b, r0, c0;
};

__device__ __forceinline__ F8Tile f8_tile(int entry) {  // entry: conv2_common.h tile order
  F8Tile x;
  x.b = (int)((uint32_t)entry >> 24);
  x.r0 = ((entry >> 12) & 4095) * F8_TH;
  x.c0 = (entry & 4095) * F8_TC;
  return x;
}

// A thread's two chunks of the staged window (tile-independent): chunk c -> record c / 2 = (rr, cc),
// channels 8 (c & 1) .. +7.  Chunks 480 .. 511 repeat chunk 479 (the same bytes written twice).
struct F8Lane {
  int rr[2], cc[2], half[2];
  uint32_t lds[2];
};

__device__ __forceinline__ F8Lane f8_lane(int tid) {
  F8Lane L;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = min(tid + u * F8_THREADS, F8_CHUNKS - 1);
    const int rec = c >> 1;
    L.half[u] = c & 1;
    L.rr[u] = rec / F8_SC;
    L.cc[u] = rec - L.rr[u] * F8_SC;
    L.lds[u] = (uint32_t)(L.rr[u] * F8_ROWB + L.cc[u] * 16 + L.half[u] * 8);
  }
  return L;
}

// the tile's window into registers: 8 fp16 channels per chunk, zeros outside the image
__device__ __forceinline__ void f8_load(const uint4* __restrict__ p1, const F8Tile& x, int P, const F8Lane& L,
                                        uint4 (&v)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int gr = x.r0 - 2 + L.rr[u], gc = x.c0 - 2 + L.cc[u];
    const bool ok = (unsigned)gr < (unsigned)P && (unsigned)gc < (unsigned)P;
    const int64_t idx = ((int64_t)(x.b * P + gr) * P + gc) * 2 + L.half[u];
    v[u] = p1[ok ? idx : 0];  // (clamped, then masked: the load itself is unconditional)
    if (!ok) v[u] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// p1h * 2^ep -> E4M3, into the plane
__device__ __forceinline__ void f8_stage(char* plane, const F8Lane& L, const uint4 (&v)[2], float psc) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const f16x8 h = __builtin_bit_cast(f16x8, v[u]);
    const uint32_t lo = f8_pack4((float)h[0] * psc, (float)h[1] * psc, (float)h[2] * psc, (float)h[3] * psc);
    const uint32_t hi = f8_pack4((float)h[4] * psc, (float)h[5] * psc, (float)h[6] * psc, (float)h[7] * psc);
    *reinterpret_cast<uint2*>(plane + L.lds[u]) = make_uint2(lo, hi);
  }
}

// one wave's 16 MFMAs: output rows 2wv + o, both N tiles
__device__ __forceinline__ void f8_compute(const char* plane, const i32x8 (&W)[2][F8_KSTEPS], f32x4 (&acc)[2][2],
                                           const uint32_t (&aoff)[F8_KSTEPS], int wv) {
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    acc[o][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[o][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* row = plane + (2 * wv + o) * F8_ROWB;
#pragma unroll
    for (int s = 0; s < F8_KSTEPS; ++s) {
      const uint4 lo = *reinterpret_cast<const uint4*>(row + aoff[s]);
      const uint4 hi = *reinterpret_cast<const uint4*>(row + aoff[s] + 16);
      const i32x8 a = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)  // formats 0 / 0: E4M3 x E4M3; both block scales 2^0 (0x7f)
        acc[o][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, W[nt][s], acc[o][nt], 0, 0, 0, 0x7f7f7f7f, 0,
                                                                      0x7f7f7f7f);
    }
  }
}

// window extreme in the direction of BN2's affine; a NaN anywhere wins (conv2_fwd2.hip f2_ext4)
__device__ __forceinline__ float f8_ext4(float a, float b, float c, float d, bool neg) {
  const float mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), __builtin_elementwise_maximum(c, d));
  const float mn = __builtin_elementwise_minimum(__builtin_elementwise_minimum(a, b), __builtin_elementwise_minimum(c, d));
  return neg ? mn : mx;
}

// the wave's 2 x 16 pixels x 32 channels -> pooled row wv of the staged block: lane (i, g) holds the
// windows (wv, 2g) and (wv, 2g + 1) of channels i and 16 + i; fac > 0, so v -> fp16(v fac) is monotone
// and the stored value is the window's extreme as a pixel-wise store would round it
__device__ __forceinline__ void f8_pool(const f32x4 (&acc)[2][2], uint32_t* ystage, int wv, int lane,
                                        const float (&fac)[2], const bool (&neg)[2], const bool (&zg)[2]) {
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    uint32_t e[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float v0 = acc[0][nt][2 * j], v1 = acc[0][nt][2 * j + 1], v2 = acc[1][nt][2 * j], v3 = acc[1][nt][2 * j + 1];
      const float m = zg[nt] ? v0 : f8_ext4(v0, v1, v2, v3, neg[nt]);  // gamma2 == 0: the first position
      e[j] = f16_bits(m * fac[nt]);
    }
    ystage[(16 * nt + li) * F8_YCO + 4 * wv + g] = e[0] | (e[1] << 16);
  }
}

// the workgroup stores a staged pooled block: thread e -> channel e / 8, halves 4 (e % 8) .. +3 (8 B)
__device__ __forceinline__ void f8_store_ya(const uint32_t* ystage, const F8Tile& x, unsigned short* __restrict__ ya,
                                            const PBGeom& pg, int tid) {
  const int tr = x.r0 / F8_TH, tc = x.c0 / F8_TC;  // = the tile's pooled block
  if (tr >= pg.Q4 || tc >= pg.Q8) return;
  const int co = tid >> 3, part = tid & 7;
  unsigned short* dst = ya + (((int64_t)(x.b * 32 + co) * pg.Q4 + tr) * pg.Q8 + tc) * 32 + part * 4;
  const uint32_t* src = ystage + co * F8_YCO + part * 2;
  st_stream(reinterpret_cast<uint2*>(dst), make_uint2(src[0], src[1]));
}

__global__ __launch_bounds__(F8_THREADS, F8_WG) void conv2_fwd_fp8_kernel(
    const uint4* __restrict__ p1, const uint4* __restrict__ wp8, const int* __restrict__ wexp,
    const float* __restrict__ gamma, unsigned short* __restrict__ ya, const uint32_t* __restrict__ mag,
    const int* __restrict__ order, int sw, int sk, int B, int P) {
  __shared__ __attribute__((aligned(16))) char smem[F8_LDS];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_c = (P + F8_TC - 1) / F8_TC, tiles_r = (P + F8_TH - 1) / F8_TH;
  const int total = tiles_c * tiles_r * B;
  const int w = xcd_remap(blockIdx.x, gridDim.x);
  const int* __restrict__ mine = order + w * sw;  // per-workgroup tile lists (fused_ops.cpp tile_order)
  // the zero column of both planes (never staged over)
  if (tid < 2 * F8_SR)
    *reinterpret_cast<uint4*>(smem + (tid / F8_SR) * F8_PLANE + (tid % F8_SR) * F8_ROWB + F8_SC * 16) =
        make_uint4(0u, 0u, 0u, 0u);
  // weights: [nt][s][tap of the pair][lane] uint4 (conv2_pack.hip conv2_pack_fp8_kernel)
  i32x8 W[2][F8_KSTEPS];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int s = 0; s < F8_KSTEPS; ++s) {
      const uint4 lo = wp8[((nt * F8_KSTEPS + s) * 2 + 0) * 64 + lane], hi = wp8[((nt * F8_KSTEPS + s) * 2 + 1) * 64 + lane];
      W[nt][s] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    }
  const float psc = __uint_as_float(mag[kMagP1Fp8]);       // 2^ep
  const float ksc = __uint_as_float(mag[kMagScales + 2]);  // 2^k
  float fac[2];
  bool neg[2], zg[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int co = 16 * nt + li;
    fac[nt] = ldexpf(ksc / psc, -wexp[co]);
    neg[nt] = gamma != nullptr && gamma[co] < 0.f;
    zg[nt] = gamma != nullptr && gamma[co] == 0.f;
  }
  uint32_t aoff[F8_KSTEPS];  // the lane's tap pair of K-step s, from the output row's first record
#pragma unroll
  for (int s = 0; s < F8_KSTEPS; ++s) {
    const int q = 4 * s + g;
    aoff[s] = (uint32_t)(f8_pair_ky(q) * F8_ROWB + (li + f8_pair_kx(q)) * 16);
  }
  const PBGeom pg = pb_geom(P / 2);
  const F8Lane L = f8_lane(tid);
  uint32_t* ys = reinterpret_cast<uint32_t*>(smem + F8_OFF_Y);
  f32x4 acc[2][2];
  uint4 pre[2];
  F8Tile nx{0, 0, 0}, prev{0, 0, 0};
  bool have_prev = false;
  int t = w;
  if (t < total) {
    nx = f8_tile(mine[0]);
    f8_load(p1, nx, P, L, pre);
    f8_stage(smem, L, pre, psc);
  }
  int kk = 0;
  for (; t < total; t += gridDim.x, ++kk) {
    const F8Tile cur = nx;
    const bool more = t + (int)gridDim.x < total;
    // plane kk & 1 is staged; plane (kk + 1) & 1 and pooled block kk & 1 are free; the pooled block of
    // tile t - 1 is complete
    __syncthreads();
    if (more) {
      nx = f8_tile(mine[(kk + 1) * sk]);
      f8_load(p1, nx, P, L, pre);
    }
    if (have_prev) f8_store_ya(ys + ((kk + 1) & 1) * (F8_YSTAGE / 4), prev, ya, pg, tid);
    f8_compute(smem + (kk & 1) * F8_PLANE, W, acc, aoff, wv);
    f8_pool(acc, ys + (kk & 1) * (F8_YSTAGE / 4), wv, lane, fac, neg, zg);
    if (more) f8_stage(smem + ((kk + 1) & 1) * F8_PLANE, L, pre, psc);
    prev = cur;
    have_prev = true;
  }
  __syncthreads();
  if (have_prev) f8_store_ya(ys + ((kk - 1) & 1) * (F8_YSTAGE / 4), prev, ya, pg, tid);
}

}  // namespace tds

using namespace tds;

void tds_conv2_fwd_fp8_tiles(int P, int* tiles_r, int* tiles_c) {
  *tiles_r = (P + F8_TH - 1) / F8_TH;
  *tiles_c = (P + F8_TC - 1) / F8_TC;
}

void tds_conv2_fwd_fp8(const void* p1, const void* wp8, const int* wexp, const float* gamma, unsigned short* ya,
                       const uint32_t* mag, const int* order, int nwg, int sw, int sk, int B, int P, hipStream_t st) {
  hipLaunchKernelGGL(conv2_fwd_fp8_kernel, dim3(nwg), dim3(F8_THREADS), 0, st, reinterpret_cast<const uint4*>(p1),
                     reinterpret_cast<const uint4*>(wp8), wexp, gamma, ya, mag, order, sw, sk, B, P);
  TDS_LAUNCH_CHECK();
}
