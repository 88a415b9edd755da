// The input op under a per-image affine map (random-affine augmentation: rotation, scale, shift):
// the 28x28 -> HxW upsample to uint8 levels that samples the source THROUGH the map at the output
// resolution -- one interpolation, no warped intermediate -- and forms the same 42 exact
// autocorrelation sums from the levels it writes as ups_moments.hip does, so the fused plan takes an
// augmented batch with no extra launch.  ups_moments.hip's separable taps (horizontal taps per
// thread, vertical per row) cannot express a rotation; this kernel samples every pixel on its own.
//
// Contract (mats[b] = m00 m01 m02 m10 m11 m12, fp32): output pixel (X, Y) of image b samples
//   u = fmaf(m00, X + 0.5f, fmaf(m01, Y + 0.5f, m02)),  v = fmaf(m10, X + 0.5f, fmaf(m11, Y + 0.5f, m12))
// (source pixel index units), clamped to [-1, w] x [-1, h] (a NaN lands on -1), bilinearly with
// zero padding: i0 = floor(u), ax = u - i0, likewise j0, ay, and
//   ups_lerp(ups_lerp(s[j0][i0], s[j0][i0+1], ax), ups_lerp(s[j0+1][i0], s[j0+1][i0+1], ax), ay)
// rounded to the nearest level (a convex combination of levels and 0: the magic-constant round of
// ups_moments.hip).  With mats[b] = (w/W, 0, -0.5, 0, h/H, -0.5) the coordinates and the lerps are
// the plain upsample's own, so the levels are its bytes wherever its edge clamp does not bind.
// A level is a pure function of (b, X, Y): u and v come from the absolute X and Y, so a halo lane
// or a row recomputed below a band reproduces the byte its owner stores.
//
// Work split and moments: um_ring.h, unchanged (one wave, UA_RB rows x up to 62 quads + 2 halo
// lanes, 4 more rows below the band).  The sampling front end is this kernel's own:
//   * LDS holds the source framed with zeros as VERTICAL pairs, one 8-byte entry per position:
//     vp[j + 1][i + 1] = (s[j][i], s[j + 1][i]) for j in [-1, h], i in [-1, w + 1], s = 0 outside
//     the source: (h + 2) x (w + 3) entries (7440 B at 28 x 28).  Zero padding needs no branch,
//     and after the clamp every index is in range for any matrix (largest: (h + 2)(w + 3) - 1).
//   * a pixel reads entries (j0, i0) and (j0, i0 + 1), adjacent in LDS: ONE ds_read2_b64 brings all
//     four taps, as (top-left, bottom-left) and (top-right, bottom-right).  The horizontal lerps of
//     the top and the bottom row are then the two halves of one packed multiply and one packed
//     fma; the vertical lerp is scalar.  Four LDS reads per quad and row.
//   * the row terms fmaf(m01, Y + 0.5f, m02), fmaf(m11, Y + 0.5f, m12) are wave-uniform: lane i
//     holds row r0 + i's, read back per row with v_readlane.
//   * the entry index is formed in fp32, (int)fmaf(j0, ld, i0) (exact: below 2^15), one
//     conversion for the pair of floors.
#include "common.h"
#include "launchers.h"
#include "ups_common.h"
#include "um_ring.h"

namespace tds {

#ifdef TDS_UA_RB  // (A/B builds of the band height: _build.py --variant ... -D TDS_UA_RB=32)
constexpr int UA_RB = TDS_UA_RB;
#else
// output rows per wave (isolated op, 3000^2 x 5: 32 rows 67.8 - 68.6 us, 48: 64.3 - 65.0, 60: 76.4 - 77.4)
constexpr int UA_RB = UM_RB;
#endif
static_assert((unsigned long long)UA_RB * 4ull * 62ull * 65025ull < (1ull << 32), "u32 wave sums would wrap");
static_assert(UA_RB + 4 <= 64, "one lane per row of the band");

// bytes of LDS for an h x w source
static size_t ua_lds_bytes(int h, int w) { return (size_t)(h + 2) * (w + 3) * sizeof(um_f2); }

__global__ __launch_bounds__(64) void ups_affine_moments_u8_kernel(const uint8_t* __restrict__ src,
                                                                   const float* __restrict__ mats,
                                                                   uint8_t* __restrict__ x,
                                                                   double* __restrict__ partial, int h, int w, int H,
                                                                   int W, int nqg, int qpw) {
  extern __shared__ um_f2 vp[];  // (h + 2) x ld vertical pairs
  const int b = blockIdx.y, unit = blockIdx.x, units = gridDim.x;
  const int lane = threadIdx.x;
  const uint8_t* s = src + (int64_t)b * h * w;
  const int ld = w + 3, n = (h + 2) * ld;
  for (int e0 = 0; e0 < n; e0 += 4 * 64) {  // every load issued before the first conversion
    uint8_t t[4], u[4];
    bool okt[4], oku[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + k * 64 + lane, row = e / ld;
      const int j = row - 1, i = e - row * ld - 1;  // entry (j, i): s[j][i] over s[j + 1][i]
      const bool in = e < n && i >= 0 && i < w;
      okt[k] = in && j >= 0 && j < h;
      oku[k] = in && j + 1 < h;
      t[k] = s[okt[k] ? j * w + i : 0];  // (clamped: used only in range)
      u[k] = s[oku[k] ? (j + 1) * w + i : 0];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + k * 64 + lane;
      if (e < n) vp[e] = um_f2{okt[k] ? (float)t[k] : 0.f, oku[k] ? (float)u[k] : 0.f};
    }
  }
  __syncthreads();
  const float* m = mats + b * 6;
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  const int qg = unit % nqg, band = unit / nqg;
  const int q = qg * qpw + lane - 1;
  const bool vq = lane <= qpw + 1 && q >= 0 && q < (W >> 2);
  const bool own = vq && lane >= 1 && lane <= qpw;
  um_f2 xf[2];  // X + 0.5 of pixels 0,1 | 2,3 (any value in lanes without a quad: the clamp holds)
#pragma unroll
  for (int k = 0; k < 4; ++k) xf[k >> 1][k & 1] = (float)(4 * q + k) + 0.5f;
  uint32_t acc[42];
#pragma unroll
  for (int i = 0; i < 42; ++i) acc[i] = 0u;
  uint32_t ring[5][9];
  const int r0 = band * UA_RB;
  // the row terms of the wave's rows r0 .. r0 + UA_RB + 3, lane i holding row r0 + i's
  const float yf = (float)(r0 + lane) + 0.5f;
  const float ru = fmaf(m01, yf, m02), rv = fmaf(m11, yf, m12);
  const float umax = (float)w, vmax = (float)h, ldf = (float)ld;
  const um_f2* vp0 = vp + ld + 1;  // entry (0, 0)
  const um_f2 m00_2 = {m00, m00}, m10_2 = {m10, m10};
  uint32_t* xrow = reinterpret_cast<uint32_t*>(x + ((int64_t)b * H + r0) * W) + q;
#pragma unroll 1
  for (int i0 = 0; i0 < UA_RB + 4; i0 += 5) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int i = i0 + j, r = r0 + i;
      if (i < UA_RB + 4) {
        uint32_t cur = 0u;
        if (r < H) {
          const float rowu = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ru), i));
          const float rowv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rv), i));
          const um_f2 rowu2 = {rowu, rowu}, rowv2 = {rowv, rowv};
          uint32_t lv[4];
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const um_f2 u2 = __builtin_elementwise_fma(m00_2, xf[p], rowu2);
            const um_f2 v2 = __builtin_elementwise_fma(m10_2, xf[p], rowv2);
            const float uu[2] = {u2.x, u2.y}, vv[2] = {v2.x, v2.y};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              // fmaxf first: a NaN becomes the lower bound; the conversion sees [-1, w] x [-1, h] only
              const float u = fminf(fmaxf(uu[k], -1.f), umax), v = fminf(fmaxf(vv[k], -1.f), vmax);
              const float fu = floorf(u), fv = floorf(v);
              const float ax = u - fu, ay = v - fv;
              const int e = (int)fmaf(fv, ldf, fu);  // in [-ld - 1, h * ld + w]
              const um_f2 lf = vp0[e], rt = vp0[e + 1];
              // (top, bottom) = ups_lerp(left, right, ax) of both rows at once
              const um_f2 ax2 = {ax, ax}, nx2 = {1.f - ax, 1.f - ax};
              const um_f2 tb = __builtin_elementwise_fma(ax2, rt, nx2 * lf);
              // ups_level of a value in [0, 255 + 2^-15]: the magic-constant round (ups_moments.hip)
              lv[2 * p + k] = __float_as_uint(ups_lerp(tb.x, tb.y, ay) + 12582912.f) & 0xFFu;
            }
          }
          cur = vq ? (lv[0] | (lv[1] << 8) | (lv[2] << 16) | (lv[3] << 24)) : 0u;
          if (own && i < UA_RB) xrow[(int64_t)i * (W >> 2)] = cur;
        }
        um_row(ring, acc, i, j, cur, own);
      }
    }
  }
  // wave sums (exact in u32), one partial row per wave
  double out = 0.0;
#pragma unroll
  for (int k = 0; k < 42; ++k) {
    const uint32_t v = xm_wave_sum(acc[k]);
    if (lane == k) out = (double)v;
  }
  if (lane < 42) partial[((int64_t)b * units + unit) * 42 + lane] = out;
}

}  // namespace tds

using namespace tds;

// partial rows [B * units][42] the affine upsample + moments writes (the layout of
// tds_ups_moments_rows at this kernel's band height); 0 = shape unsupported
int tds_ups_affine_rows(int B, int h, int w, int H, int W) {
  if (B < 1 || B > 65535 || h < 1 || w < 1 || h * w > kUpsImg || W % 4 != 0 || W < 8 || H < 8) return 0;
  if ((int64_t)H * W > 0xFFFFFFF0LL) return 0;
  const UmGeo g = um_geo(H, W, UA_RB);
  return B * g.nband * g.nqg;
}

void tds_ups_affine_moments_u8(const uint8_t* src, const float* mats, uint8_t* x, double* partial, int nrows, int B,
                               int h, int w, int H, int W, hipStream_t st) {
  if (nrows < 1 || nrows != tds_ups_affine_rows(B, h, w, H, W)) {
    tds_launch_fail("ups_affine_moments_u8: partial row count does not match the shape");
    return;
  }
  const UmGeo g = um_geo(H, W, UA_RB);
  const size_t lds = ua_lds_bytes(h, w);
  if (lds > 65536) {  // long thin sources (up to 131 KB at 1 x 4096): past the default dynamic limit
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(ups_affine_moments_u8_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      tds_launch_fail("ups_affine_moments_u8: the framed source does not fit LDS");
      return;
    }
  }
  hipLaunchKernelGGL(ups_affine_moments_u8_kernel, dim3(g.nband * g.nqg, B), dim3(64), lds, st, src, mats, x, partial,
                     h, w, H, W, g.nqg, g.qpw);
  TDS_LAUNCH_CHECK();
}
