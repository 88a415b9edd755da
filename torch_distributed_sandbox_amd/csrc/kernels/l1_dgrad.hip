// Layer-1 input gradient dL/dx of the fused plan (docs/KERNELS.md "Layer 1: input gradient").
//
// With dz_c the pooled gradient routed to each window's argmax where the ReLU passes (the idx1 byte),
// BN1's batch-statistics backward is dy_c = A_c dz_c + B_c (y_c - b1_c) + C_c, and
//   dx[q] = sum_c sum_{t : q - t inside the image} w_c[t] dy_c[q - t]
//         = sum_c sum_t (A_c w_c[t]) dz_c[q - t]      sparse: one non-zero per window and channel
//         + (K2^class(q) * x)[q]                       x has one channel: sum_c B_c w_c^T * (w_c * x) is ONE
//                                                      9 x 9 filter on x, y1 is never rebuilt
//         + K0^class(q)                                constant per border class
// (class: which taps t keep q - t inside the image, 5 per axis).
//
//   l1_dgrad_coef_kernel : A, B, C from the layer-1 backward's fp64 sums; the 25 x 81 K2 tables, the
//                          25 K0, and G_c[t] = A_c w_c[t] as an fp16 hi + lo pair at one power-of-two
//                          scale.  fp64 arithmetic, fp32 / fp16 stores.  25 workgroups, one per class.
//   l1_dgrad_kernel      : persistent workgroups over 16 x 16 tiles of dx.
//     1. the tile's 10 x 16 pooled windows (1 window of halo: dz within +-2 pixels contributes) become
//        a DENSE fp16 dz tile in LDS, [20 rows][32 cols][16 channels]: a thread takes 4 windows x 8
//        channels and places each stored fp16 value at its argmax slot with one 64-bit shift;
//     2. T[pixel][tap] = sum_c dz_c[pixel] G_c[tap] on v_mfma_f32_16x16x32_f16: M = 16 pixels, N = 25
//        taps in two blocks, K = 32 = 16 channels x (hi, lo): the A operand repeats dz, the B operand
//        holds G's hi in k < 16 and its lo in k >= 16, so ONE MFMA forms dz (hi + lo), dz exact as
//        stored, G to 22 bits.  B lives in 8 registers for the whole kernel.  T (400 pixels x 25 taps,
//        fp32) goes to LDS at a pixel stride of 25 words (odd: a tap's column is conflict-free);
//     3. one thread per output pixel: the 25-tap shift-add dx[q] += T[q - t][t], then the 81-tap K2
//        filter on the staged x window in fp32 FMA -- interior tiles on the interior table through
//        wave-uniform loads, tiles that touch an image edge on the per-pixel class tables -- and K0;
//        four neighbours meet in one lane for a 16-byte non-temporal store.
// No atomics anywhere: dx is a pure function of its inputs, bit for bit.
#include <algorithm>

#include "bf16x3.h"
#include "launchers.h"

namespace tds {

// 64 zero bytes: the source of every staged vector that lies outside the image
__device__ __attribute__((aligned(16))) uint4 g_l1d_zero[4] = {};

constexpr int LD_T = 16;               // tile side (output pixels)
constexpr int LD_ZR = LD_T + 4;        // dz rows / needed dz columns (halo 2)
constexpr int LD_ZC = 32;              // dz tile columns: 4 dp1h column groups of 4 windows
constexpr int LD_ZOFF = 6;             // dz tile column of full-resolution column c0 - 2
constexpr int LD_XR = LD_T + 8;        // x window side (halo 4)
constexpr int LD_NPIX = LD_ZR * LD_ZR; // pixels of T
constexpr int LD_TS = 25;              // T pixel stride (words)
constexpr int LD_DZ_BYTES = LD_ZR * LD_ZC * 32, LD_X_BYTES = LD_XR * LD_XR * 4, LD_T_BYTES = LD_NPIX * LD_TS * 4;
static_assert(LD_NPIX % 16 == 0, "T in whole MFMA row blocks");
static_assert(LD_DZ_BYTES + LD_X_BYTES + LD_T_BYTES <= 65536, "l1_dgrad LDS");

// coefficient buffer (floats): K2[25][81] | K0[25] | 1 / G scale | pad | G halves [hi, lo][32 taps][16 ch] fp16
constexpr int LD_K0 = 25 * 81, LD_GINV = LD_K0 + 25, LD_G = LD_GINV + 2, LD_COEF = LD_G + 2 * 32 * 16 / 2;
static_assert(LD_G % 4 == 0, "G fragments are read as 16-byte vectors");

// valid tap range [lo, hi] (centred, -2..2) of a border class on one axis: classes 0, 1 the first two
// lines, 2 the interior, 3, 4 the last two
__device__ __forceinline__ void ld_class_range(int cls, int& lo, int& hi) {
  lo = cls == 3 ? -1 : cls == 4 ? 0 : -2;
  hi = cls == 0 ? 0 : cls == 1 ? 1 : 2;
}
__device__ __forceinline__ int ld_class(int q, int n) { return q < 2 ? q : q >= n - 2 ? q - (n - 5) : 2; }

__global__ __launch_bounds__(256) void l1_dgrad_coef_kernel(const double* __restrict__ bwd_sum,
                                                            const float* __restrict__ w1,
                                                            const float* __restrict__ b1,
                                                            const float* __restrict__ gamma1,
                                                            const float* __restrict__ stats1, int64_t n,
                                                            float* __restrict__ coef) {
  __shared__ double sw[400], sa[16], sb[16], sc[16], smax[4];
  const int t = threadIdx.x, cls = blockIdx.x;
  for (int i = t; i < 400; i += 256) sw[i] = (double)w1[i];
  __syncthreads();
  if (t < 16) {
    // the sums l1_finalize_one reads: [0] sum dz, [2 + k] sum dz xpatch_k (decoded, fp64)
    const double* acc = bwd_sum + t * 27;
    const double mean = stats1[t], is = stats1[16 + t], gm = gamma1 ? (double)gamma1[t] : 1.0;
    const double sdz = acc[0];
    double sdzy = (double)b1[t] * sdz;
    for (int k = 0; k < 25; ++k) sdzy += sw[t * 25 + k] * acc[2 + k];
    const double dgamma = is * (sdzy - mean * sdz);
    const double A = gm * is, Bc = -gm * is * is * dgamma / (double)n;
    sa[t] = A;
    sb[t] = Bc;
    sc[t] = -A * sdz / (double)n + Bc * ((double)b1[t] - mean);
  }
  __syncthreads();
  int rlo, rhi, clo, chi;
  ld_class_range(cls / 5, rlo, rhi);
  ld_class_range(cls % 5, clo, chi);
  if (t < 81) {
    // K2[d] = sum_c B_c sum_{t valid, s = t + d a tap} w_c[t] w_c[s]
    const int dy = t / 9 - 4, dx = t % 9 - 4;
    double k2 = 0.0;
    for (int c = 0; c < 16; ++c) {
      double s = 0.0;
      for (int ty = rlo; ty <= rhi; ++ty)
        for (int tx = clo; tx <= chi; ++tx) {
          const int sy = ty + dy, sx = tx + dx;
          if (sy >= -2 && sy <= 2 && sx >= -2 && sx <= 2)
            s += sw[c * 25 + (ty + 2) * 5 + tx + 2] * sw[c * 25 + (sy + 2) * 5 + sx + 2];
        }
      k2 += sb[c] * s;
    }
    coef[cls * 81 + t] = (float)k2;
  } else if (t == 96) {
    double k0 = 0.0;
    for (int c = 0; c < 16; ++c) {
      double s = 0.0;
      for (int ty = rlo; ty <= rhi; ++ty)
        for (int tx = clo; tx <= chi; ++tx) s += sw[c * 25 + (ty + 2) * 5 + tx + 2];
      k0 += sc[c] * s;
    }
    coef[LD_K0 + cls] = (float)k0;
  }
  if (cls != 0) return;
  // G_c[t] = A_c w_c[t] at the power of two that puts max |G| in [2^14, 2^15): fp16 hi + lo
  double gmax = 0.0;
  for (int i = t; i < 400; i += 256) gmax = fmax(gmax, fabs(sa[i / 25] * sw[i]));
  gmax = block_max(gmax, smax);
  int k = 0;
  if (gmax > 0.0 && gmax < 1e300) k = 14 - ilogb(gmax);
  k = k < -120 ? -120 : k > 120 ? 120 : k;
  if (t == 0) coef[LD_GINV] = ldexpf(1.f, -k);
  _Float16* gh = reinterpret_cast<_Float16*>(coef + LD_G);
  for (int i = t; i < 32 * 16; i += 256) {
    const int tap = i / 16, c = i % 16;
    const double g = tap < 25 ? ldexp(sa[c] * sw[c * 25 + tap], k) : 0.0;
    const _Float16 hi = (_Float16)(float)g;
    gh[i] = hi;
    gh[32 * 16 + i] = (_Float16)(float)(g - (double)(float)hi);
  }
}

__global__ __launch_bounds__(256, 2) void l1_dgrad_kernel(const float* __restrict__ x, const uint4* __restrict__ dp1,
                                                          const uint32_t* __restrict__ dp1_dec,
                                                          const uint8_t* __restrict__ idx1,
                                                          const float* __restrict__ coef, float* __restrict__ dx,
                                                          int B, int H, int W) {
  __shared__ __attribute__((aligned(16))) char lds[LD_DZ_BYTES + LD_X_BYTES + LD_T_BYTES];
  uint4* dzs = reinterpret_cast<uint4*>(lds);  // [row 20][col 32][channel octet 2] x 8 fp16
  float* xs = reinterpret_cast<float*>(lds + LD_DZ_BYTES);
  float* ts = reinterpret_cast<float*>(lds + LD_DZ_BYTES + LD_X_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
  const int P = H / 2, PW = W / 2, PG = (PW + 3) >> 2;
  const int tiles_r = (H + LD_T - 1) / LD_T, tiles_c = (W + LD_T - 1) / LD_T;
  const int total = B * tiles_r * tiles_c;
  const float dec = __uint_as_float(dp1_dec[0]), ginv = coef[LD_GINV];
  const char* zero = reinterpret_cast<const char*>(g_l1d_zero);

  // B operand: lane (tap n = 16 blk + li, k = 8 g .. 8 g + 7) = G hi (g < 2) or lo (g >= 2) of channels
  // 8 (g & 1) .. + 7
  s16x8 bfrag[2];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
    bfrag[blk] = __builtin_bit_cast(
        s16x8, reinterpret_cast<const uint4*>(coef + LD_G)[((g >> 1) * 32 + 16 * blk + li) * 2 + (g & 1)]);

  // staging roles: tid < 80 builds the dz of (pooled row lr, column group lg, channel octet o);
  // tid < 144 loads x vector (row xr, vector xv)
  const int o = tid & 1, lg = (tid >> 1) & 3, lr = tid >> 3;
  const int xr = tid / 6, xv = tid - 6 * xr;
  // the output pixel of this thread
  const int orow = tid >> 4, ocol = tid & 15;

  for (int t = blockIdx.x; t < total; t += gridDim.x) {
    const int b = t / (tiles_r * tiles_c), rem = t - b * (tiles_r * tiles_c);
    const int tr = rem / tiles_c, tc = rem - tr * tiles_c;
    const int r0 = tr * LD_T, c0 = tc * LD_T, pr0 = r0 >> 1, pc0 = c0 >> 1;
    // ---- loads: one unconditional load per vector, out-of-range vectors from the zero block
    uint4 dpv[4];
    uint2 idv[4];
    uint4 xvec;
    {
      const int prow = pr0 - 1 + lr, grp = (pc0 >> 2) - 1 + lg;
      const bool okg = (tid < 80) & ((uint32_t)prow < (uint32_t)P) & ((uint32_t)grp < (uint32_t)PG);
      const char* dsrc = okg ? reinterpret_cast<const char*>(dp1) + ((int64_t)(b * P + prow) * PG + grp) * 128 + o * 64
                             : zero;
#pragma unroll
      for (int j = 0; j < 4; ++j) dpv[j] = reinterpret_cast<const uint4*>(dsrc)[j];
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        const int pcol = 4 * grp + px;
        const bool ok = okg & (pcol < PW);
        const char* isrc = ok ? reinterpret_cast<const char*>(idx1) + ((int64_t)(b * P + prow) * PW + pcol) * 16 + o * 8
                              : zero;
        idv[px] = *reinterpret_cast<const uint2*>(isrc);
      }
      const int gr = r0 - 4 + xr, gc = c0 - 4 + 4 * xv;
      const bool okx = (tid < LD_XR * 6) & ((uint32_t)gr < (uint32_t)H) & ((uint32_t)gc < (uint32_t)W);
      const char* xsrc = okx ? reinterpret_cast<const char*>(x + ((int64_t)(b * H + gr) * W + gc)) : zero;
      xvec = *reinterpret_cast<const uint4*>(xsrc);
    }
    __syncthreads();  // the previous tile's readers are done
    if (tid < LD_XR * 6) *reinterpret_cast<uint4*>(xs + xr * LD_XR + 4 * xv) = xvec;
    if (tid < 80) {
      // value (channel 8 o + 2 j + h, window px) = half-word 4 h + px of dpv[j]; its byte of the argmax
      // record: slot in bits 0-1, ReLU mask in bit 2.  The window's four slots are the half-words of
      // hb << 16 * slot; a vector of the dense tile is one slot of 8 channels.
      const uint32_t* dw = reinterpret_cast<const uint32_t*>(dpv);
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        uint32_t out[4][4] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const uint32_t word = dw[4 * (i >> 1) + 2 * (i & 1) + (px >> 1)];
          const uint32_t ab = ((i < 4 ? idv[px].x : idv[px].y) >> (8 * (i & 3))) & 0xFFu;
          const uint32_t relu = (uint32_t)((int32_t)(ab << 29) >> 31);
          const uint32_t hb = ((px & 1) ? word >> 16 : word & 0xFFFFu) & relu;
          const uint64_t h64 = (uint64_t)hb << (16u * (ab & 3u));
#pragma unroll
          for (int s = 0; s < 4; ++s)
            out[s][i >> 1] |= (uint32_t)((h64 >> (16 * s)) & 0xFFFFu) << (16 * (i & 1));
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
          dzs[((2 * lr + (s >> 1)) * LD_ZC + 8 * lg + 2 * px + (s & 1)) * 2 + o] =
              make_uint4(out[s][0], out[s][1], out[s][2], out[s][3]);
      }
    }
    __syncthreads();
    // ---- T = dz G: M block mb = pixels 16 mb .. + 15 of the 20 x 20 region, row-major
    for (int mb = wv; mb < LD_NPIX / 16; mb += 4) {
      const int p = 16 * mb + li, pr = p / LD_ZR, pc = p - pr * LD_ZR;
      const s16x8 a = __builtin_bit_cast(s16x8, dzs[(pr * LD_ZC + pc + LD_ZOFF) * 2 + (g & 1)]);
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        const f32x4 acc = mfma_f16(a, bfrag[blk], f32x4{0.f, 0.f, 0.f, 0.f});
        const int tap = 16 * blk + li;
        if (tap < 25) {
#pragma unroll
          for (int r = 0; r < 4; ++r) ts[(16 * mb + 4 * g + r) * LD_TS + tap] = acc[r];
        }
      }
    }
    __syncthreads();
    // ---- dx[q] = sum_t T[q - t][t] (decoded once) + K2 * x + K0
    float sp = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) sp += ts[((orow + 4 - ky) * LD_ZR + ocol + 4 - kx) * LD_TS + ky * 5 + kx];
    const int gr = r0 + orow, gc = c0 + ocol;
    float dn = 0.f, k0;
    const float* xw = xs + orow * LD_XR + ocol;
    if (r0 >= 2 && c0 >= 2 && r0 + LD_T + 2 <= H && c0 + LD_T + 2 <= W) {  // wave-uniform: interior table
      const float* k2 = coef + 12 * 81;
#pragma unroll
      for (int iy = 0; iy < 9; ++iy)
#pragma unroll
        for (int ix = 0; ix < 9; ++ix) dn = fmaf(k2[iy * 9 + ix], xw[iy * LD_XR + ix], dn);
      k0 = coef[LD_K0 + 12];
    } else {
      // (pixels past the image in a partial tile take a clamped class; they are not stored)
      const int cls = ld_class(min(gr, H - 1), H) * 5 + ld_class(min(gc, W - 1), W);
      const float* k2 = coef + cls * 81;
      for (int iy = 0; iy < 9; ++iy)
#pragma unroll
        for (int ix = 0; ix < 9; ++ix) dn = fmaf(k2[iy * 9 + ix], xw[iy * LD_XR + ix], dn);
      k0 = coef[LD_K0 + cls];
    }
    const float v = (sp * ginv) * dec + dn + k0;
    // lanes 4 j .. 4 j + 3 hold 4 consecutive pixels of a row: one 16-byte store from lane 4 j
    const float v1 = __shfl_down(v, 1, 4), v2 = __shfl_down(v, 2, 4), v3 = __shfl_down(v, 3, 4);
    if ((ocol & 3) == 0 && gr < H && gc < W)
      st_stream(reinterpret_cast<float4*>(dx + ((int64_t)(b * H + gr) * W + gc)), make_float4(v, v1, v2, v3));
  }
}

}  // namespace tds

using namespace tds;

int tds_l1_dgrad_coef_numel() { return LD_COEF; }

void tds_l1_dgrad(const float* x, const void* dp1h, const uint32_t* dp1_dec, const uint8_t* idx1, const double* bwd_sum,
                  const float* w1, const float* b1, const float* gamma1, const float* stats1, float* coef, float* dx,
                  int B, int H, int W, hipStream_t st) {
  if (B < 1 || H < 8 || W < 8 || H % 2 != 0 || W % 4 != 0) {
    tds_launch_fail("l1_dgrad: needs H, W >= 8, H even and W % 4 == 0");
    return;
  }
  hipLaunchKernelGGL(l1_dgrad_coef_kernel, dim3(25), dim3(256), 0, st, bwd_sum, w1, b1, gamma1, stats1,
                     (int64_t)B * H * W, coef);
  TDS_LAUNCH_CHECK();
  const int64_t tiles = (int64_t)B * ((H + LD_T - 1) / LD_T) * ((W + LD_T - 1) / LD_T);
  if (tiles > 0x7FFFFFFFLL) {
    tds_launch_fail("l1_dgrad: too many tiles");
    return;
  }
  const int nwg = (int)std::min<int64_t>(tiles, (int64_t)tds_fused_num_wg(2));
  hipLaunchKernelGGL(l1_dgrad_kernel, dim3(nwg), dim3(256), 0, st, x, static_cast<const uint4*>(dp1h), dp1_dec, idx1,
                     coef, dx, B, H, W);
  TDS_LAUNCH_CHECK();
}
