// Fused ConvNet head for 11 .. 64 classes and up to 16 images on the pooled-blocked ya / planar g2m
// (pooled_layout.h): the same operations as head_pb.hip -- BN2 affine + ReLU + fc forward, fc / ReLU
// backward up to g2m with the BN2 backward sums and the fc weight step -- with every fc product on the
// matrix pipe in exact fp32: v_mfma_f32_16x16x4_f32, fp32 operands unrounded, fp32 accumulation.
// head_pb.hip keeps classes x images accumulators per thread on VALU, which stops at ten classes;
// here a wave owns 16 x 16 tiles and the class count only sets the number of tiles NT = ceil(NC / 16).
//
// Workgroup = (channel c, band of block rows), 4 waves; wave w takes pooled row 4 R + w of each block
// row R of the band and walks it in spans of HW_SPAN = 64 columns.  l = lane, g = l / 16, n = l % 16.
// MFMA layouts: A[i][k] in lane (i = n, k = g); B[k][j] in lane (k = g, j = n); D[4 g + r][n] in
// register r of lane (g, n).
//
// Forward, per span and class tile t: M = images, N = classes, K = positions.
//   the span's K index (u, g, e), u, e = 0 .. 3, is column p0 + 16 u + 4 g + e: lane (n, g) loads the
//   4 fp16 ya values of image n and one dwordx4 of weight row 16 t + n at columns p0 + 16 u + 4 g .. + 3,
//   and MFMA step (u, e) takes element e of both.  4 loads of a class row cover one 256-B run.
//   D = logits[image 4 g + r][class 16 t + n], kept over the whole band; the 4 waves' tiles meet in
//   LDS and leave as one fp64 row of partials per workgroup; head_wide_logits_kernel sums the rows
//   in a fixed order (deterministic) and adds the bias.  max |W| per (workgroup, class) goes to
//   wmax for the backward's g2m scale.
//
// Backward, per span: lane (g, n) owns columns px = p0 + 4 n .. + 3 (element e), so a wave
// instruction reads or writes each of 4 class rows in one 256-B run.
//   w[t][s]  = dwordx4 of class 16 t + 4 g + s at px                      (16 NT VGPRs)
//   x[s][e]  = X of image 4 s + g at px + e, from one 8-B ya load per s   (s < ceil(B / 4))
//   g product  (M = images, N = the 16 columns px + e of element e, K = classes): A = dl[image(i)]
//     [16 t + 4 g + s] with image(i) = 4 (i % 4) + i / 4, B = w[t][s].e; D register r of lane (g, n) is
//     image 4 r + g at column px + e -- the image and columns of x[r][e], so the ReLU mask, the y
//     value of the BN2 sums and the 8-B fp16 g2m store need no exchange between lanes.
//   dW product (M = classes, N = columns, K = images): A = dl[4 s + g][16 t + n], B = x[s][e];
//     D register r of lane (g, n) is class 16 t + 4 g + r at px + e: over e = 0 .. 3 the dwordx4 at
//     the address w[t][r] was loaded from.  One load of W serves the g product, the SGD rule's old
//     value and the store address; dl sits in registers in both operand orders (8 NT VGPRs each).
//   Rows start at any dword (odd Q): loads are dwordx4 at 4-B alignment, stores split by the row's
//   alignment class as head_pb.hip's hp_st4 (wave-uniform: spans start at multiples of 64).
// Edges: columns >= Q, images >= B and classes >= NC enter the products as zeros (loads clamped or
// guarded per element at the row end) and are never stored.
// Registers (NT = 4): forward 64 W + 8 ya + 16 acc; backward 64 W + 8 ya + 16 X + 32 dl + 16 g
// + 16 dW (+ 16 momentum-buffer values per class tile).
#include <type_traits>

#include "bf16x3.h"
#include "common.h"
#include "launchers.h"
#include "pooled_layout.h"

namespace tds {

constexpr int HW_THREADS = 256;
constexpr int HW_BAND = 4;   // block rows per workgroup (forward; the backward's band is head_pb.hip's)
constexpr int HW_SPAN = 64;  // pooled columns per wave iteration

__device__ __forceinline__ f32x4 hw_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// (head_pb.hip's hp_relu / hp_fma_h / hp_fma4 / hp_ydec: the same instructions on the same values, so
// X is bitwise what the ten-class head forms)
__device__ __forceinline__ float hw_relu(float z) { return z > 0.f ? z : (isnan(z) ? z : 0.f); }
template <int HI>
__device__ __forceinline__ float hw_fma_h(float a, uint32_t w, float c) {
  float d;
  if constexpr (HI != 0)
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(d) : "v"(a), "v"(w), "v"(c));
  else
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(d) : "v"(a), "v"(w), "v"(c));
  return d;
}
__device__ __forceinline__ void hw_fma4(float a, uint2 y, float c, float (&o)[4]) {
  o[0] = hw_fma_h<0>(a, y.x, c);
  o[1] = hw_fma_h<1>(a, y.x, c);
  o[2] = hw_fma_h<0>(a, y.y, c);
  o[3] = hw_fma_h<1>(a, y.y, c);
}
__device__ __forceinline__ float hw_ydec(const uint32_t* ysc) {
  return ysc != nullptr ? __uint_as_float(ysc[0]) * __uint_as_float(ysc[1]) / __uint_as_float(ysc[2]) : 1.f;
}
__device__ __forceinline__ float hw_f16(uint32_t h) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)(h & 0xFFFFu));
}
__device__ __forceinline__ float hw_el(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// columns px .. px + 3 of a Q-wide row (row: its first element; any dword alignment): one dwordx4
// inside the row, guarded elements at its end, zeros past it.  FULL: the wave's whole span lies
// inside the row -- the loads of a span are then issued back to back, not one per branch
template <bool FULL>
__device__ __forceinline__ float4 hw_ld4(const float* row, int px, int Q) {
  if (FULL || px + 3 < Q) return *reinterpret_cast<const float4*>(row + px);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (px < Q) v.x = row[px];
  if (px + 1 < Q) v.y = row[px + 1];
  if (px + 2 < Q) v.z = row[px + 2];
  return v;
}

// nvalid (0 .. 4) floats at p, non-temporal; al = (element index of p) % 4, wave-uniform: no store
// straddles a 16-B granule (head_pb.hip hp_st4)
__device__ __forceinline__ void hw_st4(float* p, int al, int nvalid, float4 v) {
  if (nvalid == 4 && al == 0) {
    st_stream(reinterpret_cast<float4*>(p), v);
  } else if (nvalid == 4 && al == 2) {
    st_stream(reinterpret_cast<float2*>(p), make_float2(v.x, v.y));
    st_stream(reinterpret_cast<float2*>(p + 2), make_float2(v.z, v.w));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nvalid) st_stream(p + k, hw_el(v, k));
  }
}

// the same for 4 fp16 values (two packed pairs, element 0 low)
__device__ __forceinline__ void hw_st4h(unsigned short* p, int al, int nvalid, uint32_t lo, uint32_t hi) {
  if (nvalid == 4 && al == 0) {
    st_stream(reinterpret_cast<uint2*>(p), make_uint2(lo, hi));
  } else if (nvalid == 4 && al == 2) {
    st_stream(reinterpret_cast<uint32_t*>(p), lo);
    st_stream(reinterpret_cast<uint32_t*>(p + 2), hi);
  } else {
    const unsigned short e[4] = {(unsigned short)lo, (unsigned short)(lo >> 16), (unsigned short)hi,
                                 (unsigned short)(hi >> 16)};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nvalid) p[k] = e[k];
  }
}

// ---------------------------------------------------------------------------------------- forward
// partial[wg][B * NC] (fp64): this workgroup's share of logits[b][j]; wmax[wg][64]: its max |W[j]| as
// float bits (0 for j >= NC); wg = c * nband + band
template <int NT>
__global__ __launch_bounds__(HW_THREADS) void head_wide_fwd_kernel(const unsigned short* __restrict__ ya, TdsYaDec yd,
                                                                   const float* __restrict__ W,
                                                                   const float* __restrict__ aff2,
                                                                   double* __restrict__ partial,
                                                                   uint32_t* __restrict__ wmax, PBGeom g, int B, int NC,
                                                                   int nband) {
  __shared__ float red[4][16 * 16 * NT];
  __shared__ uint32_t wred[4][16 * NT];
  const int c = (int)blockIdx.x / nband, band = (int)blockIdx.x - c * nband;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int n = lane & 15, gq = lane >> 4;
  const float a = aff2[c], ad = a * hw_ydec(yd.ysc), bd = fmaf(a, yd.b2[c], aff2[32 + c]);
  const int Q = g.Q;
  const int64_t QQ = (int64_t)Q * Q, plane = g.plane(), cls = 32 * QQ;
  f32x4 acc[NT];
  float wmx[NT];
  const float* wj[NT];  // this lane's class rows (B operand column n), clamped
  bool jok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    wmx[t] = 0.f;
    jok[t] = 16 * t + n < NC;
    wj[t] = W + (int64_t)min(16 * t + n, NC - 1) * cls + (int64_t)c * QQ;
  }
  const bool bok = n < B;  // (A operand row n = image n)
  const unsigned short* yc = ya + ((int64_t)min(n, B - 1) * 32 + c) * plane;
  const int R1 = min(g.Q4, (band + 1) * HW_BAND);
  for (int R = band * HW_BAND; R < R1; ++R) {
    const int py = 4 * R + wv;
    if (py >= Q) break;  // (wave-uniform; the barrier below is outside the loop)
    const unsigned short* yrow = yc + (int64_t)R * g.Q8 * 32 + wv * 8;
#pragma unroll 1
    for (int p0 = 0; p0 < Q; p0 += HW_SPAN) {
      uint2 y[4];
      float4 w[NT][4];
      auto loads = [&](auto full) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int px = p0 + 16 * u + 4 * gq;
          y[u] = *reinterpret_cast<const uint2*>(yrow + (int64_t)min(px >> 3, g.Q8 - 1) * 32 + (px & 4));
#pragma unroll
          for (int t = 0; t < NT; ++t) w[t][u] = hw_ld4<decltype(full)::value>(wj[t] + (int64_t)py * Q, px, Q);
        }
      };
      if (p0 + HW_SPAN <= Q) loads(std::true_type{}); else loads(std::false_type{});
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int px = p0 + 16 * u + 4 * gq;
        float zz[4], x[4];
        hw_fma4(ad, y[u], bd, zz);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = (bok && px + e < Q) ? hw_relu(zz[e]) : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          float4 w4 = w[t][u];  // (hw_ld4 zeroed the columns past the row)
          if (!jok[t]) w4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t] = hw_mfma(x[e], hw_el(w4, e), acc[t]);
          wmx[t] = fmaxf(fmaxf(wmx[t], fmaxf(fabsf(w4.x), fabsf(w4.y))), fmaxf(fabsf(w4.z), fabsf(w4.w)));
        }
      }
    }
  }
  // the 4 waves' tiles in a fixed order; max |W| over the lane groups, then the waves
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wv][(4 * gq + r) * 16 * NT + 16 * t + n] = acc[t][r];
    uint32_t m = __float_as_uint(wmx[t]);  // (non-negative: bits order as values)
    m = max(m, (uint32_t)__shfl_xor((int)m, 16, TDS_WAVE));
    m = max(m, (uint32_t)__shfl_xor((int)m, 32, TDS_WAVE));
    if (gq == 0) wred[wv][16 * t + n] = m;
  }
  __syncthreads();
  const int64_t wg = blockIdx.x;
  for (int i = threadIdx.x; i < B * NC; i += HW_THREADS) {
    const int b = i / NC, j = i - b * NC, k = b * 16 * NT + j;
    partial[wg * B * NC + i] = (((double)red[0][k] + (double)red[1][k]) + (double)red[2][k]) + (double)red[3][k];
  }
  if ((int)threadIdx.x < 64) {
    const int j = threadIdx.x;
    wmax[wg * 64 + j] = j < 16 * NT ? max(max(wred[0][j], wred[1][j]), max(wred[2][j], wred[3][j])) : 0u;
  }
}

// logits[i] = sum_k partial[k][i] + bias[i % NC]: one workgroup per logit, fixed order
__global__ __launch_bounds__(256) void head_wide_logits_kernel(const double* __restrict__ partial, int nwg,
                                                               const float* __restrict__ bias,
                                                               float* __restrict__ logits, int BN, int NC) {
  __shared__ double sh[4];
  const int i = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < nwg; k += 256) s += partial[(int64_t)k * BN + i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) logits[i] = (float)s + (bias ? bias[i % NC] : 0.f);
}

// --------------------------------------------------------------------------------------- backward
// What head_bwd_pb_kernel hands on, for images 0 .. B-1 in one pass:
//   g2h[b][c][py][px] = fp16(2^e_c (sum_j dl[b][j] W[j][c][py][px]) [a ya + b > 0]), g2inv[c] = 2^-e_c
//     with 2^e_c from the same bound rule: sum_j |dl[b][j]| max |W[j][c][.]| < 2^14 (wmax: the
//     forward's, wrows rows per channel)
//   partial[c][band][4] = { sum g2m, sum g2m y } over the fp32 values, then over the stored ones
//   gpart[c * nband + band] = max |g2m| (float bits)
//   dW = scale dl^T X (keep), W / mbuf stepped in place (upd: plain SGD, MOM: common.h sgd_rule_step)
//   fin: the BN2 backward finalize in this launch (the last workgroup of a channel, then of all 32)
struct HWFin {
  uint32_t* sync;      // 33 counters
  uint32_t* cmax;      // [32]
  const float* stats;  // [64] mean | invstd of BN2
  const float* gamma;  // [32] or nullptr
  float* dgamma;
  float* dbeta;
  float* kbuf;         // [96] k1 | k2 | k3
  int64_t n;           // B * P * P
  float* dbfc;         // [NC]
  uint32_t* mag;       // mag[32] <- max |g2m|, or nullptr
};

// DW false: the no-dW form (the activation exchange forms the fc step from the gathered pooled
// inputs, head_wide_upd_kernel below): no dW product, no weight-layout store; everything else as is
template <int NT, bool MOM, bool DW>
__global__ __launch_bounds__(HW_THREADS) void head_wide_bwd_kernel(
    const unsigned short* __restrict__ ya, TdsYaDec yd, const float* W, const float* __restrict__ aff2,
    const float* __restrict__ dl, const uint32_t* __restrict__ wmax, int wrows, unsigned short* __restrict__ g2h,
    float* __restrict__ g2inv, double* __restrict__ partial, uint32_t* __restrict__ gpart, float* dW, float* Wupd,
    float* mbuf, PBGeom g, int B, int NC, int nband, int bandrows, float scale, float lr, SgdRule rule, HWFin fin) {
  __shared__ uint32_t wms[64];
  __shared__ float g2sc;
  __shared__ float red[4][4];
  __shared__ uint32_t gred[4];
  __shared__ double dred[4][4];
  __shared__ int last_flag;
  // workgroups in the reverse of the forward's order (head_pb.hip: the forward's last lines are
  // still in the Infinity Cache)
  const int wg = (int)gridDim.x - 1 - (int)blockIdx.x;
  const int c = wg / nband, band = wg - c * nband;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int n = lane & 15, gq = lane >> 4;
  const int ns = (B + 3) >> 2;  // K steps of the dW product / live registers of the g tiles
  // g2m's fp16 scale of channel c
  if (threadIdx.x < 64) wms[threadIdx.x] = 0u;
  __syncthreads();
  for (int i = threadIdx.x; i < wrows * 64; i += HW_THREADS)
    atomicMax(&wms[i & 63], wmax[(int64_t)c * wrows * 64 + i]);
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.f;
    if ((int)threadIdx.x < B)
      for (int j = 0; j < NC; ++j) s = fmaf(fabsf(dl[threadIdx.x * NC + j]), __uint_as_float(wms[j]), s);
    const float bound = __uint_as_float(wave_max(__float_as_uint(s)));  // (NaN: bits above inf -> no scale)
    if (threadIdx.x == 0) {
      int e = 0;
      if (bound > 0.f && __builtin_isfinite(bound)) {
        int x;
        (void)frexpf(bound, &x);  // bound < 2^x
        e = min(100, max(-100, 14 - x));
      }
      g2sc = ldexpf(1.f, e);
      if (band == 0) g2inv[c] = ldexpf(1.f, -e);
    }
  }
  __syncthreads();
  const float gsc = g2sc, ginv = 1.f / g2sc;  // (powers of two: exact)
  const float a = aff2[c], yds = hw_ydec(yd.ysc), ad = a * yds, b2c = yd.b2[c], bd = fmaf(a, b2c, aff2[32 + c]);
  const int Q = g.Q;
  const int64_t QQ = (int64_t)Q * Q, plane = g.plane(), cls = 32 * QQ;
  // dl in both operand orders (file header); zeros for images >= B and classes >= NC
  float dlg[NT][4];
  [[maybe_unused]] float dlw[NT][4];
  {
    const int ig = 4 * (n & 3) + (n >> 2);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int jg = 16 * t + 4 * gq + s, iw = 4 * s + gq, jw = 16 * t + n;
        dlg[t][s] = (ig < B && jg < NC) ? dl[ig * NC + jg] : 0.f;
        if constexpr (DW) dlw[t][s] = (iw < B && jw < NC) ? dl[iw * NC + jw] : 0.f;
      }
  }
  float sdz = 0.f, sdy = 0.f, sdzr = 0.f, sdyr = 0.f;  // (r: the stored values)
  uint32_t gmx = 0u;
  const bool keep = dW != nullptr, upd = Wupd != nullptr;
  const int R1 = min(g.Q4, (band + 1) * bandrows);
  for (int R = band * bandrows; R < R1; ++R) {
    const int py = 4 * R + wv;
    if (py >= Q) break;  // (wave-uniform; no barrier inside the loop)
    const int64_t rowoff = (int64_t)c * QQ + (int64_t)py * Q;
    const int al = __builtin_amdgcn_readfirstlane((int)(rowoff & 3));  // (cls and 64-column spans keep it)
#pragma unroll 1
    for (int p0 = 0; p0 < Q; p0 += HW_SPAN) {
      const int px = p0 + 4 * n;
      const int nvalid = max(0, min(4, Q - px));
      const bool full = p0 + HW_SPAN <= Q;  // (wave-uniform)
      float4 w[NT][4];
      uint2 y[4];
      auto wloads = [&](auto fl) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            w[t][s] = hw_ld4<decltype(fl)::value>(W + (int64_t)min(16 * t + 4 * gq + s, NC - 1) * cls + rowoff, px, Q);
      };
      if (full) wloads(std::true_type{}); else wloads(std::false_type{});
      const int64_t yoff = (((int64_t)c * g.Q4 + R) * g.Q8 + min(px >> 3, g.Q8 - 1)) * 32 + wv * 8 + (px & 4);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < ns) y[s] = *reinterpret_cast<const uint2*>(ya + (int64_t)min(4 * s + gq, B - 1) * 32 * plane + yoff);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (16 * (NT - 1) + 4 * gq + s >= NC) w[NT - 1][s] = make_float4(0.f, 0.f, 0.f, 0.f);
      // the g product: tile e = columns px + e of the 16 lanes n
      f32x4 ga[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ga[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int s = 0; s < 4; ++s) ga[e] = hw_mfma(dlg[t][s], hw_el(w[t][s], e), ga[e]);
      }
      // X, the ReLU mask, g2m and the BN2 sums: register r of the g tiles = image 4 r + g = x[r]
      [[maybe_unused]] float x[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r < ns) {
          const int b = 4 * r + gq;
          const bool iok = b < B;
          float zz[4], yy[4], gm[4];
          hw_fma4(ad, y[r], bd, zz);
          hw_fma4(yds, y[r], b2c, yy);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = iok && e < nvalid;
            x[r][e] = ok ? hw_relu(zz[e]) : 0.f;
            gm[e] = (ok && zz[e] > 0.f) ? ga[e][r] : 0.f;
            if (!ok) yy[e] = 0.f;
            sdz += gm[e];
            sdy = fmaf(gm[e], yy[e], sdy);
          }
          const uint32_t lo = cvt2_f16(gm[0] * gsc, gm[1] * gsc), hi = cvt2_f16(gm[2] * gsc, gm[3] * gsc);
          if (iok) hw_st4h(g2h + (int64_t)b * cls + rowoff + px, al, nvalid, lo, hi);
          const float gr[4] = {hw_f16(lo) * ginv, hw_f16(lo >> 16) * ginv, hw_f16(hi) * ginv, hw_f16(hi >> 16) * ginv};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            gmx = max(gmx, __float_as_uint(gr[e]) & 0x7fffffffu);
            sdzr += gr[e];
            sdyr = fmaf(gr[e], yy[e], sdyr);
          }
        }
      }
      // the dW product per class tile: register r over e = the dwordx4 w[t][r] came from
#pragma unroll
      for (int t = 0; DW && t < NT; ++t) {
        [[maybe_unused]] float4 mb[4];
        if constexpr (MOM) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float* mrow = mbuf + (int64_t)min(16 * t + 4 * gq + r, NC - 1) * cls + rowoff;
            mb[r] = rule.first ? make_float4(0.f, 0.f, 0.f, 0.f)
                               : full ? hw_ld4<true>(mrow, px, Q) : hw_ld4<false>(mrow, px, Q);
          }
        }
        f32x4 da[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          da[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (s < ns) da[e] = hw_mfma(dlw[t][s], x[s][e], da[e]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * t + 4 * gq + r;
          if (j < NC) {
            const int64_t off = (int64_t)j * cls + rowoff + px;
            const float4 d = make_float4(scale * da[0][r], scale * da[1][r], scale * da[2][r], scale * da[3][r]);
            if (keep) hw_st4(dW + off, al, nvalid, d);
            if constexpr (MOM) {
              const float4 wo = w[t][r], bo = mb[r];
              float4 bn, wn;
              wn.x = sgd_rule_step(wo.x, d.x, bo.x, rule, true, bn.x);
              wn.y = sgd_rule_step(wo.y, d.y, bo.y, rule, true, bn.y);
              wn.z = sgd_rule_step(wo.z, d.z, bo.z, rule, true, bn.z);
              wn.w = sgd_rule_step(wo.w, d.w, bo.w, rule, true, bn.w);
              hw_st4(mbuf + off, al, nvalid, bn);
              hw_st4(Wupd + off, al, nvalid, wn);
            } else if (upd) {  // torch SGD: p -= lr * g
              const float4 wo = w[t][r];
              hw_st4(Wupd + off, al, nvalid,
                     make_float4(wo.x - lr * d.x, wo.y - lr * d.y, wo.z - lr * d.z, wo.w - lr * d.w));
            }
          }
        }
      }
    }
  }
  gmx = wave_max(gmx);
  sdz = wave_sum(sdz);
  sdy = wave_sum(sdy);
  sdzr = wave_sum(sdzr);
  sdyr = wave_sum(sdyr);
  if (lane == 0) {
    red[0][wv] = sdz;
    red[1][wv] = sdy;
    red[2][wv] = sdzr;
    red[3][wv] = sdyr;
    gred[wv] = gmx;
  }
  __syncthreads();
  if (gpart != nullptr && threadIdx.x == 0)
    st_agent(gpart + (int64_t)c * nband + band, max(max(gred[0], gred[1]), max(gred[2], gred[3])));
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    const double s = (((double)red[k][0] + (double)red[k][1]) + (double)red[k][2]) + (double)red[k][3];
    st_agent(partial + ((int64_t)c * nband + band) * 4 + k, s);  // (write-through: tds_arrive)
  }
  if (fin.sync == nullptr) return;
  if (!tds_arrive(fin.sync + c, (uint32_t)nband, &last_flag)) return;
  {  // channel c: its bands in a fixed order
    double sd[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t m = 0u;
    for (int k = threadIdx.x; k < nband; k += HW_THREADS) {
      const double2 v = *reinterpret_cast<const double2*>(partial + ((int64_t)c * nband + k) * 4);
      const double2 vr = *reinterpret_cast<const double2*>(partial + ((int64_t)c * nband + k) * 4 + 2);
      sd[0] += v.x;
      sd[1] += v.y;
      sd[2] += vr.x;
      sd[3] += vr.y;
      if (gpart != nullptr) m = max(m, gpart[(int64_t)c * nband + k]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sd[i] = wave_sum(sd[i]);
    m = wave_max(m);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) dred[i][wv] = sd[i];
      gred[wv] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // (head_pb.hip HBFin / bn_bwd_finalize2_kernel: the same constants)
#pragma unroll
      for (int i = 0; i < 4; ++i) sd[i] = ((dred[i][0] + dred[i][1]) + dred[i][2]) + dred[i][3];
      st_agent(fin.cmax + c, max(max(gred[0], gred[1]), max(gred[2], gred[3])));
      const double mean = fin.stats[c], is = fin.stats[32 + c];
      const double gm = fin.gamma ? fin.gamma[c] : 1.0;
      const double sdxh = sd[1] - mean * sd[0];
      fin.dgamma[c] = (float)(is * sdxh);
      fin.dbeta[c] = (float)sd[0];
      const double sdxr = sd[3] - mean * sd[2];
      const double k2 = -gm * is * is * is * sdxr / (double)fin.n;
      fin.kbuf[c] = (float)(gm * is);
      fin.kbuf[32 + c] = (float)k2;
      fin.kbuf[64 + c] = (float)(-gm * is * sd[2] / (double)fin.n - k2 * mean);
    }
  }
  if (!tds_arrive(fin.sync + 32, 32u, &last_flag)) return;
  if (threadIdx.x < 64) {
    const uint32_t m = wave_max(threadIdx.x < 32 ? fin.cmax[threadIdx.x] : 0u);
    if (threadIdx.x == 0 && fin.mag != nullptr) fin.mag[32] = m;
  } else if ((int)threadIdx.x - 64 < NC) {
    const int j = (int)threadIdx.x - 64;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += dl[b * NC + j];
    fin.dbfc[j] = v * scale;
  }
}

// ---------------------------------------------------------------------------------- pooled update
// The activation exchange's fc step from every rank's pooled input (head_pb.hip head_upd_pb_kernel
// for 11 .. 64 classes): ya [M][32][PB] fp16 of the images m = r * B + b of all ranks, rec [ranks][128]
// the ranks' head records, dl [M][NC];
//   MODE 0: out = W - lr * scale * sum_m dl[m] (x) X_m   (out may be W: each element is read and written
//                                                         by the one lane that owns it)
//   MODE 1: out = scale * sum_m dl[m] (x) X_m
//   MODE 2: out += scale * sum_m dl[m] (x) X_m
//   MODE 3: W, mbuf = torch's SGD rule on d = scale * sum_m dl[m] (x) X_m, both in place (out = W; common.h
//           sgd_rule_step on the value MODE 1 stores; no dW is written).  The buffer tile is loaded at the
//           old weight's turn and address and stored beside it; a creating step (rule.first) loads none.
//           The rule must see the whole sum once: a single launch (<= 4 * HWU_STEPS images).  Buffer and
//           rule are one trailing argument (HWURule) that only this mode's instantiations have -- an
//           argument the other modes merely ignored would still grow their kernel-argument segment and
//           with it change how their scalar argument loads are merged.
// One product per class tile: M = classes, N = 16 pooled columns, K = the image list, four images per
// MFMA step -- the backward's dW product with its lane ownership: lane (g, n) owns columns
// px = p0 + 4 n .. + 3, in K step s it forms X of image 4 s + g there (B operand, element e) and D
// register r of tile (t, e) is class 16 t + 4 g + r at px + e: over e the dwordx4 of W / out at the
// store address.  X is formed as the head forward forms it (hw_fma4 / hw_relu on the same values)
// with the constants of the image's own rank; a K step may hold images of two ranks, so the constants
// are per image: the workgroup stages (a d, fma(a, b2, b)) of its channel per image, and dl in
// A-operand order (dls[s][t][lane] = dl[4 s + g][16 t + n], one conflict-free ds_read_b32 per tile and
// step), in LDS once.  Zeros for images >= M and classes >= NC; columns >= Q are masked in X.
// A launch holds at most 4 * HWU_STEPS images (32 KB of dl at NT = 4); the launcher runs longer lists
// in image chunks, each later chunk accumulating into what the one before left (same grid, fixed
// order: deterministic).
// Registers: 16 NT accumulators; the old values (MODE 0 / 2) are loaded tile by tile after the image
// stream -- not the backward's 64 weight registers, which its g product needs live during it; no
// wmax, no g2m, no sums.  (Tile 0's old values issued before the stream, to land under it, measured
// 0.5 % faster at 26 classes and 1.7 % slower at 62: not kept.)
// Grid = (channel, band of block rows) as the backward: nothing in it depends on the rank, every rank
// forms bitwise the same step.
constexpr int HWU_STEPS = 32;

struct HWURule {
  float* mbuf;
  SgdRule rule;
};

template <int NT, int MODE, class... RULE>  // RULE: HWURule in MODE 3, nothing otherwise
__global__ __launch_bounds__(HW_THREADS) void head_wide_upd_kernel(const unsigned short* __restrict__ ya,
                                                                   const float* __restrict__ rec,
                                                                   const float* __restrict__ dl, const float* W,
                                                                   float* out, PBGeom g, int B, int m0, int M, int NC,
                                                                   int nband, int bandrows, float scale, float lr,
                                                                   RULE... rule_arg) {
  static_assert(sizeof...(RULE) == (MODE == 3 ? 1 : 0), "the rule argument belongs to MODE 3");
  __shared__ float dls[HWU_STEPS * NT * 64];
  __shared__ float2 cst[HWU_STEPS * 4];
  const int c = (int)blockIdx.x / nband, band = (int)blockIdx.x - c * nband;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int n = lane & 15, gq = lane >> 4;
  const int ns = (M + 3) >> 2;  // K steps of this launch (images m0 .. m0 + M - 1)
  for (int i = threadIdx.x; i < 4 * ns; i += HW_THREADS) {
    float2 k = make_float2(0.f, 0.f);
    if (i < M) {  // the image's rank's constants, formed as its head kernels formed them
      const float* rr = rec + (int64_t)((m0 + i) / B) * 128;
      const float a = rr[c];
      k = make_float2(a * hw_ydec(reinterpret_cast<const uint32_t*>(rr + 64)), fmaf(a, rr[68 + c], rr[32 + c]));
    }
    cst[i] = k;
  }
  for (int i = threadIdx.x; i < ns * NT * 64; i += HW_THREADS) {
    const int l = i & 63, t = (i >> 6) % NT, s = (i >> 6) / NT;
    const int m = 4 * s + (l >> 4), j = 16 * t + (l & 15);
    dls[i] = (m < M && j < NC) ? dl[(int64_t)(m0 + m) * NC + j] : 0.f;
  }
  __syncthreads();
  const int Q = g.Q;
  const int64_t QQ = (int64_t)Q * Q, plane = g.plane(), cls = 32 * QQ;
  const float* src = (MODE == 0 || MODE == 3) ? W : out;  // the old values (MODE 1: none)
  const int R1 = min(g.Q4, (band + 1) * bandrows);
  for (int R = band * bandrows; R < R1; ++R) {
    const int py = 4 * R + wv;
    if (py >= Q) break;  // (wave-uniform; no barrier inside the loop)
    const int64_t rowoff = (int64_t)c * QQ + (int64_t)py * Q;
    const int al = __builtin_amdgcn_readfirstlane((int)(rowoff & 3));  // (cls and 64-column spans keep it)
#pragma unroll 1
    for (int p0 = 0; p0 < Q; p0 += HW_SPAN) {
      const int px = p0 + 4 * n;
      const int nvalid = max(0, min(4, Q - px));
      const bool full = p0 + HW_SPAN <= Q;  // (wave-uniform)
      f32x4 acc[NT][4];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
      const unsigned short* yp =
          ya + (((int64_t)c * g.Q4 + R) * g.Q8 + min(px >> 3, g.Q8 - 1)) * 32 + wv * 8 + (px & 4);
#pragma unroll 1
      for (int s0 = 0; s0 < ns; s0 += 4) {
        uint2 y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (s0 + u < ns)
            y[u] = *reinterpret_cast<const uint2*>(yp + (int64_t)(m0 + min(4 * (s0 + u) + gq, M - 1)) * 32 * plane);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < ns) {
            const int s = s0 + u, ml = 4 * s + gq;
            const float2 k = cst[ml];
            float zz[4], x[4];
            hw_fma4(k.x, y[u], k.y, zz);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = (ml < M && e < nvalid) ? hw_relu(zz[e]) : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              const float a = dls[(s * NT + t) * 64 + lane];
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[t][e] = hw_mfma(a, x[e], acc[t][e]);
            }
          }
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        // (NT > 2: the class stride made opaque per tile, so the tile's 4 row addresses are formed here,
        // not all 16 NT of them kept in registers across the image stream -- 3 waves per SIMD instead of
        // 2 at NT = 4 in the modes that read old values; at NT = 2 the plain form measured 4 % faster)
        int64_t tcls = cls;
        if constexpr (NT > 2) asm volatile("" : "+s"(tcls));
        [[maybe_unused]] float4 old[4];
        if constexpr (MODE != 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float* row = src + (int64_t)min(16 * t + 4 * gq + r, NC - 1) * tcls + rowoff;
            old[r] = full ? hw_ld4<true>(row, px, Q) : hw_ld4<false>(row, px, Q);
          }
        }
        [[maybe_unused]] float4 mb[4];
        if constexpr (MODE == 3) {
          const HWURule& mr = (rule_arg, ...);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float* row = mr.mbuf + (int64_t)min(16 * t + 4 * gq + r, NC - 1) * tcls + rowoff;
            mb[r] = mr.rule.first ? make_float4(0.f, 0.f, 0.f, 0.f)
                                  : full ? hw_ld4<true>(row, px, Q) : hw_ld4<false>(row, px, Q);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * t + 4 * gq + r;
          if (j < NC) {
            float* p = out + (int64_t)j * tcls + rowoff + px;
            const float4 d = make_float4(scale * acc[t][0][r], scale * acc[t][1][r], scale * acc[t][2][r],
                                         scale * acc[t][3][r]);
            if constexpr (MODE == 0) {  // torch SGD: p -= lr * g
              const float4 o = old[r];
              hw_st4(p, al, nvalid, make_float4(o.x - lr * d.x, o.y - lr * d.y, o.z - lr * d.z, o.w - lr * d.w));
            } else if constexpr (MODE == 1) {
              hw_st4(p, al, nvalid, d);
            } else if constexpr (MODE == 3) {  // torch SGD with momentum / weight decay
              const HWURule& mr = (rule_arg, ...);
              const float4 o = old[r], bo = mb[r];
              float4 bn, wn;
              wn.x = sgd_rule_step(o.x, d.x, bo.x, mr.rule, true, bn.x);
              wn.y = sgd_rule_step(o.y, d.y, bo.y, mr.rule, true, bn.y);
              wn.z = sgd_rule_step(o.z, d.z, bo.z, mr.rule, true, bn.z);
              wn.w = sgd_rule_step(o.w, d.w, bo.w, mr.rule, true, bn.w);
              hw_st4(mr.mbuf + (int64_t)j * tcls + rowoff + px, al, nvalid, bn);
              hw_st4(p, al, nvalid, wn);
            } else {
              const float4 o = old[r];
              hw_st4(p, al, nvalid, make_float4(o.x + d.x, o.y + d.y, o.z + d.z, o.w + d.w));
            }
          }
        }
      }
    }
  }
}

}  // namespace tds

using namespace tds;

static bool hw_dims_ok(int B, int Q, int NC) { return B >= 1 && B <= 16 && NC >= 11 && NC <= 64 && Q >= 4; }

int tds_head_wide_nblk(int Q) { return (pb_geom(Q).Q4 + HW_BAND - 1) / HW_BAND; }

int tds_head_wide_fwd(const unsigned short* ya, TdsYaDec yd, const float* Wfc, const float* bias, const float* aff2,
                      double* partial, uint32_t* wmax, float* logits, int B, int Q, int NC, hipStream_t st) {
  if (!hw_dims_ok(B, Q, NC)) return -1;
  const PBGeom g = pb_geom(Q);
  const int nband = tds_head_wide_nblk(Q), nwg = 32 * nband;
  auto launch = [&](auto nt) {
    hipLaunchKernelGGL((head_wide_fwd_kernel<decltype(nt)::value>), dim3(nwg), dim3(HW_THREADS), 0, st, ya, yd, Wfc, aff2,
                       partial, wmax, g, B, NC, nband);
  };
  switch ((NC + 15) / 16) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    default: launch(std::integral_constant<int, 4>{}); break;
  }
  TDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_wide_logits_kernel, dim3(B * NC), dim3(256), 0, st, partial, nwg, bias, logits, B * NC, NC);
  TDS_LAUNCH_CHECK();
  return 0;
}

int tds_head_wide_bwd(const unsigned short* ya, TdsYaDec yd, const float* Wfc, const float* aff2, const float* dlogits,
                      const uint32_t* wmax, unsigned short* g2m, float* g2inv, double* partial, uint32_t* gpart,
                      float* dW, float* Wupd, int B, int Q, int NC, float scale, float lr, hipStream_t st,
                      const TdsHeadBwdFin* hf, const TdsHeadMom* hm) {
  if (!hw_dims_ok(B, Q, NC)) return -1;
  if (hm != nullptr && (hm->buf == nullptr || Wupd == nullptr || !(lr > 0.f))) return -3;
  const PBGeom g = pb_geom(Q);
  // the band of head_pb.hip's backward: the step's magnitude workspace holds one gpart word per
  // (channel, band) of that grid
  const int nband = tds_head_bwd_pb_nblk(Q), bandrows = (g.Q4 + nband - 1) / nband;
  HWFin fin{};
  if (hf != nullptr) {
    fin.sync = tds_sync_words(kSyncHeadWide, st);
    if (fin.sync == nullptr) return -4;
    fin.cmax = hf->cmax;
    fin.stats = hf->stats;
    fin.gamma = hf->gamma;
    fin.dgamma = hf->dgamma;
    fin.dbeta = hf->dbeta;
    fin.kbuf = hf->kbuf;
    fin.n = (int64_t)B * (2 * Q) * (2 * Q);
    fin.dbfc = hf->dbfc;
    fin.mag = hf->mag;
  }
  const SgdRule rule = hm == nullptr ? SgdRule{}
                                     : SgdRule::make(lr, hm->wd, hm->momentum, hm->dampening, hm->nesterov ? 1 : 0,
                                                     hm->first_step ? 1 : 0);
  float* mbuf = hm != nullptr ? hm->buf : nullptr;
  // neither dW nor Wupd: the no-dW form (the fc step comes from tds_head_wide_upd)
  auto launch = [&](auto nt, auto mom, auto dw) {
    hipLaunchKernelGGL((head_wide_bwd_kernel<decltype(nt)::value, decltype(mom)::value, decltype(dw)::value>),
                       dim3(32 * nband), dim3(HW_THREADS), 0, st, ya, yd, Wfc, aff2, dlogits, wmax,
                       tds_head_wide_nblk(Q), g2m, g2inv, partial, gpart, dW, Wupd, mbuf, g, B, NC, nband, bandrows,
                       scale, lr, rule, fin);
  };
  auto pick = [&](auto mom, auto dw) {
    switch ((NC + 15) / 16) {
      case 1: launch(std::integral_constant<int, 1>{}, mom, dw); break;
      case 2: launch(std::integral_constant<int, 2>{}, mom, dw); break;
      case 3: launch(std::integral_constant<int, 3>{}, mom, dw); break;
      default: launch(std::integral_constant<int, 4>{}, mom, dw); break;
    }
  };
  if (hm != nullptr) pick(std::true_type{}, std::true_type{});
  else if (dW != nullptr || Wupd != nullptr) pick(std::false_type{}, std::true_type{});
  else pick(std::false_type{}, std::false_type{});
  TDS_LAUNCH_CHECK();
  return 0;
}

int tds_head_wide_upd(const unsigned short* ya_all, const float* rec, int nranks, const float* dl, const float* W,
                      float* out, int B, int Q, int NC, float scale, float lr, int mode, hipStream_t st,
                      const TdsHeadMom* hm) {
  if (!hw_dims_ok(B, Q, NC) || nranks < 1 || nranks > (1 << 20) || mode < 0 || mode > 2) return -1;
  const PBGeom g = pb_geom(Q);
  const int nband = tds_head_bwd_pb_nblk(Q), bandrows = (g.Q4 + nband - 1) / nband;
  const int Mall = nranks * B;
  // the rule form: mode 0's in-place step with its buffer, in the one launch that holds the whole sum
  if (hm != nullptr && (hm->buf == nullptr || mode != 0 || out != W || !(lr > 0.f) || Mall > 4 * HWU_STEPS)) return -2;
  const HWURule rule{hm != nullptr ? hm->buf : nullptr,
                     hm == nullptr ? SgdRule{}
                                   : SgdRule::make(lr, hm->wd, hm->momentum, hm->dampening, hm->nesterov ? 1 : 0,
                                                   hm->first_step ? 1 : 0)};
  for (int m0 = 0; m0 < Mall; m0 += 4 * HWU_STEPS) {
    // image chunks after the first go on from what the one before wrote: the stepped weight, or += into dW
    const int M = min(4 * HWU_STEPS, Mall - m0), md = m0 == 0 ? mode : (mode == 0 ? 0 : 2);
    const float* Wsrc = m0 == 0 ? W : out;
    auto launch = [&](auto nt, auto mdc) {
      constexpr int NT = decltype(nt)::value, MODE = decltype(mdc)::value;
      if constexpr (MODE == 3)
        hipLaunchKernelGGL((head_wide_upd_kernel<NT, MODE, HWURule>), dim3(32 * nband), dim3(HW_THREADS), 0, st, ya_all,
                           rec, dl, Wsrc, out, g, B, m0, M, NC, nband, bandrows, scale, lr, rule);
      else
        hipLaunchKernelGGL((head_wide_upd_kernel<NT, MODE>), dim3(32 * nband), dim3(HW_THREADS), 0, st, ya_all, rec, dl,
                           Wsrc, out, g, B, m0, M, NC, nband, bandrows, scale, lr);
    };
    auto pick = [&](auto mdc) {
      switch ((NC + 15) / 16) {
        case 1: launch(std::integral_constant<int, 1>{}, mdc); break;
        case 2: launch(std::integral_constant<int, 2>{}, mdc); break;
        case 3: launch(std::integral_constant<int, 3>{}, mdc); break;
        default: launch(std::integral_constant<int, 4>{}, mdc); break;
      }
    };
    if (hm != nullptr) pick(std::integral_constant<int, 3>{});
    else if (md == 0) pick(std::integral_constant<int, 0>{});
    else if (md == 1) pick(std::integral_constant<int, 1>{});
    else pick(std::integral_constant<int, 2>{});
    TDS_LAUNCH_CHECK();
  }
  return 0;
}
