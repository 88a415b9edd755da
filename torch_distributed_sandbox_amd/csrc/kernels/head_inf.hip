// Inference-only fc head on a packed low-precision weight: BN2 affine + ReLU + fc over the pooled-blocked
// ya (pooled_layout.h) for 1 .. 64 classes and 1 .. 32 images in ONE pass over ya and the pack, every
// product on v_mfma_f32_16x16x32_f16 with fp32 accumulation.  The training heads (head_pb.hip,
// head_wide.hip) stream the fp32 weight, once per 8 images; in evaluation the weight is a constant, so
// it is packed once (head_inf.h: fragment order, no padding classes) as
//   "fp16": fp16(W_j 2^e_j), e_j per class from max |W_j| (W_j 2^e_j < 2^15: weights around 1e-4 stay
//           far from fp16's subnormals, 28 binades below the class's max are normal numbers), or
//   "fp8":  OCP E4M3 bytes of W 2^e_jc, e_jc per (class, channel) from that plane's max (<= 448),
//           decoded exactly to fp16 in registers (v_cvt_scalef32_pk_f16_fp8 at scale 1) for the same MFMA
// and the head reads 2 or 1 byte per weight instead of 4.
//
// MFMA: M = images (tile mt = images 16 mt .. + 15, MT <= 2), N = classes (tile t, NT = ceil(NC / 16)),
// K = the 32 positions of one pooled block.  l = lane, n = l % 16, g = l / 16: lane (n, g) holds the
// 8 K values of block row g -- A: one 16-B piece of image 16 mt + n's block, B: piece (g, class
// 16 t + n) of the pack -- and D[4 g + r][n] in register r.  Lanes whose image is >= B or whose class
// is >= NC issue no load and enter a zero operand.
//
// A operand: X = relu(a ya + b) formed in fp32 exactly as the training heads form it (TdsYaDec, one
// v_fma_mix_f32 per value, hp_relu's NaN rule), then rounded ONCE to fp16 at one power-of-two scale
// s_x: bound = max_c |a_c d| 65504 + |a_c b2_c + b_c| can not be exceeded by any X (|ya| <= 65504), and
// bound s_x < 2^15.  fp16 has 30 binades below that: an X above 2^-29 bound keeps 11 significant bits,
// anything smaller gets an absolute error of at most 2^-40 bound -- a loose bound costs nothing that
// matters.  s_x is formed by every wave from aff2 and the decode words (no host read, no extra launch).
// Positions of a block outside the Q x Q image are selected to zero on the X side (the producer leaves
// don't-care values, NaN included, there) and hold zeros in the pack.
//
// Work split: workgroup = (channel c, band of HI_BAND = 4 block rows), 4 waves; the band's blocks are
// one contiguous run of the pack (64 NC B per block) and of every image's ya plane (64 B per block);
// wave w takes blocks w, w + 4, ... of the run, HI_U = 4 blocks' loads in flight per wave.  No LDS in
// the stream: every byte is used by exactly one lane.  A wave keeps MT x NT fp32 accumulator tiles over
// its Q8 (or fewer) blocks, i.e. chains of at most 32 Q8 fp32 additions; the 4 waves' tiles meet in LDS
// and are summed in fp64, where each class column gets its 2^-e / s_x (once per workgroup: a workgroup
// stays inside one channel), and leave as one fp64 row of partials.  The last workgroup of a channel
// to arrive (tds_arrive) sums the channel's rows, the last channel sums the 32 and adds the bias:
// fixed orders, deterministic.  All indexing is 64-bit (the 62-class pack at 3000^2 is above 2 GiB).
#include <type_traits>

#include "bf16x3.h"
#include "common.h"
#include "conv2_fp8.h"
#include "head_inf.h"
#include "launchers.h"

namespace tds {

constexpr int HI_THREADS = 256;
constexpr int HI_U = 4;  // blocks in flight per wave

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// exponent e with m 2^e < 2^HI_F16_TOP (0 for m = 0 or a non-finite m)
__device__ __forceinline__ int hi_f16_exp(float m) {
  if (!(m > 0.f) || !__builtin_isfinite(m)) return 0;
  int x;
  (void)frexpf(m, &x);  // m < 2^x
  return min(HI_EXP_LIM, max(-HI_EXP_LIM, HI_F16_TOP - x));
}

// ------------------------------------------------------------------------------------------- pack
__global__ __launch_bounds__(256) void head_inf_zero_kernel(uint32_t* p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// wmx[j * 32 + c] = max |W[j][c][.]| (float bits; zeroed before): grid (chunks of a plane, NC * 32 planes)
__global__ __launch_bounds__(256) void head_inf_wmax_kernel(const float* __restrict__ W, uint32_t* __restrict__ wmx,
                                                            int64_t QQ, int chunk) {
  __shared__ uint32_t sh[4];
  const int64_t pl = blockIdx.y;
  const float* p = W + pl * QQ;
  const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(QQ, i0 + chunk);
  uint32_t m = 0u;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) m = max(m, __float_as_uint(p[i]) & 0x7fffffffu);
  m = block_max(m, sh);
  if (threadIdx.x == 0) atomicMax(wmx + pl, m);
}

// the scale exponents from the maxima: fp16 wexp[j], fp8 wexp[c * NC + j]
template <bool F8>
__global__ __launch_bounds__(256) void head_inf_exp_kernel(const uint32_t* __restrict__ wmx, int* __restrict__ wexp,
                                                           int NC) {
  if constexpr (F8) {
    for (int i = threadIdx.x; i < 32 * NC; i += 256) {
      const int c = i / NC, j = i - c * NC;
      wexp[i] = f8_scale_exp((double)__uint_as_float(wmx[j * 32 + c]));
    }
  } else {
    for (int j = threadIdx.x; j < NC; j += 256) {
      uint32_t m = 0u;
      for (int c = 0; c < 32; ++c) m = max(m, wmx[j * 32 + c]);  // (NaN bits stay on top: no scale)
      wexp[j] = hi_f16_exp(__uint_as_float(m));
    }
  }
}

// one thread per piece (head_inf.h): 8 columns of a weight row (any dword alignment), zeros outside the image
template <bool F8>
__global__ __launch_bounds__(256) void head_inf_pack_kernel(const float* __restrict__ W, const int* __restrict__ wexp,
                                                            void* __restrict__ wpk, PBGeom g, int NC, int64_t npieces) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= npieces) return;
  const int j = (int)(u % NC);
  int64_t r = u / NC;
  const int gq = (int)(r & 3);
  r >>= 2;
  const int bx = (int)(r % g.Q8);
  r /= g.Q8;
  const int R = (int)(r % g.Q4), c = (int)(r / g.Q4);
  const int Q = g.Q, py = 4 * R + gq, px = 8 * bx;
  const int e = wexp[F8 ? c * NC + j : j];
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = 0.f;
  if (py < Q) {
    const float* row = W + ((int64_t)j * 32 + c) * Q * Q + (int64_t)py * Q;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (px + k < Q) v[k] = ldexpf(row[px + k], e);
  }
  if constexpr (F8)
    reinterpret_cast<uint2*>(wpk)[u] = make_uint2(f8_pack4(v[0], v[1], v[2], v[3]), f8_pack4(v[4], v[5], v[6], v[7]));
  else
    reinterpret_cast<uint4*>(wpk)[u] =
        make_uint4(cvt2_f16(v[0], v[1]), cvt2_f16(v[2], v[3]), cvt2_f16(v[4], v[5]), cvt2_f16(v[6], v[7]));
}

// ---------------------------------------------------------------------------------------- forward
// (head_pb.hip's hp_relu / hp_fma_h / hp_ydec: the same instructions on the same values)
__device__ __forceinline__ float hi_relu(float z) { return z > 0.f ? z : (isnan(z) ? z : 0.f); }
template <int HI>
__device__ __forceinline__ float hi_fma_h(float a, uint32_t w, float c) {
  float d;
  if constexpr (HI != 0)
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(d) : "v"(a), "v"(w), "v"(c));
  else
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(d) : "v"(a), "v"(w), "v"(c));
  return d;
}
__device__ __forceinline__ float hi_ydec(const uint32_t* ysc) {
  return ysc != nullptr ? __uint_as_float(ysc[0]) * __uint_as_float(ysc[1]) / __uint_as_float(ysc[2]) : 1.f;
}

// the A operand of one piece: X s_x in fp16 for the first ncol columns, zeros after them
__device__ __forceinline__ f16x8_t hi_x(u32x4 y, float ad, float bd, float sx, int ncol) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float z0 = hi_fma_h<0>(ad, y[k], bd), z1 = hi_fma_h<1>(ad, y[k], bd);
    o[k] = cvt2_f16(2 * k < ncol ? hi_relu(z0) * sx : 0.f, 2 * k + 1 < ncol ? hi_relu(z1) * sx : 0.f);
  }
  return __builtin_bit_cast(f16x8_t, o);
}

// 8 E4M3 bytes -> 8 fp16, exact
__device__ __forceinline__ f16x8_t hi_dec8(u32x2 w) {
  const f16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.f, false);
  const f16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.f, true);
  const f16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.f, false);
  const f16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.f, true);
  return f16x8_t{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

// store(i, sum of column i over nrows rows of BN doubles), fixed order, by the whole workgroup: one round of
// loads where common.h's wide_row_sum fits (part: 256 doubles), else 16 independent loads per round
// (a reducer that walks its rows as a dependent chain pays one global round trip per row)
template <class F>
__device__ __forceinline__ void hi_sum_rows(const double* base, int nrows, int BN, double* part, F&& store) {
  if (BN <= 256 && nrows <= WRS_MAXL * (256 / BN)) {
    const double s = wide_row_sum(base, nrows, BN, BN, part);
    if ((int)threadIdx.x < BN) store((int)threadIdx.x, s);
    return;
  }
  for (int i = threadIdx.x; i < BN; i += HI_THREADS) {
    double s = 0.0;
    for (int k0 = 0; k0 < nrows; k0 += 16) {
      double v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = base[(int64_t)min(k0 + q, nrows - 1) * BN + i];  // (clamped, dropped below)
#pragma unroll
      for (int q = 0; q < 16; ++q) s += k0 + q < nrows ? v[q] : 0.0;
    }
    store(i, s);
  }
}

// partial: [32 * nband + 32][B * NC] doubles (the last 32 rows: the channel sums); sync: 33 counters
template <int MT, int NT, bool F8>
__global__ __launch_bounds__(HI_THREADS) void head_inf_fwd_kernel(const unsigned short* __restrict__ ya, TdsYaDec yd,
                                                                  const void* __restrict__ wpk,
                                                                  const int* __restrict__ wexp,
                                                                  const float* __restrict__ aff2,
                                                                  const float* __restrict__ bias, double* partial,
                                                                  float* __restrict__ logits, uint32_t* sync, PBGeom g,
                                                                  int B, int NC, int nband) {
  using Piece = std::conditional_t<F8, u32x2, u32x4>;
  __shared__ float red[4][MT * 16 * NT * 16];
  __shared__ double rsum[256];
  __shared__ int last_flag;
  const int c = (int)blockIdx.x / nband, band = (int)blockIdx.x - c * nband;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int n = lane & 15, gq = lane >> 4;
  const float dec = hi_ydec(yd.ysc);
  float sx;
  {  // s_x from the bound over all 32 channels (file header); every wave forms the same value
    const int ch = lane & 31;
    const float ac = aff2[ch];
    const float bnd = fabsf(ac * dec) * 65504.f + fabsf(fmaf(ac, yd.b2[ch], aff2[32 + ch]));
    sx = ldexpf(1.f, hi_f16_exp(__uint_as_float(wave_max(__float_as_uint(bnd)))));  // (NaN: bits above inf -> 1)
  }
  const float a = aff2[c], ad = a * dec, bd = fmaf(a, yd.b2[c], aff2[32 + c]);
  const int Q = g.Q;
  const int64_t plane = g.plane(), pc = (int64_t)c * g.Q4 * g.Q8;
  const int i0 = band * HI_BAND * g.Q8, i1 = min(g.Q4, (band + 1) * HI_BAND) * g.Q8;  // the band's blocks
  const unsigned short* yp[MT];
  bool aok[MT], jok[NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    aok[mt] = 16 * mt + n < B;
    yp[mt] = ya + ((int64_t)min(16 * mt + n, B - 1) * 32 + c) * plane + gq * 8;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    jok[t] = 16 * t + n < NC;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const Piece* wp = reinterpret_cast<const Piece*>(wpk);
#pragma unroll 1
  for (int i = i0 + wv; i < i1; i += 4 * HI_U) {
    u32x4 av[HI_U][MT];
    Piece bv[HI_U][NT];
    // every load of the HI_U blocks first (a block past the band: the band's last, not used)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int u = 0; u < HI_U; ++u) av[u][mt] = u32x4{0u, 0u, 0u, 0u};
      if (aok[mt]) {
#pragma unroll
        for (int u = 0; u < HI_U; ++u)
          av[u][mt] = *reinterpret_cast<const u32x4*>(yp[mt] + (int64_t)min(i + 4 * u, i1 - 1) * 32);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int u = 0; u < HI_U; ++u) bv[u][t] = Piece{};
      if (jok[t]) {
#pragma unroll
        for (int u = 0; u < HI_U; ++u)
          bv[u][t] = __builtin_nontemporal_load(wp + ((pc + min(i + 4 * u, i1 - 1)) * 4 + gq) * NC + 16 * t + n);
      }
    }
#pragma unroll
    for (int u = 0; u < HI_U; ++u) {
      const int iu = i + 4 * u;
      if (iu < i1) {  // (wave-uniform)
        const int R = iu / g.Q8, bx = iu - R * g.Q8;
        const int ncol = 4 * R + gq < Q ? min(8, Q - 8 * bx) : 0;  // valid columns of this lane's piece
        f16x8_t xh[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xh[mt] = hi_x(av[u][mt], ad, bd, sx, aok[mt] ? ncol : 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          f16x8_t wh;
          if constexpr (F8) wh = hi_dec8(bv[u][t]);
          else wh = __builtin_bit_cast(f16x8_t, bv[u][t]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[mt], wh, acc[mt][t], 0, 0, 0);
        }
      }
    }
  }
  // the 4 waves' tiles in a fixed order, in fp64, each class column at its 2^-e / s_x
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wv][(16 * mt + 4 * gq + r) * 16 * NT + 16 * t + n] = acc[mt][t][r];
  __syncthreads();
  const int BN = B * NC;
  const double sxinv = 1.0 / (double)sx;
  for (int i = threadIdx.x; i < BN; i += HI_THREADS) {
    const int b = i / NC, j = i - b * NC, k = b * 16 * NT + j;
    const double s = (((double)red[0][k] + (double)red[1][k]) + (double)red[2][k]) + (double)red[3][k];
    st_agent(partial + (int64_t)blockIdx.x * BN + i, s * ldexp(sxinv, -wexp[F8 ? c * NC + j : j]));
  }
  if (!tds_arrive(sync + c, (uint32_t)nband, &last_flag)) return;
  double* chp = partial + (int64_t)gridDim.x * BN;  // channel sums [32][BN]
  hi_sum_rows(partial + (int64_t)c * nband * BN, nband, BN, rsum,
              [&](int i, double s) { st_agent(chp + (int64_t)c * BN + i, s); });
  if (!tds_arrive(sync + 32, 32u, &last_flag)) return;
  hi_sum_rows(chp, 32, BN, rsum, [&](int i, double s) {
    logits[i] = (float)(s + (bias != nullptr ? (double)bias[i % NC] : 0.0));  // (one rounding)
  });
}

}  // namespace tds

using namespace tds;

static bool hi_dims_ok(int B, int Q, int NC, int kind) {
  return B >= 1 && B <= HI_MAX_B && NC >= 1 && NC <= HI_MAX_NC && Q >= 4 && Q <= 32760 &&
         (kind == kHeadInfF16 || kind == kHeadInfF8);
}

int64_t tds_head_inf_partials(int B, int Q, int NC) { return ((int64_t)32 * hi_nband(Q) + 32) * B * NC; }

int tds_head_inf_pack(const float* Wfc, void* wpk, int* wexp, uint32_t* wmx, int Q, int NC, int kind, hipStream_t st) {
  if (!hi_dims_ok(1, Q, NC, kind)) return -1;
  const PBGeom g = pb_geom(Q);
  const int64_t QQ = (int64_t)Q * Q, np = hi_pack_pieces(Q, NC);
  constexpr int kChunk = 1 << 16;
  hipLaunchKernelGGL(head_inf_zero_kernel, dim3((32 * NC + 255) / 256), dim3(256), 0, st, wmx, 32 * NC);
  TDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_inf_wmax_kernel, dim3((unsigned)((QQ + kChunk - 1) / kChunk), 32 * NC), dim3(256), 0, st, Wfc,
                     wmx, QQ, kChunk);
  TDS_LAUNCH_CHECK();
  const dim3 pgrid((unsigned)((np + 255) / 256));
  if (kind == kHeadInfF8) {
    hipLaunchKernelGGL(head_inf_exp_kernel<true>, dim3(1), dim3(256), 0, st, wmx, wexp, NC);
    TDS_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_inf_pack_kernel<true>, pgrid, dim3(256), 0, st, Wfc, wexp, wpk, g, NC, np);
  } else {
    hipLaunchKernelGGL(head_inf_exp_kernel<false>, dim3(1), dim3(256), 0, st, wmx, wexp, NC);
    TDS_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_inf_pack_kernel<false>, pgrid, dim3(256), 0, st, Wfc, wexp, wpk, g, NC, np);
  }
  TDS_LAUNCH_CHECK();
  return 0;
}

int tds_head_inf_fwd(const unsigned short* ya, TdsYaDec yd, const void* wpk, const int* wexp, const float* bias,
                     const float* aff2, double* partial, float* logits, int B, int Q, int NC, int kind, hipStream_t st) {
  if (!hi_dims_ok(B, Q, NC, kind)) return -1;
  uint32_t* sync = tds_sync_words(kSyncHeadInf, st);
  if (sync == nullptr) return -4;
  const PBGeom g = pb_geom(Q);
  const int nband = hi_nband(Q);
  auto launch = [&](auto mt, auto nt, auto f8) {
    hipLaunchKernelGGL((head_inf_fwd_kernel<decltype(mt)::value, decltype(nt)::value, decltype(f8)::value>),
                       dim3(32 * nband), dim3(HI_THREADS), 0, st, ya, yd, wpk, wexp, aff2, bias, partial, logits, sync,
                       g, B, NC, nband);
  };
  auto pick_nt = [&](auto mt, auto f8) {
    switch ((NC + 15) / 16) {
      case 1: launch(mt, std::integral_constant<int, 1>{}, f8); break;
      case 2: launch(mt, std::integral_constant<int, 2>{}, f8); break;
      case 3: launch(mt, std::integral_constant<int, 3>{}, f8); break;
      default: launch(mt, std::integral_constant<int, 4>{}, f8); break;
    }
  };
  auto pick_mt = [&](auto f8) {
    if (B <= 16) pick_nt(std::integral_constant<int, 1>{}, f8);
    else pick_nt(std::integral_constant<int, 2>{}, f8);
  };
  if (kind == kHeadInfF8) pick_mt(std::true_type{}); else pick_mt(std::false_type{});
  TDS_LAUNCH_CHECK();
  return 0;
}
