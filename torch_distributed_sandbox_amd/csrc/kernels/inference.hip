// The inference plan's small launches (models/convnet_fused.py forward_inference, trainer.evaluate):
//   * inference_constants_kernel: the BN1 / BN2 affines from the RUNNING statistics and p1's fp16
//     range guard, in the forms the training kernels' consumers read (l1_conv_bf3_kernel's aff[33],
//     the head's aff2[64], the conv2 kernels' mag[kMagScales + 1]).  Reads the BN buffers, writes none.
//   * x_absmax_kernel: max |x| of an fp32 batch (the guard's bound on the input; uint8 levels are
//     bounded by 255 without a read).
//   * eval_metrics_kernel: cross-entropy sum, correct count and sample count of one batch's logits
//     added to a device accumulator, so an evaluation loop never synchronises with the host.
#include <algorithm>

#include "ce_small.h"
#include "conv2_common.h"
#include "launchers.h"

namespace tds {

// uint8 level input: x = level / 255 in fp32 (convnet_fused.hip L1_LEVEL_SCALE)
constexpr float INF_LEVEL_SCALE = 1.f / 255.f;
constexpr int XAM_THREADS = 256, XAM_PER = 8;  // float4 loads per thread and grid stride

// per-workgroup max |x| as float bits (|x| >= 0 orders as its bits do; a NaN is above every finite
// value and survives to the constants kernel, which then leaves p1 unscaled)
__global__ __launch_bounds__(XAM_THREADS) void x_absmax_kernel(const float4* __restrict__ x, int64_t n4,
                                                               uint32_t* __restrict__ part) {
  __shared__ uint32_t sh[XAM_THREADS / TDS_WAVE];
  uint32_t m = 0u;
  const int64_t stride = (int64_t)gridDim.x * XAM_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * XAM_THREADS + threadIdx.x; e < n4; e += stride * XAM_PER) {
    float4 v[XAM_PER];
#pragma unroll
    for (int u = 0; u < XAM_PER; ++u) v[u] = x[min(e + u * stride, n4 - 1)];  // (clamped: a repeat leaves the max)
#pragma unroll
    for (int u = 0; u < XAM_PER; ++u) {
      m = max(m, max(__float_as_uint(v[u].x) & 0x7fffffffu, __float_as_uint(v[u].y) & 0x7fffffffu));
      m = max(m, max(__float_as_uint(v[u].z) & 0x7fffffffu, __float_as_uint(v[u].w) & 0x7fffffffu));
    }
  }
  m = block_max(m, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// One workgroup.  BN1: a = gamma * rsqrt(running_var + eps), b = beta - running_mean * a, both times
// p1_scale; BN2: aff2 = [a | b] unscaled.  p1's range guard: training bounds p1 by Samuelson's
// inequality on the BATCH statistics (convnet_fused.hip l1_gram_body), which says nothing about the
// running ones; here, per channel and for any input with |x| <= xmax,
//   |p1_c| <= |a_c| (sum_k |w1_ck| xmax + |b1_c - running_mean_c|) + |beta_c|
// with the same 2^-10 margin, the same power-of-two choice and the same hand-off (aff1[32] = p1_scale,
// *p1inv = 1 / p1_scale where the conv2 kernels read it).
__global__ __launch_bounds__(256) void inference_constants_kernel(
    const uint32_t* __restrict__ xpart, int nxp, float xmax_fixed, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ g1, const float* __restrict__ be1,
    const float* __restrict__ rm1, const float* __restrict__ rv1, float eps1, const float* __restrict__ g2,
    const float* __restrict__ be2, const float* __restrict__ rm2, const float* __restrict__ rv2, float eps2,
    float* __restrict__ aff1, float* __restrict__ aff2, uint32_t* __restrict__ p1inv) {
  __shared__ uint32_t sh[4];
  const int tid = threadIdx.x;
  float xmax = xmax_fixed;
  if (xpart != nullptr) {  // (kernel-uniform)
    uint32_t m = 0u;
    for (int i = tid; i < nxp; i += 256) m = max(m, xpart[i]);
    xmax = __uint_as_float(block_max(m, sh));
  }
  if (tid < 64) {  // wave 0
    const int c = tid & 15;
    const float a = g1[c] * (float)(1.0 / sqrt((double)rv1[c] + (double)eps1));
    double bound = 0.0;
    if (tid < 16) {
      double l1 = 0.0;
      for (int k = 0; k < 25; ++k) l1 += fabs((double)w1[c * 25 + k]);
      bound = fabs((double)a) * (l1 * (double)xmax + fabs((double)b1[c] - (double)rm1[c])) + fabs((double)be1[c]);
    }
    for (int off = 32; off > 0; off >>= 1) bound = fmax(bound, __shfl_xor(bound, off, 64));
    bound *= 1.0 + 1.0 / 1024.0;
    int e1 = 0;
    if (bound > 65504.0 && __builtin_isfinite(bound)) {
      int x;
      (void)frexp(bound / 65504.0, &x);  // bound / 65504 < 2^x
      e1 = -min(x, 120);
    }
    const float p1_scale = ldexpf(1.f, e1);
    if (tid == 0) {
      aff1[32] = p1_scale;
      *p1inv = __float_as_uint(1.f / p1_scale);
    }
    if (tid < 16) {
      aff1[c] = a * p1_scale;
      aff1[16 + c] = (be1[c] - rm1[c] * a) * p1_scale;
    }
  } else if (tid < 96) {
    const int c = tid - 64;
    const float a = g2[c] * (float)(1.0 / sqrt((double)rv2[c] + (double)eps2));
    aff2[c] = a;
    aff2[32 + c] = be2[c] - rm2[c] * a;
  }
}

// acc: [0] the fp64 sum of the per-sample losses (ce_small.h's row body, no label smoothing), [1]
// the samples whose argmax is the label, [2] the samples counted (labels equal to ignore_index are
// skipped).  argmax as torch.argmax breaks ties (the lowest index); a row holding a NaN counts as
// wrong.  One workgroup, a wave per row; launches on one stream are ordered, so the accumulator
// takes plain read-modify-writes by one thread.
__global__ __launch_bounds__(256) void eval_metrics_kernel(const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels, int M, int N,
                                                           int64_t ignore_index, unsigned long long* __restrict__ acc) {
  __shared__ double shl[4];
  __shared__ unsigned long long shc[4], shn[4];
  const int lane = lane_id(), wv = wave_id(), nw = blockDim.x / TDS_WAVE;
  double ls = 0.0;
  unsigned long long nc = 0ull, nn = 0ull;
  for (int row = wv; row < M; row += nw) {
    const float* z = logits + (int64_t)row * N;
    const int64_t lab = labels[row];
    bool valid;
    const float loss = ce_row_loss(z, N, lab, ignore_index, 0.f, lane, valid);
    float best = -INFINITY;
    int bi = INT32_MAX;  // (a lane without an element: loses every tie)
    bool nan = false;
    for (int j = lane; j < N; j += TDS_WAVE) {
      const float v = z[j];
      nan |= v != v;
      if (bi == INT32_MAX || v > best) {  // (j ascends: the lane keeps its lowest index of a tie)
        best = v;
        bi = j;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    const bool any_nan = __builtin_amdgcn_ballot_w64(nan) != 0;
    if (valid) {  // (wave-uniform; every lane keeps the same sums, lane 0's are used)
      ls += (double)loss;
      nn += 1ull;
      nc += (!any_nan && (int64_t)bi == lab) ? 1ull : 0ull;
    }
  }
  if (lane == 0) {
    shl[wv] = ls;
    shc[wv] = nc;
    shn[wv] = nn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0.0;
    unsigned long long c = 0ull, n = 0ull;
    for (int i = 0; i < nw; ++i) {  // fixed order
      l += shl[i];
      c += shc[i];
      n += shn[i];
    }
    double* accl = reinterpret_cast<double*>(acc);
    accl[0] += l;
    acc[1] += c;
    acc[2] += n;
  }
}

}  // namespace tds

using namespace tds;

int tds_x_absmax_num_wg(int64_t n4) {
  const int64_t per = (int64_t)XAM_THREADS * XAM_PER;
  return (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n4 + per - 1) / per));
}

void tds_x_absmax(const float* x, int64_t n4, uint32_t* part, int nwg, hipStream_t st) {
  hipLaunchKernelGGL(x_absmax_kernel, dim3(nwg), dim3(XAM_THREADS), 0, st, reinterpret_cast<const float4*>(x), n4, part);
  TDS_LAUNCH_CHECK();
}

void tds_inference_constants(const uint32_t* xpart, int nxp, const float* w1, const float* b1, const float* g1,
                             const float* be1, const float* rm1, const float* rv1, float eps1, const float* g2,
                             const float* be2, const float* rm2, const float* rv2, float eps2, float* aff1, float* aff2,
                             uint32_t* mag, hipStream_t st) {
  hipLaunchKernelGGL(inference_constants_kernel, dim3(1), dim3(256), 0, st, xpart, nxp, 255.f * INF_LEVEL_SCALE, w1, b1,
                     g1, be1, rm1, rv1, eps1, g2, be2, rm2, rv2, eps2, aff1, aff2, mag + kMagScales + 1);
  TDS_LAUNCH_CHECK();
}

void tds_eval_metrics(const float* logits, const int64_t* labels, int M, int N, int64_t ignore_index,
                      unsigned long long* acc, hipStream_t st) {
  hipLaunchKernelGGL(eval_metrics_kernel, dim3(1), dim3(256), 0, st, logits, labels, M, N, ignore_index, acc);
  TDS_LAUNCH_CHECK();
}
