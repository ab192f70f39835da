// Per-sample completion metrics of one Chamfer result in one launch: what calc_cd(calc_f1=True) and
// calc_dcd (utils/loss_utils.py:98-155, metrics/CD/fscore.py:3-16) compute from chamfer(gt, output)'s
// (dist1, dist2, idx1, idx2) with ~50 scalar / elementwise torch launches (sqrt, mean, compare,
// scatter_add_, gather, pow, exp ...) and a second Chamfer search.  n_lambda == 1 only.
//
// One workgroup per sample, the two directions one after the other:
//   1. hit counts: a histogram of 32-bit bins, integer atomics (order-free), in LDS up to
//      kMetricsLdsBins targets, else in the caller's workspace (zeroed here, by this workgroup);
//   2. one pass over the direction's points: every thread sums its stride-kMetricsThreads points
//      serially in index order (sqrt d, d, the density term, and the integer count of d < threshold),
//      the 64 lanes of a wave combine by the xor butterfly (32, 16, ... 1), wave 0's thread 0 adds the
//      waves' partial sums in wave order.
// Nothing is shared between workgroups (no float atomics, no global counters), so a sample's row is
// the same bits run to run and whatever else the batch holds.
//
// The means are `sum * (1.0f / n)`: that is what torch's GPU mean computes (MeanOps projects
// acc * factor, factor = 1 / n in fp32), so precision_1 / precision_2 / f1 equal metrics.fscore on the
// same distances bit for bit (the count of points below the threshold is an exact integer either way).
#include "common.h"

namespace {

constexpr int kMetricsThreads = 1024;
constexpr int kMetricsWaves = kMetricsThreads / PC_WAVE;
constexpr int kMetricsLdsBins = 32768;   // 32768 bins x 4 B = 128 KB of LDS

struct DirSums {
  float l1, l2, term;   // mean(sqrt d), mean(d), mean(1 - exp(-alpha d) w)
  float p;              // count(d < threshold) / n
};

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, PC_WAVE);
  return v;
}

// bins: T counters (LDS, or global when GLOBAL); red: 4 * kMetricsWaves words of LDS.  Every thread
// of the workgroup returns the same sums.
template <bool GLOBAL>
__device__ __forceinline__ DirSums metrics_direction(const float *__restrict__ d, const int *__restrict__ idx, int n,
                                                     int T, float threshold, float alpha, float frac,
                                                     unsigned *bins, float *red) {
  const int tid = threadIdx.x;
  for (int j = tid; j < T; j += kMetricsThreads) bins[j] = 0u;
  if (GLOBAL) __threadfence();
  __syncthreads();
  for (int i = tid; i < n; i += kMetricsThreads) {
    const int j = idx[i];
    if ((unsigned)j < (unsigned)T) atomicAdd(&bins[j], 1u);   // an out-of-range index counts no hit
  }
  if (GLOBAL) __threadfence();
  __syncthreads();
  float s1 = 0.f, s2 = 0.f, st = 0.f;
  int below = 0;
  for (int i = tid; i < n; i += kMetricsThreads) {
    const float x = d[i];
    const int j = idx[i];
    unsigned hits = 0u;
    if ((unsigned)j < (unsigned)T)
      hits = GLOBAL ? __hip_atomic_load(&bins[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : bins[j];
    const float w = 1.0f / ((float)hits + 1e-6f) * frac;
    s1 += sqrtf(x);
    s2 += x;
    st += 1.0f - expf(-x * alpha) * w;
    below += x < threshold ? 1 : 0;
  }
  s1 = wave_sum_f32(s1);
  s2 = wave_sum_f32(s2);
  st = wave_sum_f32(st);
  below = wave_sum_i32(below);
  __syncthreads();   // red may still be read from the other direction
  if ((tid & (PC_WAVE - 1)) == 0) {
    float *r = red + 4 * (tid / PC_WAVE);
    r[0] = s1;
    r[1] = s2;
    r[2] = st;
    r[3] = __int_as_float(below);
  }
  __syncthreads();
  s1 = s2 = st = 0.f;
  below = 0;
  for (int w = 0; w < kMetricsWaves; ++w) {   // wave order, the same on every thread
    s1 += red[4 * w];
    s2 += red[4 * w + 1];
    st += red[4 * w + 2];
    below += __float_as_int(red[4 * w + 3]);
  }
  const float inv_n = 1.0f / (float)n;
  DirSums r;
  r.l1 = s1 * inv_n;
  r.l2 = s2 * inv_n;
  r.term = st * inv_n;
  r.p = (float)below * inv_n;
  return r;
}

template <bool GLOBAL>
__global__ __launch_bounds__(kMetricsThreads) void completion_metrics_kernel(
    const float *__restrict__ dist1, const int *__restrict__ idx1, const float *__restrict__ dist2,
    const int *__restrict__ idx2, int N, int M, float threshold, float alpha, float frac1, float frac2,
    unsigned *ws, size_t ws_bins, float *__restrict__ out) {
  extern __shared__ unsigned metrics_bins[];
  __shared__ float red[4 * kMetricsWaves];
  const int b = blockIdx.x;
  unsigned *bins = GLOBAL ? ws + (size_t)b * ws_bins : metrics_bins;
  // dist1 / idx1: every gt point's nearest output point (M targets); dist2 / idx2: the reverse
  const DirSums a = metrics_direction<GLOBAL>(dist1 + (size_t)b * N, idx1 + (size_t)b * N, N, M, threshold, alpha,
                                              frac1, bins, red);
  const DirSums c = metrics_direction<GLOBAL>(dist2 + (size_t)b * M, idx2 + (size_t)b * M, M, N, threshold, alpha,
                                              frac2, bins, red);
  if (threadIdx.x == 0) {
    float *o = out + (size_t)b * PCOPS_METRICS_COLS;
    float f1 = 2.0f * a.p * c.p / (a.p + c.p);
    if (f1 != f1) f1 = 0.f;
    o[PCOPS_METRICS_L1A] = a.l1;
    o[PCOPS_METRICS_L1B] = c.l1;
    o[PCOPS_METRICS_L2A] = a.l2;
    o[PCOPS_METRICS_L2B] = c.l2;
    o[PCOPS_METRICS_CD_P] = (a.l1 + c.l1) / 2.0f;
    o[PCOPS_METRICS_CD_T] = a.l2 + c.l2;
    o[PCOPS_METRICS_P1] = a.p;
    o[PCOPS_METRICS_P2] = c.p;
    o[PCOPS_METRICS_F1] = f1;
    o[PCOPS_METRICS_T1] = a.term;
    o[PCOPS_METRICS_T2] = c.term;
    o[PCOPS_METRICS_DCD] = (a.term + c.term) / 2.0f;
  }
}

// ---- counted clouds (pcops_completion_metrics_counts): per-cloud n = counts1[b] / m = counts2[b],
// clamped to [0, N] / [0, M]; the rows are strided by the padded N / M.  Everything else is the
// kernel above on cloud b's valid rows: the bins cover the m (n) valid targets only, and the
// density fractions are this cloud's fp32(double(m) / double(n)) and its inverse (max(1, .) when
// non_reg) -- what the uniform entry's caller passes for equal sizes.  A cloud pair with an empty
// side gets an all-NaN row, so a tally over the batch cannot absorb it silently.
__device__ __forceinline__ int metrics_count(const int *cnt, int b, int n) {
  return cnt ? min(max(cnt[b], 0), n) : n;
}

template <bool GLOBAL>
__global__ __launch_bounds__(kMetricsThreads) void completion_metrics_counts_kernel(
    const float *__restrict__ dist1, const int *__restrict__ idx1, const float *__restrict__ dist2,
    const int *__restrict__ idx2, const int *__restrict__ cnt1, const int *__restrict__ cnt2, int N, int M,
    float threshold, float alpha, int non_reg, unsigned *ws, size_t ws_bins, float *__restrict__ out) {
  extern __shared__ unsigned metrics_bins[];
  __shared__ float red[4 * kMetricsWaves];
  const int b = blockIdx.x;
  const int n = metrics_count(cnt1, b, N), m = metrics_count(cnt2, b, M);
  float *o = out + (size_t)b * PCOPS_METRICS_COLS;
  if (n == 0 || m == 0) {
    if (threadIdx.x < PCOPS_METRICS_COLS) o[threadIdx.x] = __int_as_float(0x7FC00000);
    return;
  }
  float f12 = (float)((double)m / (double)n), f21 = (float)((double)n / (double)m);
  if (non_reg) f12 = fmaxf(1.f, f12), f21 = fmaxf(1.f, f21);
  unsigned *bins = GLOBAL ? ws + (size_t)b * ws_bins : metrics_bins;
  const DirSums a = metrics_direction<GLOBAL>(dist1 + (size_t)b * N, idx1 + (size_t)b * N, n, m, threshold, alpha,
                                              f21, bins, red);
  const DirSums c = metrics_direction<GLOBAL>(dist2 + (size_t)b * M, idx2 + (size_t)b * M, m, n, threshold, alpha,
                                              f12, bins, red);
  if (threadIdx.x == 0) {
    float f1 = 2.0f * a.p * c.p / (a.p + c.p);
    if (f1 != f1) f1 = 0.f;
    o[PCOPS_METRICS_L1A] = a.l1;
    o[PCOPS_METRICS_L1B] = c.l1;
    o[PCOPS_METRICS_L2A] = a.l2;
    o[PCOPS_METRICS_L2B] = c.l2;
    o[PCOPS_METRICS_CD_P] = (a.l1 + c.l1) / 2.0f;
    o[PCOPS_METRICS_CD_T] = a.l2 + c.l2;
    o[PCOPS_METRICS_P1] = a.p;
    o[PCOPS_METRICS_P2] = c.p;
    o[PCOPS_METRICS_F1] = f1;
    o[PCOPS_METRICS_T1] = a.term;
    o[PCOPS_METRICS_T2] = c.term;
    o[PCOPS_METRICS_DCD] = (a.term + c.term) / 2.0f;
  }
}

// The per-cloud means the counted Chamfer losses are formed from, in the summation order of
// metrics_direction (so column 0..3 equal the counted metrics row's l1a, l1b, l2a, l2b bit for
// bit): out[b] = (mean sqrt d1, mean sqrt d2, mean d1, mean d2) over cloud b's valid rows; a pair
// with an empty side gives zeros (its loss contribution).  One workgroup per cloud pair.
__device__ __forceinline__ void counts_means_direction(const float *__restrict__ d, int n, float *red, float &l1,
                                                       float &l2) {
  const int tid = threadIdx.x;
  float s1 = 0.f, s2 = 0.f;
  for (int i = tid; i < n; i += kMetricsThreads) {
    const float x = d[i];
    s1 += sqrtf(x);
    s2 += x;
  }
  s1 = wave_sum_f32(s1);
  s2 = wave_sum_f32(s2);
  __syncthreads();   // red may still be read from the other direction
  if ((tid & (PC_WAVE - 1)) == 0) {
    red[2 * (tid / PC_WAVE)] = s1;
    red[2 * (tid / PC_WAVE) + 1] = s2;
  }
  __syncthreads();
  s1 = s2 = 0.f;
  for (int w = 0; w < kMetricsWaves; ++w) {   // wave order, the same on every thread
    s1 += red[2 * w];
    s2 += red[2 * w + 1];
  }
  const float inv_n = 1.0f / (float)n;
  l1 = s1 * inv_n;
  l2 = s2 * inv_n;
}

__global__ __launch_bounds__(kMetricsThreads) void chamfer_counts_means_kernel(
    const float *__restrict__ dist1, const float *__restrict__ dist2, const int *__restrict__ cnt1,
    const int *__restrict__ cnt2, int N, int M, float *__restrict__ out) {
  __shared__ float red[2 * kMetricsWaves];
  const int b = blockIdx.x;
  const int n = metrics_count(cnt1, b, N), m = metrics_count(cnt2, b, M);
  float *o = out + (size_t)b * 4;
  if (n == 0 || m == 0) {
    if (threadIdx.x < 4) o[threadIdx.x] = 0.f;
    return;
  }
  float a1, a2, c1, c2;
  counts_means_direction(dist1 + (size_t)b * N, n, red, a1, a2);
  counts_means_direction(dist2 + (size_t)b * M, m, red, c1, c2);
  if (threadIdx.x == 0) o[0] = a1, o[1] = c1, o[2] = a2, o[3] = c2;
}

}  // namespace

extern "C" unsigned long long pcops_completion_metrics_workspace_bytes(int B, int N, int M) {
  if (B <= 0 || N <= 0 || M <= 0) return 0;
  const int T = N > M ? N : M;
  return T <= kMetricsLdsBins ? 0ull : (unsigned long long)B * (unsigned long long)T * sizeof(unsigned);
}

extern "C" int pcops_completion_metrics(const float *dist1, const int *idx1, const float *dist2, const int *idx2,
                                        int B, int N, int M, float threshold, float alpha, float frac1, float frac2,
                                        float *out, void *workspace, unsigned long long workspace_bytes,
                                        pcops_stream_t stream) {
  if (B <= 0 || N <= 0 || M <= 0) return PCOPS_ERR_INVALID;
  if (!dist1 || !idx1 || !dist2 || !idx2 || !out) return PCOPS_ERR_INVALID;
  const int T = N > M ? N : M;
  if (T > kMetricsLdsBins) {
    if (!workspace || workspace_bytes < pcops_completion_metrics_workspace_bytes(B, N, M)) return PCOPS_ERR_WORKSPACE;
    hipLaunchKernelGGL(completion_metrics_kernel<true>, dim3(B), dim3(kMetricsThreads), 0, (hipStream_t)stream, dist1,
                       idx1, dist2, idx2, N, M, threshold, alpha, frac1, frac2, (unsigned *)workspace, (size_t)T, out);
    PC_CHECK_LAUNCH();
    return PCOPS_OK;
  }
  static const hipError_t attr = hipFuncSetAttribute((const void *)completion_metrics_kernel<false>,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      kMetricsLdsBins * (int)sizeof(unsigned));
  if (attr != hipSuccess) return PCOPS_ERR_LAUNCH;
  hipLaunchKernelGGL(completion_metrics_kernel<false>, dim3(B), dim3(kMetricsThreads), (size_t)T * sizeof(unsigned),
                     (hipStream_t)stream, dist1, idx1, dist2, idx2, N, M, threshold, alpha, frac1, frac2,
                     (unsigned *)nullptr, (size_t)0, out);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

// pcops_completion_metrics over counted clouds; the workspace (pcops_completion_metrics_workspace_bytes
// of the padded sizes) is needed when max(N, M) exceeds the LDS bins, whatever the counts are.
extern "C" int pcops_completion_metrics_counts(const float *dist1, const int *idx1, const float *dist2,
                                               const int *idx2, const int *counts1, const int *counts2, int B, int N,
                                               int M, float threshold, float alpha, int non_reg, float *out,
                                               void *workspace, unsigned long long workspace_bytes,
                                               pcops_stream_t stream) {
  if (B < 0 || N <= 0 || M <= 0) return PCOPS_ERR_INVALID;
  if (B == 0) return PCOPS_OK;
  if (!counts1 && !counts2) return PCOPS_ERR_INVALID;
  if (!dist1 || !idx1 || !dist2 || !idx2 || !out) return PCOPS_ERR_INVALID;
  const int T = N > M ? N : M;
  if (T > kMetricsLdsBins) {
    if (!workspace || workspace_bytes < pcops_completion_metrics_workspace_bytes(B, N, M)) return PCOPS_ERR_WORKSPACE;
    hipLaunchKernelGGL(completion_metrics_counts_kernel<true>, dim3(B), dim3(kMetricsThreads), 0, (hipStream_t)stream,
                       dist1, idx1, dist2, idx2, counts1, counts2, N, M, threshold, alpha, non_reg,
                       (unsigned *)workspace, (size_t)T, out);
    PC_CHECK_LAUNCH();
    return PCOPS_OK;
  }
  static const hipError_t attr = hipFuncSetAttribute((const void *)completion_metrics_counts_kernel<false>,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      kMetricsLdsBins * (int)sizeof(unsigned));
  if (attr != hipSuccess) return PCOPS_ERR_LAUNCH;
  hipLaunchKernelGGL(completion_metrics_counts_kernel<false>, dim3(B), dim3(kMetricsThreads),
                     (size_t)T * sizeof(unsigned), (hipStream_t)stream, dist1, idx1, dist2, idx2, counts1, counts2, N,
                     M, threshold, alpha, non_reg, (unsigned *)nullptr, (size_t)0, out);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

// out (B, 4): per cloud pair (mean sqrt d1, mean sqrt d2, mean d1, mean d2) over the valid rows
extern "C" int pcops_chamfer_counts_means(const float *dist1, const float *dist2, const int *counts1,
                                          const int *counts2, int B, int N, int M, float *out,
                                          pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 0) return PCOPS_ERR_INVALID;
  if (B == 0) return PCOPS_OK;
  if (!counts1 && !counts2) return PCOPS_ERR_INVALID;
  if ((N && !dist1) || (M && !dist2) || !out) return PCOPS_ERR_INVALID;
  hipLaunchKernelGGL(chamfer_counts_means_kernel, dim3(B), dim3(kMetricsThreads), 0, (hipStream_t)stream, dist1, dist2,
                     counts1, counts2, N, M, out);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}
