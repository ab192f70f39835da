// GeoSpecNet's SpectralAdapter pooling (models/GeoSpecNet.py:68-105) for gfx950.
//
// The reference gathers the K neighbours' features to (B, N, K, C), permutes to
// (B, C, N, K), multiplies by the DCT-II basis W, scales by the per-channel
// frequency gates g, multiplies by W^T and sums over K with the geometric
// softmax weights a: two skinny matmuls, a repeat, a broadcast multiply and a
// sum over four full-size temporaries.  W is orthonormal, so the inverse DCT
// followed by the weighted sum is a dot product with the DCT of the weights:
//   ahat[b,n,m]   = sum_k W[k,m] a[b,n,k]
//   Xhat[b,n,c,m] = sum_j x[b, idx[b,n,j], c] W[j,m]
//   out[b,n,c]    = sum_m g[c,m] ahat[b,n,m] Xhat[b,n,c,m]
// x is token-major (B, N, C): a neighbour is one contiguous row, a thread owns
// a channel, loads coalesce over channels.  fp32 VALU work (K^2 FMAs per
// output), launch-bound at the model's shape (B*N = 1536 points).
//
// Backward, for dout[b,n,c]:
//   dg[c,m]   = sum_{b,n} dout ahat[b,n,m] Xhat[b,n,c,m]
//   da[b,n,k] = sum_m W[k,m] sum_c dout g[c,m] Xhat[b,n,c,m]
//   dx[b,p,c] = sum_{(n,j): idx[b,n,j] = p} dout[b,n,c] sum_m W[j,m] g[c,m] ahat[b,n,m]
// in three launches, each output element stored exactly once, no fill, no
// atomics, every sum in a fixed order:
//   spectral_bwd_kernel   a chunk of points per block: recomputes Xhat, reduces
//                         da over channels (wave DPP sums, then the block's
//                         waves in order), keeps the chunk's dg in registers and
//                         writes it as partial [chunk][m][c]; ahat goes to the
//                         workspace for the dx pass
//   spectral_dg_kernel    sums the partials over chunks in ascending order
//   spectral_dx_kernel    gather form: one block per destination point (b, p)
//                         scans idx[b] from LDS 64 entries at a time (ballot) and
//                         accumulates the matches in ascending (n, j) order
// An index outside [0, N) is never dereferenced: its feature counts as zero
// in forward and backward, and it matches no destination in the dx scan.
#include "common.h"

namespace {

constexpr int SP_PMAX = 16;     // points per backward chunk, at most
constexpr int SP_CHUNKS = 256;  // chunks aimed at (one per CU) before SP_PMAX caps the chunk

__device__ __forceinline__ float sp_ld(const void *p, int dt, long long i) {
  return dt == 0 ? reinterpret_cast<const float *>(p)[i] : (float)reinterpret_cast<const __bf16 *>(p)[i];
}
__device__ __forceinline__ void sp_st(void *p, int dt, long long i, float v) {
  if (dt == 0)
    reinterpret_cast<float *>(p)[i] = v;
  else
    reinterpret_cast<__bf16 *>(p)[i] = (__bf16)v;
}

__host__ __device__ inline int sp_points_per_chunk(long long BN) {
  long long p = (BN + SP_CHUNKS - 1) / SP_CHUNKS;
  return (int)(p < 1 ? 1 : (p > SP_PMAX ? SP_PMAX : p));
}

// one block per point (b, n); thread c (+ blockDim.x ...) owns channel c
template <int K>
__global__ __launch_bounds__(256) void spectral_fwd_kernel(const void *__restrict__ x, int xdt,
                                                           const int *__restrict__ idx, const float *__restrict__ a,
                                                           const float *__restrict__ g, const float *__restrict__ basis,
                                                           int N, int C, void *__restrict__ out) {
  __shared__ float sW[K * K], sa[K], sah[K];
  __shared__ int sidx[K];
  const long long pt = blockIdx.x;  // b * N + n
  const long long b = pt / N;
  const int t = threadIdx.x;
  for (int i = t; i < K * K; i += blockDim.x) sW[i] = basis[i];
  if (t < K) {
    sa[t] = a[pt * K + t];
    const int v = idx[pt * K + t];
    sidx[t] = (v >= 0 && v < N) ? v : -1;
  }
  __syncthreads();
  if (t < K) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) s = __builtin_fmaf(sW[k * K + t], sa[k], s);
    sah[t] = s;
  }
  __syncthreads();
  const long long xb = b * N * (long long)C;
  for (int c = t; c < C; c += blockDim.x) {
    float v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int q = sidx[j];
      v[j] = q >= 0 ? sp_ld(x, xdt, xb + (long long)q * C + c) : 0.f;
    }
    float o = 0.f;
#pragma unroll
    for (int m = 0; m < K; ++m) {
      float xh = 0.f;
#pragma unroll
      for (int j = 0; j < K; ++j) xh = __builtin_fmaf(v[j], sW[j * K + m], xh);
      o = __builtin_fmaf(g[(long long)c * K + m] * sah[m], xh, o);
    }
    sp_st(out, xdt, pt * C + c, o);
  }
}

// one block per chunk of P consecutive points; all lanes stay active through the wave sums
template <int K>
__global__ __launch_bounds__(256) void spectral_bwd_kernel(const void *__restrict__ x, int xdt,
                                                           const void *__restrict__ dout, int ddt,
                                                           const int *__restrict__ idx, const float *__restrict__ a,
                                                           const float *__restrict__ g, const float *__restrict__ basis,
                                                           long long BN, int N, int C, int P, float *__restrict__ da,
                                                           float *__restrict__ ahat, float *__restrict__ dgp) {
  __shared__ float sW[K * K], sah[SP_PMAX * K], sacc[SP_PMAX * 4 * K];
  __shared__ int sidx[SP_PMAX * K];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = blockDim.x >> 6;
  const long long p0 = (long long)blockIdx.x * P;
  const int np = (int)((BN - p0) < P ? (BN - p0) : P);
  for (int i = t; i < K * K; i += blockDim.x) sW[i] = basis[i];
  for (int i = t; i < np * K; i += blockDim.x) {
    const int v = idx[p0 * K + i];
    sidx[i] = (v >= 0 && v < N) ? v : -1;
  }
  for (int i = t; i < SP_PMAX * 4 * K; i += blockDim.x) sacc[i] = 0.f;
  __syncthreads();
  for (int i = t; i < np * K; i += blockDim.x) {  // ahat[p][m] = sum_k W[k][m] a[p][k]
    const int p = i / K, m = i % K;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) s = __builtin_fmaf(sW[k * K + m], a[(p0 + p) * K + k], s);
    sah[i] = s;
    ahat[p0 * K + i] = s;
  }
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += blockDim.x) {
    const int c = c0 + t;
    const bool live = c < C;
    float gk[K], dg[K];
#pragma unroll
    for (int m = 0; m < K; ++m) {
      gk[m] = live ? g[(long long)c * K + m] : 0.f;
      dg[m] = 0.f;
    }
    for (int p = 0; p < np; ++p) {
      const long long pt = p0 + p;
      const long long xb = (pt / N) * N * (long long)C;
      const float d = live ? sp_ld(dout, ddt, pt * C + c) : 0.f;
      float v[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int q = sidx[p * K + j];
        v[j] = (live && q >= 0) ? sp_ld(x, xdt, xb + (long long)q * C + c) : 0.f;
      }
#pragma unroll
      for (int m = 0; m < K; ++m) {
        float xh = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) xh = __builtin_fmaf(v[j], sW[j * K + m], xh);
        const float dxh = d * xh;
        dg[m] = __builtin_fmaf(dxh, sah[p * K + m], dg[m]);
        const float s = wave_sum_f32_dpp(dxh * gk[m]);  // over this wave's 64 channels
        if (lane == 0) sacc[(p * 4 + w) * K + m] += s;  // the slot belongs to this wave
      }
    }
    if (live) {
#pragma unroll
      for (int m = 0; m < K; ++m) dgp[((long long)blockIdx.x * K + m) * C + c] = dg[m];
    }
  }
  __syncthreads();
  for (int i = t; i < np * K; i += blockDim.x) {  // the block's waves, in order
    const int p = i / K, m = i % K;
    float s = sacc[(p * 4) * K + m];
    for (int ww = 1; ww < nw; ++ww) s += sacc[(p * 4 + ww) * K + m];
    sah[i] = s;  // ahat is no longer read
  }
  __syncthreads();
  for (int i = t; i < np * K; i += blockDim.x) {  // da[p][k] = sum_m W[k][m] s[p][m]
    const int p = i / K, k = i % K;
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < K; ++m) s = __builtin_fmaf(sW[k * K + m], sah[p * K + m], s);
    da[p0 * K + i] = s;
  }
}

// dg[c][m] = sum over chunks (ascending) of dgp[chunk][m][c]
__global__ __launch_bounds__(256) void spectral_dg_kernel(const float *__restrict__ dgp, int chunks, int K, int C,
                                                          float *__restrict__ dg) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)K * C) return;
  const int m = (int)(e / C), c = (int)(e % C);
  float s = 0.f;
  for (int ch = 0; ch < chunks; ++ch) s += dgp[(long long)ch * K * C + e];
  dg[(long long)c * K + m] = s;
}

// one block per destination point (b, p); dynamic LDS: idx[b] (N*K ints)
template <int K>
__global__ __launch_bounds__(256) void spectral_dx_kernel(const void *__restrict__ dout, int ddt,
                                                          const int *__restrict__ idx, const float *__restrict__ g,
                                                          const float *__restrict__ basis,
                                                          const float *__restrict__ ahat, int N, int C,
                                                          void *__restrict__ dx, int xdt) {
  extern __shared__ int sidx_all[];  // the whole 64 KiB at N*K = 16384: no static LDS beside it
  const long long pt = blockIdx.x;
  const long long b = pt / N;
  const int p = (int)(pt - b * N);
  const int t = threadIdx.x, lane = t & 63;
  const int NK = N * K;
  for (int i = t; i < NK; i += blockDim.x) sidx_all[i] = idx[b * NK + i];
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += blockDim.x) {
    const int c = c0 + t;
    const bool live = c < C;
    float gk[K];
#pragma unroll
    for (int m = 0; m < K; ++m) gk[m] = live ? g[(long long)c * K + m] : 0.f;
    float acc = 0.f;
    for (int e0 = 0; e0 < NK; e0 += 64) {
      const int e = e0 + lane;
      unsigned long long hit = __ballot(e < NK && sidx_all[e] == p);
      while (hit) {  // wave-uniform: ascending (n, j)
        const int f = e0 + (int)__builtin_ctzll(hit);
        hit &= hit - 1;
        const int n = f / K, j = f % K;
        const float *ah = ahat + (b * N + n) * K, *wj = basis + j * K;  // both wave-uniform
        float tj = 0.f;
#pragma unroll
        for (int m = 0; m < K; ++m) tj = __builtin_fmaf(wj[m] * ah[m], gk[m], tj);
        if (live) acc = __builtin_fmaf(sp_ld(dout, ddt, (b * N + n) * C + c), tj, acc);
      }
    }
    if (live) sp_st(dx, xdt, pt * C + c, acc);
  }
}

bool sp_eligible(int B, int N, int K, int C) {
  return (K == 4 || K == 8 || K == 16 || K == 32) && (long long)N * K <= 16384 && C >= 1 && B >= 1 && N >= 1;
}

int sp_threads(int C) { return C >= 256 ? 256 : (C + 63) / 64 * 64; }

}  // namespace

extern "C" unsigned long long pcops_spectral_pool_workspace_bytes(int B, int N, int K, int C) {
  if (B <= 0 || N <= 0 || K <= 0 || C <= 0) return 0;
  const long long BN = (long long)B * N;
  const int P = sp_points_per_chunk(BN);
  const long long chunks = (BN + P - 1) / P;
  return (unsigned long long)(BN * K + chunks * K * C) * sizeof(float);
}

extern "C" int pcops_spectral_pool_forward(const void *x, int x_dtype, const int *idx, const float *a, const float *g,
                                           const float *basis, int B, int N, int K, int C, void *out,
                                           pcops_stream_t stream) {
  if (B < 0 || N < 0 || K <= 0 || C <= 0 || (x_dtype & ~1)) return PCOPS_ERR_INVALID;
  if (B == 0 || N == 0) return PCOPS_OK;
  if (!x || !idx || !a || !g || !basis || !out) return PCOPS_ERR_INVALID;
  if (!sp_eligible(B, N, K, C) || (long long)B * N > INT_MAX) return PCOPS_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((long long)B * N)), block(sp_threads(C));
#define SP_FWD(KK) \
  hipLaunchKernelGGL(spectral_fwd_kernel<KK>, grid, block, 0, s, x, x_dtype, idx, a, g, basis, N, C, out)
  switch (K) {
    case 4: SP_FWD(4); break;
    case 8: SP_FWD(8); break;
    case 16: SP_FWD(16); break;
    default: SP_FWD(32); break;
  }
#undef SP_FWD
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

extern "C" int pcops_spectral_pool_backward(const void *x, int x_dtype, const void *dout, int dout_dtype,
                                            const int *idx, const float *a, const float *g, const float *basis, int B,
                                            int N, int K, int C, void *dx, float *da, float *dg, void *workspace,
                                            unsigned long long workspace_bytes, pcops_stream_t stream) {
  if (B < 0 || N < 0 || K <= 0 || C <= 0 || (x_dtype & ~1) || (dout_dtype & ~1)) return PCOPS_ERR_INVALID;
  if (!sp_eligible(B < 1 ? 1 : B, N < 1 ? 1 : N, K, C) || (long long)B * N > INT_MAX) return PCOPS_ERR_UNSUPPORTED;
  if (!dg) return PCOPS_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0 || N == 0) {  // no points: dg is all zeros, dx and da are empty
    if (pc_memset_async(dg, 0, (size_t)C * K * sizeof(float), s) != hipSuccess) return PCOPS_ERR_LAUNCH;
    return PCOPS_OK;
  }
  if (!x || !dout || !idx || !a || !g || !basis || !dx || !da) return PCOPS_ERR_INVALID;
  if (!workspace || workspace_bytes < pcops_spectral_pool_workspace_bytes(B, N, K, C)) return PCOPS_ERR_WORKSPACE;
  const long long BN = (long long)B * N;
  const int P = sp_points_per_chunk(BN);
  const int chunks = (int)((BN + P - 1) / P);
  float *ahat = reinterpret_cast<float *>(workspace);
  float *dgp = ahat + BN * K;
  const dim3 block(sp_threads(C));
  const size_t lds = (size_t)N * K * sizeof(int);  // <= 64 KiB by eligibility
#define SP_BWD(KK)                                                                                               \
  hipLaunchKernelGGL(spectral_bwd_kernel<KK>, dim3(chunks), block, 0, s, x, x_dtype, dout, dout_dtype, idx, a, g, \
                     basis, BN, N, C, P, da, ahat, dgp);                                                          \
  PC_CHECK_LAUNCH();                                                                                             \
  hipLaunchKernelGGL(spectral_dx_kernel<KK>, dim3((unsigned)BN), block, lds, s, dout, dout_dtype, idx, g, basis,  \
                     ahat, N, C, dx, x_dtype)
  switch (K) {
    case 4: SP_BWD(4); break;
    case 8: SP_BWD(8); break;
    case 16: SP_BWD(16); break;
    default: SP_BWD(32); break;
  }
#undef SP_BWD
  PC_CHECK_LAUNCH();
  hipLaunchKernelGGL(spectral_dg_kernel, dim3((unsigned)(((long long)K * C + 255) / 256)), dim3(256), 0, s, dgp, chunks,
                     K, C, dg);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}
