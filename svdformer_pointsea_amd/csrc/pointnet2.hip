// PointNet++ set-abstraction / feature-propagation composites for gfx950:
//   pcops_ball_group          ball_query (ball_query_gpu.cu:9-44) + pcops_sa_group's row write
//   pcops_fp_interp_forward   three_nn (interpolate_gpu.cu:9-59) + the inverse-distance weights
//                             (models/model_utils.py:244-247, pointnet2_modules.py:187-189) +
//                             three_interpolate (interpolate_gpu.cu:72-101) + the skip concat
//   pcops_fp_interp_backward  three_interpolate_grad (interpolate_gpu.cu:114-154), token-major
// The unfused entry points (pcops_ball_query, pcops_sa_group, pcops_three_nn,
// pcops_three_interpolate) stay in pointops.hip and are the parity partners.
#include "common.h"

namespace {

constexpr int BG_WAVES = 4;      // centres per workgroup, one wave each
constexpr int BG_MAX_K = 1024;   // index slots a wave keeps in LDS (4 KB)

// One wave per centre.  Step: 64 candidates, one per lane; the hit lanes append their index at
// cnt + (hits in lower lanes), so slots fill in index order exactly as the serial scan does, and
// the scan stops once K are found.  The K slots live in the wave's own LDS row (no wave reads
// another's; the workgroup barrier only makes the row visible to the wave's own lanes), then the
// wave streams idx (K ints) and the K * Ct contiguous output elements of its centre.
template <int DT>
__global__ __launch_bounds__(BG_WAVES * 64) void ball_group_kernel(
    const float *__restrict__ xyz, const float *__restrict__ new_xyz, const float *__restrict__ pts, int N, int S,
    int K, int C, long long centres, float r2, int *__restrict__ idx, void *__restrict__ out) {
  __shared__ int slot[BG_WAVES][BG_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Ct = 3 + C;
  const long long per = (long long)K * Ct;
  // every wave of a workgroup runs the same number of rounds, so the barriers are uniform
  for (long long e0 = (long long)blockIdx.x * BG_WAVES; e0 < centres; e0 += (long long)gridDim.x * BG_WAVES) {
    const long long e = e0 + wave;
    const bool live = e < centres;
    const long long b = live ? e / S : 0;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    int cnt = 0;
    if (live) {
      nx = new_xyz[e * 3], ny = new_xyz[e * 3 + 1], nz = new_xyz[e * 3 + 2];
      const float *p = xyz + b * N * 3;
      for (int base = 0; base < N && cnt < K; base += 64) {
        const int k = base + lane;
        bool hit = false;
        if (k < N) hit = sqd3(nx - p[3 * (long long)k], ny - p[3 * (long long)k + 1], nz - p[3 * (long long)k + 2]) < r2;
        const unsigned long long mask = __ballot(hit);
        if (hit) {
          const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
          if (pos < K) slot[wave][pos] = k;
        }
        cnt += __popcll(mask);
      }
      cnt = min(cnt, K);
    }
    __syncthreads();
    if (live) {
      // slots after the last hit hold the first hit; a centre without a hit holds zeros
      const int first = cnt > 0 ? slot[wave][0] : 0;
      int *io = idx + e * K;
      for (int j = lane; j < K; j += 64) io[j] = j < cnt ? slot[wave][j] : first;
      for (long long t = lane; t < per; t += 64) {
        const int k = (int)(t / Ct);
        const int c = (int)(t - (long long)k * Ct);
        const int a = k < cnt ? slot[wave][k] : first;
        const bool ok = (unsigned)a < (unsigned)N;   // N == 0: index 0 reads zero (index rule)
        float v;
        if (c < 3)
          v = (ok ? xyz[(b * N + a) * 3 + c] : 0.f) - (c == 0 ? nx : (c == 1 ? ny : nz));
        else
          v = ok ? pts[(b * N + a) * C + (c - 3)] : 0.f;
        if (DT == 1)
          reinterpret_cast<__bf16 *>(out)[e * per + t] = (__bf16)v;
        else
          reinterpret_cast<float *>(out)[e * per + t] = v;
      }
    }
    __syncthreads();   // the row is rewritten in the next round
  }
}

constexpr int FP_BLOCK = 256;   // threads per workgroup
constexpr int FP_ROWS = 64;     // unknown points per workgroup: wave 0 searches, one point per lane
constexpr int FP_TILE = 1024;   // known points per LDS tile (three_nn_kernel's)

// A workgroup owns 64 unknown points.  Search: three_nn_kernel's loop in wave 0 (one unknown point
// per lane, the known cloud in 1024-point LDS tiles loaded by all four waves, nn3_insert's compare
// chain).  Each lane then turns its three squared distances into weights and parks (idx, weight)
// in LDS, and all four waves stream the 64 rows of Ct = C2 + C1 elements: consecutive threads write
// consecutive channels of one row.  The stream is the long part (Ct elements against 3 indices per
// point), so it gets four times the search's lanes and four workgroups' streams overlap the
// searches of others on a CU (256 points per workgroup left 4 waves per CU at B 32, N 2048).
template <int DT>
__global__ __launch_bounds__(FP_BLOCK) void fp_interp_kernel(
    const float *__restrict__ unknown, const float *__restrict__ known, const float *__restrict__ p2,
    const float *__restrict__ p1, int N, int M, int C2, int C1, int mode, int *__restrict__ idx,
    float *__restrict__ weight, void *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float4 kt[FP_TILE];
  __shared__ int si[FP_ROWS * 3];
  __shared__ float sw[FP_ROWS * 3];
  const int b = blockIdx.y;
  const int j0 = blockIdx.x * FP_ROWS;
  const bool searcher = threadIdx.x < FP_ROWS;   // wave-uniform: wave 0
  const int j = j0 + (threadIdx.x & (FP_ROWS - 1));
  const float *u = unknown + ((size_t)b * N + (j < N ? j : N - 1)) * 3;
  const float *kn = known + (size_t)b * M * 3;
  const float ux = u[0], uy = u[1], uz = u[2];
  float best1 = INFINITY, best2 = INFINITY, best3 = INFINITY;
  int bi1 = 0, bi2 = 0, bi3 = 0;
  for (int t0 = 0; t0 < M; t0 += FP_TILE) {
    const int cnt = min(FP_TILE, M - t0);
    for (int e = threadIdx.x; e < cnt; e += FP_BLOCK)
      kt[e] = make_float4(kn[(size_t)(t0 + e) * 3], kn[(size_t)(t0 + e) * 3 + 1], kn[(size_t)(t0 + e) * 3 + 2], 0.f);
    __syncthreads();
    if (searcher)
      for (int e = 0; e < cnt; ++e) {
        const float4 c = kt[e];
        nn3_insert(sqd3(ux - c.x, uy - c.y, uz - c.z), t0 + e, best1, best2, best3, bi1, bi2, bi3);
      }
    __syncthreads();
  }
  if (searcher) {
    const float d0 = sqrtf(best1), d1 = sqrtf(best2), d2 = sqrtf(best3);
    float r0, r1, r2;
    if (mode == 0) {
      r0 = 1.0f / fmaxf(d0, 1e-10f), r1 = 1.0f / fmaxf(d1, 1e-10f), r2 = 1.0f / fmaxf(d2, 1e-10f);
    } else {
      r0 = 1.0f / (d0 + 1e-8f), r1 = 1.0f / (d1 + 1e-8f), r2 = 1.0f / (d2 + 1e-8f);
    }
    const float norm = (r0 + r1) + r2;   // an empty (inf) slot has r = 0, so its weight is exactly 0
    const float w0 = r0 / norm, w1 = r1 / norm, w2 = r2 / norm;
    const int t = threadIdx.x * 3;
    si[t] = bi1, si[t + 1] = bi2, si[t + 2] = bi3;
    sw[t] = w0, sw[t + 1] = w1, sw[t + 2] = w2;
    if (j < N) {
      int *ii = idx + ((size_t)b * N + j) * 3;
      float *ww = weight + ((size_t)b * N + j) * 3;
      ii[0] = bi1, ii[1] = bi2, ii[2] = bi3;
      ww[0] = w0, ww[1] = w1, ww[2] = w2;
    }
  }
  __syncthreads();
  const int Ct = C2 + C1;
  const int rows = min(FP_ROWS, N - j0);
  const long long total = (long long)rows * Ct;
  const float *pp = p2 + (size_t)b * M * C2;
  for (long long e = threadIdx.x; e < total; e += FP_BLOCK) {
    const int r = (int)(e / Ct);
    const int c = (int)(e - (long long)r * Ct);
    const size_t row = (size_t)b * N + j0 + r;
    float v;
    if (c < C2) {
      // every index is in [0, M): M >= 1 and the search only stores visited k (or its initial 0)
      const float q0 = pp[(size_t)si[3 * r] * C2 + c], q1 = pp[(size_t)si[3 * r + 1] * C2 + c],
                  q2 = pp[(size_t)si[3 * r + 2] * C2 + c];
      v = __builtin_fmaf(q2, sw[3 * r + 2], __builtin_fmaf(q0, sw[3 * r], q1 * sw[3 * r + 1]));
    } else {
      v = p1[row * C1 + (c - C2)];
    }
    if (DT == 1)
      reinterpret_cast<__bf16 *>(out)[row * Ct + c] = (__bf16)v;
    else
      reinterpret_cast<float *>(out)[row * Ct + c] = v;
  }
}

// grad_points2_t[b, idx[b,j,r], c] += g[b,j,c] * w[b,j,r]: consecutive lanes take consecutive
// channels of one row, so a wave's atomics of one r form contiguous runs.
template <int DT>
__global__ __launch_bounds__(256) void fp_interp_grad_kernel(const void *__restrict__ g, const int *__restrict__ idx,
                                                             const float *__restrict__ weight, int N, int M, int C2,
                                                             int Ct, long long total, float *__restrict__ gp2) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long row = e / C2;   // (b, j)
    const int c = (int)(e - row * C2);
    const long long b = row / N;
    const long long src = row * Ct + c;
    const float gv = DT == 1 ? (float)reinterpret_cast<const __bf16 *>(g)[src] : reinterpret_cast<const float *>(g)[src];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int a = idx[row * 3 + r];
      if ((unsigned)a < (unsigned)M) atomicAdd(gp2 + (b * M + a) * C2 + c, gv * weight[row * 3 + r]);
    }
  }
}

unsigned grid_ll(long long blocks, long long cap) {
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

extern "C" int pcops_ball_group(const float *xyz, const float *new_xyz, const float *points_t, int B, int N, int S,
                                int K, int C, float radius, int *idx, void *out, int out_dtype,
                                pcops_stream_t stream) {
  if (B < 0 || N < 0 || S < 0 || K < 0 || C < 0 || (out_dtype != 0 && out_dtype != 1)) return PCOPS_ERR_INVALID;
  if (K > BG_MAX_K) return PCOPS_ERR_INVALID;
  const long long centres = (long long)B * S;
  if (centres == 0 || K == 0) return PCOPS_OK;
  // an empty cloud may be NULL: index 0 is then out of range and never read
  if (!new_xyz || !idx || !out || (N > 0 && (!xyz || (C > 0 && !points_t)))) return PCOPS_ERR_INVALID;
  const unsigned grid = grid_ll((centres + BG_WAVES - 1) / BG_WAVES, 1 << 20);
  if (out_dtype == 1)
    hipLaunchKernelGGL(ball_group_kernel<1>, dim3(grid), dim3(BG_WAVES * 64), 0, (hipStream_t)stream, xyz, new_xyz,
                       points_t, N, S, K, C, centres, radius * radius, idx, out);
  else
    hipLaunchKernelGGL(ball_group_kernel<0>, dim3(grid), dim3(BG_WAVES * 64), 0, (hipStream_t)stream, xyz, new_xyz,
                       points_t, N, S, K, C, centres, radius * radius, idx, out);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

extern "C" int pcops_fp_interp_forward(const float *unknown, const float *known, const float *points2_t,
                                       const float *points1_t, int B, int N, int M, int C2, int C1, int mode, int *idx,
                                       float *weight, void *out, int out_dtype, pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 1 || C2 < 0 || C1 < 0 || (mode != 0 && mode != 1) || (out_dtype != 0 && out_dtype != 1))
    return PCOPS_ERR_INVALID;
  if (B > 65535) return PCOPS_ERR_INVALID;
  if (B == 0 || N == 0) return PCOPS_OK;
  if (!unknown || !known || !idx || !weight || (C2 > 0 && !points2_t) || (C1 > 0 && !points1_t) ||
      (C2 + C1 > 0 && !out))
    return PCOPS_ERR_INVALID;
  const dim3 grid((N + FP_ROWS - 1) / FP_ROWS, B);
  if (out_dtype == 1)
    hipLaunchKernelGGL(fp_interp_kernel<1>, grid, dim3(FP_BLOCK), 0, (hipStream_t)stream, unknown, known, points2_t,
                       points1_t, N, M, C2, C1, mode, idx, weight, out);
  else
    hipLaunchKernelGGL(fp_interp_kernel<0>, grid, dim3(FP_BLOCK), 0, (hipStream_t)stream, unknown, known, points2_t,
                       points1_t, N, M, C2, C1, mode, idx, weight, out);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

extern "C" int pcops_fp_interp_backward(const void *grad_out, int grad_dtype, const int *idx, const float *weight,
                                        int B, int N, int M, int C2, int Ct, float *grad_points2_t,
                                        pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 0 || C2 < 0 || Ct < C2 || (grad_dtype != 0 && grad_dtype != 1)) return PCOPS_ERR_INVALID;
  if ((size_t)B * M * C2 == 0) return PCOPS_OK;
  if (!grad_points2_t) return PCOPS_ERR_INVALID;
  if (pc_memset_async(grad_points2_t, 0, sizeof(float) * (size_t)B * M * C2, (hipStream_t)stream) != hipSuccess)
    return PCOPS_ERR_LAUNCH;
  const long long total = (long long)B * N * C2;
  if (total == 0) return PCOPS_OK;
  if (!grad_out || !idx || !weight) return PCOPS_ERR_INVALID;
  const unsigned grid = grid_ll((total + 255) / 256, 8192);
  if (grad_dtype == 1)
    hipLaunchKernelGGL(fp_interp_grad_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, grad_out, idx, weight,
                       N, M, C2, Ct, total, grad_points2_t);
  else
    hipLaunchKernelGGL(fp_interp_grad_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, grad_out, idx, weight,
                       N, M, C2, Ct, total, grad_points2_t);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}
