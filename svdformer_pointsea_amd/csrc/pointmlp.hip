// The ShapeNet-55 discriminator's shared point MLP 3 -> H -> H -> H with the max over the
// points (core/train_55.py:21-46) as one pass for gfx950.
//
// As torch ops each pass writes and re-reads five (B, H, N) fp32 tensors; here a pass
// reads the cloud once and writes B*H (max, arg) pairs per tile of points.
//
// Work split.  Grid = (tiles, B), a tile = PCOPS_POINT_MLP_TILE points of one cloud, 256
// threads = 4 waves.  Wave w owns the 32 output channels c0 = 32 (w % (H/32)) of layers 2
// and 3 and, at H = 64, the point group w / 2.  A workgroup walks its tile in steps of
// PI = 32 * (128 / H) points (32 per wave):
//   layer 1  VALU: thread (p, g) forms 16 channels of h1 for point p (a product, two FMAs, the
//            bias), into LDS hA[c][p]
//   layer 2  exact-f32 MFMA 32x32x2: D[c][p] = W2[c][:] hA[:][p]; act(D + b2) into LDS hB
//   layer 3  the same on hB with W3, b3; the 16 results a lane holds (16 channels of one
//            point) update its running (max, arg)
// and ends with the max over the 32 lanes of a half wave (one channel each), over the point
// groups, and one (max, arg) pair per channel into the workspace.  pm_finish_kernel folds
// the tiles in ascending order into out / arg.
//
// Weights.  A wave needs only ITS 32 rows of W2 and W3.  The MFMA's A operand is one VGPR
// per k step, so those rows live in registers for the whole tile: lane l holds row
// c0 + (l & 31), columns (l >> 5) H/2 ... + H/2 - 1, of both matrices (2 x H/2 VGPRs),
// loaded once per workgroup with 16-byte loads.  No weight ever passes through LDS; LDS
// holds only the two activation images (2 x H x PI x 4 B = 32 KiB) and 2 KiB of layer 1.
//
// Order of every dot product: acc = 0, MFMA step s = 0 .. H/2 - 1 adds k = s and then
// k = H/2 + s (the instruction is the k-ordered fmaf chain), and the bias comes last, as in
// the op chain: summed onto a bias of large magnitude first, every product would round at
// the bias's ulp (b3 = -100 cost a factor 10 to 17 in error against float64).  The order
// does not depend on the point's position, so f of a point is the same bits anywhere in the
// cloud, and the max, a selection, is independent of the order in which candidates meet.
//
// (max, arg) order: a beats b when a is NaN and b is not, or both are NaN / equal and a's
// index is lower, or a > b.  It is a total order on (value, index) pairs, so lanes, waves
// and tiles may be folded in any grouping; empty slots are (-inf, INT_MAX), which every
// real point beats.
#include <math.h>

#include "common.h"

namespace {

typedef float pm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int PM_TILE = PCOPS_POINT_MLP_TILE;
constexpr int PM_THREADS = 256;

// row i of the 32x32 accumulator held in register r of lane half h
__device__ __forceinline__ int pm_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float pm_act(float v, float slope) { return v > 0.f ? v : slope * v; }

__device__ __forceinline__ bool pm_better(float v1, int n1, float v2, int n2) {
  const bool a = v1 != v1, b = v2 != v2;
  if (a || b) return a && (!b || n1 < n2);
  return v1 > v2 || (v1 == v2 && n1 < n2);
}

// lane's H/2 consecutive weights of one row; `vec`: the row is 16-byte aligned
template <int H>
__device__ __forceinline__ void pm_load_row(float (&r)[H / 2], const float *__restrict__ row, bool vec) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < H / 8; ++q) {
      const float4 v = reinterpret_cast<const float4 *>(row)[q];
      r[4 * q] = v.x, r[4 * q + 1] = v.y, r[4 * q + 2] = v.z, r[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < H / 2; ++s) r[s] = row[s];
  }
}

template <int H>
__global__ __launch_bounds__(PM_THREADS, 2) void pm_forward_kernel(
    const float *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, float slope, int N, int tiles, int vec, float *__restrict__ pv,
    int *__restrict__ pa) {
  constexpr int CT = H / 32;        // channel tiles = waves per point group
  constexpr int PG = 4 / CT;        // point groups
  constexpr int PI = 32 * PG;       // points per step
  constexpr int NG = PM_THREADS / PI;  // layer 1: channel groups
  __shared__ float hA[H * PI], hB[H * PI];
  __shared__ float4 sW1[H];         // (w1[c][0], w1[c][1], w1[c][2], b1[c])
  __shared__ float rv[PG * H];
  __shared__ int ra[PG * H];

  const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5;
  const int c0 = 32 * (w % CT), pcol = 32 * (w / CT) + (l & 31);
  const int tile = blockIdx.x;
  const long long b = blockIdx.y;

  if (t < H) sW1[t] = make_float4(w1[3 * t], w1[3 * t + 1], w1[3 * t + 2], b1[t]);
  float w2r[H / 2], w3r[H / 2];
  pm_load_row<H>(w2r, w2 + (long long)(c0 + (l & 31)) * H + h * (H / 2), vec);
  pm_load_row<H>(w3r, w3 + (long long)(c0 + (l & 31)) * H + h * (H / 2), vec);
  pm_f32x16 b2r, b3r;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    b2r[r] = b2[c0 + pm_acc_row(r, h)];
    b3r[r] = b3[c0 + pm_acc_row(r, h)];
  }
  float mv[16];
  int ma[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) mv[r] = -INFINITY, ma[r] = INT_MAX;
  __syncthreads();

  const int p1 = t % PI, g1 = t / PI;
  for (int it = 0; it < PM_TILE / PI; ++it) {
    const int n0 = tile * PM_TILE + it * PI;
    if (n0 >= N) break;  // the whole workgroup leaves together
    {  // layer 1
      const int n = n0 + p1;
      float x0 = 0.f, x1 = 0.f, x2 = 0.f;
      if (n < N) {
        const float *xp = x + (b * N + n) * 3;
        x0 = xp[0], x1 = xp[1], x2 = xp[2];
      }
#pragma unroll
      for (int i = 0; i < H / NG; ++i) {
        const int c = g1 + NG * i;
        const float4 wb = sW1[c];
        const float v = __builtin_fmaf(wb.z, x2, __builtin_fmaf(wb.y, x1, wb.x * x0)) + wb.w;
        hA[c * PI + p1] = pm_act(v, slope);
      }
    }
    __syncthreads();
    {  // layer 2
      pm_f32x16 acc = {};
      const float *rp = hA + (h * (H / 2)) * PI + pcol;
#pragma unroll
      for (int s = 0; s < H / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w2r[s], rp[s * PI], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) hB[(c0 + pm_acc_row(r, h)) * PI + pcol] = pm_act(acc[r] + b2r[r], slope);
    }
    __syncthreads();
    {  // layer 3 and the running max
      pm_f32x16 acc = {};
      const float *rp = hB + (h * (H / 2)) * PI + pcol;
#pragma unroll
      for (int s = 0; s < H / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w3r[s], rp[s * PI], acc, 0, 0, 0);
      const int n = n0 + pcol;
      if (n < N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[r] + b3r[r];
          if (pm_better(v, n, mv[r], ma[r])) mv[r] = v, ma[r] = n;
        }
      }
    }
    // the next step's layer 1 writes hA, last read before the second barrier above; its layer 2
    // writes hB after the next step's first barrier, which every wave reaches after this layer 3
  }

  // over the 32 points of the half wave: channel c0 + pm_acc_row(r, h)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(mv[r], off, PC_WAVE);
      const int oa = __shfl_xor(ma[r], off, PC_WAVE);
      if (pm_better(ov, oa, mv[r], ma[r])) mv[r] = ov, ma[r] = oa;
    }
    if ((l & 31) == 0) {
      rv[(w / CT) * H + c0 + pm_acc_row(r, h)] = mv[r];
      ra[(w / CT) * H + c0 + pm_acc_row(r, h)] = ma[r];
    }
  }
  __syncthreads();
  if (t < H) {
    float v = rv[t];
    int a = ra[t];
#pragma unroll
    for (int g = 1; g < PG; ++g)
      if (pm_better(rv[g * H + t], ra[g * H + t], v, a)) v = rv[g * H + t], a = ra[g * H + t];
    const long long o = (b * tiles + tile) * H + t;
    pv[o] = v;
    pa[o] = a;
  }
}

// out[b][c], arg[b][c] from the tiles' pairs, ascending
__global__ __launch_bounds__(256) void pm_finish_kernel(const float *__restrict__ pv, const int *__restrict__ pa,
                                                        long long BH, int H, int tiles, float *__restrict__ out,
                                                        int *__restrict__ arg) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= BH) return;
  const long long b = e / H;
  const int c = (int)(e - b * H);
  const long long base = b * tiles * H + c;
  float v = pv[base];
  int a = pa[base];
  for (int tl = 1; tl < tiles; ++tl) {
    const float ov = pv[base + (long long)tl * H];
    const int oa = pa[base + (long long)tl * H];
    if (pm_better(ov, oa, v, a)) v = ov, a = oa;
  }
  out[e] = v;
  arg[e] = a;
}

// dx[b][n][:] = sum over c ascending with arg[b][c] == n of dxw[b][c][:]
__global__ __launch_bounds__(256) void pm_scatter_kernel(const float *__restrict__ dxw, const int *__restrict__ arg,
                                                         int N, int H, float *__restrict__ dx) {
  __shared__ int sa[128];
  __shared__ float sd[128 * 3];
  const long long b = blockIdx.y;
  const int t = threadIdx.x;
  if (t < H) sa[t] = arg[b * H + t];
  for (int i = t; i < 3 * H; i += blockDim.x) sd[i] = dxw[b * H * 3 + i];
  __syncthreads();
  const int n = blockIdx.x * blockDim.x + t;
  if (n >= N) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int c = 0; c < H; ++c)
    if (sa[c] == n) a0 += sd[3 * c], a1 += sd[3 * c + 1], a2 += sd[3 * c + 2];
  float *o = dx + (b * N + n) * 3;
  o[0] = a0, o[1] = a1, o[2] = a2;
}

long long pm_tiles(int N) { return ((long long)N + PM_TILE - 1) / PM_TILE; }

}  // namespace

extern "C" unsigned long long pcops_point_mlp_max_workspace_bytes(int B, int N, int H) {
  if (B <= 0 || N <= 0 || H <= 0) return 0;
  return (unsigned long long)B * pm_tiles(N) * H * (sizeof(float) + sizeof(int));
}

extern "C" int pcops_point_mlp_max_forward(const float *x, const float *w1, const float *b1, const float *w2,
                                           const float *b2, const float *w3, const float *b3, float slope, int B,
                                           int N, int H, float *out, int *arg, void *workspace,
                                           unsigned long long workspace_bytes, pcops_stream_t stream) {
  if (B <= 0 || N <= 0) return PCOPS_ERR_INVALID;
  if ((H != 64 && H != 128) || B > 65535) return PCOPS_ERR_UNSUPPORTED;
  if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !out || !arg) return PCOPS_ERR_INVALID;
  if (!workspace || workspace_bytes < pcops_point_mlp_max_workspace_bytes(B, N, H)) return PCOPS_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)pm_tiles(N);
  float *pv = reinterpret_cast<float *>(workspace);
  int *pa = reinterpret_cast<int *>(pv + (long long)B * tiles * H);
  const int vec = (((uintptr_t)w2 | (uintptr_t)w3) & 15) == 0;
  const dim3 grid(tiles, B), block(PM_THREADS);
  if (H == 128)
    hipLaunchKernelGGL(pm_forward_kernel<128>, grid, block, 0, s, x, w1, b1, w2, b2, w3, b3, slope, N, tiles, vec, pv,
                       pa);
  else
    hipLaunchKernelGGL(pm_forward_kernel<64>, grid, block, 0, s, x, w1, b1, w2, b2, w3, b3, slope, N, tiles, vec, pv,
                       pa);
  PC_CHECK_LAUNCH();
  const long long BH = (long long)B * H;
  hipLaunchKernelGGL(pm_finish_kernel, dim3((unsigned)((BH + 255) / 256)), dim3(256), 0, s, pv, pa, BH, H, tiles, out,
                     arg);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

extern "C" int pcops_point_mlp_max_scatter(const float *dxw, const int *arg, int B, int N, int H, float *dx,
                                           pcops_stream_t stream) {
  if (B <= 0 || N <= 0) return PCOPS_ERR_INVALID;
  if ((H != 64 && H != 128) || B > 65535) return PCOPS_ERR_UNSUPPORTED;
  if (!dxw || !arg || !dx) return PCOPS_ERR_INVALID;
  hipLaunchKernelGGL(pm_scatter_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, dxw,
                     arg, N, H, dx);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}
