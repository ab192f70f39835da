// Point <-> pixel feature exchange (gfx950).
//
// point_fea_img_fea (models/model_utils.py:1134-1154) splats per-point feature rows into an
// image plane; distribute_img_fea_points (:1157-1176, with batched_index_select :1119-1131)
// reads image features back at the points.  Each is the other's gradient, so two kernels
// serve all four directions:
//   pcops_pixel_gather  out[b,i,:] = img[b, pix(b,i), :]            (0 where rejected)
//   pcops_pixel_splat   out[b,p,:] = sum over i, ascending, with pix(b,i) == p of fea[b,i,:]
// A coordinate c takes part iff 0 <= c <= P-1, tested on the value as stored (float or
// integer) before any conversion; its pixel is the truncation.  Everything else (negative,
// >= P, NaN, +-inf, beyond the int range) contributes nothing, reads as 0 and is never used
// as an address.
//
// The splat has no float atomics.  It builds the inverted index first: a count per pixel
// (integer atomics: the counts do not depend on arrival order), then one wave per cloud turns
// the counts into offsets and places the point indices pixel by pixel IN POINT ORDER (a stable
// counting sort: 64 points per step, their rank among the equal keys of the step from
// ballots), then one lane per output element adds its pixel's rows in list order.  Every
// output element is therefore the fp32 sum of its terms in ascending point index -- the bits
// of the reference's sequential scatter_add -- and is stored exactly once, empty pixels
// included.  Nothing depends on N or on a pixel's share fitting in LDS: the lists live in the
// caller's workspace; only the per-pixel cursors move to LDS when P allows it (P <= 8192).
// Scaling limit: the placing step is ONE wave per cloud walking N/64 dependent steps, so it keeps
// B compute units busy and its time grows with N (24 us at N 2048; 636 us at N 65536, where with
// B = 1 the float-atomic torch chain is 2.1x faster -- DESIGN.md section 3, "View-space ops").
#include "common.h"

namespace {

// A coordinate as stored (dtype PCOPS_COORD_*), widened to 64 bits without looking at it, so that a
// caller can issue the load early and apply the index rule (pixel_of_raw) where it needs the pixel.
__device__ __forceinline__ uint64_t coord_raw(const void *__restrict__ coord, int dtype, size_t e) {
  if (dtype == PCOPS_COORD_F32 || dtype == PCOPS_COORD_I32) return ((const uint32_t *)coord)[e];
  return ((const uint64_t *)coord)[e];
}

__device__ __forceinline__ int pixel_of_raw(uint64_t raw, int dtype, int P) {
  switch (dtype) {
    case PCOPS_COORD_F32: {
      const float c = __uint_as_float((uint32_t)raw);
      if (!(c >= 0.f && c <= (float)(P - 1))) return -1;
      const int p = (int)c;
      return p < P ? p : -1;  // (float)(P - 1) rounds up past 2^24
    }
    case PCOPS_COORD_F64: {
      const double c = __longlong_as_double((long long)raw);
      return (c >= 0.0 && c <= (double)(P - 1)) ? (int)c : -1;
    }
    case PCOPS_COORD_I32: {
      const int c = (int)(uint32_t)raw;
      return (c >= 0 && c <= P - 1) ? c : -1;
    }
    default: {
      const long long c = (long long)raw;
      return (c >= 0 && c <= (long long)(P - 1)) ? (int)c : -1;
    }
  }
}

__device__ __forceinline__ int pixel_of(const void *__restrict__ coord, int dtype, size_t e, int P) {
  return pixel_of_raw(coord_raw(coord, dtype, e), dtype, P);
}

__global__ void pixel_gather_kernel(const float *__restrict__ img, const void *__restrict__ coord, int dtype, int B,
                                    int N, int C, int P, long long sb, long long sp, long long sc,
                                    float *__restrict__ out) {
  const size_t tot = (size_t)B * N * C;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const size_t bn = e / C;
    const size_t b = bn / N;
    const int pix = pixel_of(coord, dtype, bn, P);
    out[e] = pix >= 0 ? img[(long long)b * sb + (long long)pix * sp + (long long)c * sc] : 0.f;
  }
}

__global__ void splat_count_kernel(const void *__restrict__ coord, int dtype, int B, int N, int P,
                                   int *__restrict__ cnt) {
  const size_t tot = (size_t)B * N;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int pix = pixel_of(coord, dtype, e, P);
    if (pix >= 0) atomicAdd(cnt + (e / N) * (size_t)P + pix, 1);
  }
}

constexpr int kCursorLds = 8192;

// One wave per cloud.  cnt[b][p] holds the pixel's count on entry and the END of its list on
// exit (its list is list[b][end[p-1] .. end[p]), end[-1] = 0).  LDS: the cursors sit in LDS
// (P <= kCursorLds), else they are cnt itself.  Each step loads the next step's coordinates
// before it looks at its own, so that load is in flight under the step's work; a step still
// waits for the previous step's list store (loads and stores share one counter on gfx9).
template <bool LDS>
__global__ __launch_bounds__(PC_WAVE) void splat_place_kernel(const void *__restrict__ coord, int dtype, int N, int P,
                                                              int bits, int *__restrict__ cnt,
                                                              int *__restrict__ list) {
  __shared__ int lcur[LDS ? kCursorLds : 1];
  const int b = blockIdx.x, lane = threadIdx.x;
  int *gc = cnt + (size_t)b * P;
  int run = 0;
  for (int p0 = 0; p0 < P; p0 += PC_WAVE) {
    const int p = p0 + lane;
    const int c = p < P ? gc[p] : 0;
    int inc = c;
#pragma unroll
    for (int off = 1; off < PC_WAVE; off <<= 1) {
      const int t = __shfl_up(inc, off, PC_WAVE);
      if (lane >= off) inc += t;
    }
    if (p < P) {  // exclusive: the start of the pixel's list
      if (LDS) lcur[p] = run + inc - c;
      else gc[p] = run + inc - c;
    }
    run += __shfl(inc, PC_WAVE - 1, PC_WAVE);
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  int *lst = list + (size_t)b * N;
  const uint64_t below = (1ull << lane) - 1ull;
  const size_t last = (size_t)b * N + (N - 1);
  uint64_t raw = coord_raw(coord, dtype, min((size_t)b * N + lane, last));
  for (int i0 = 0; i0 < N; i0 += PC_WAVE) {
    const int i = i0 + lane;
    // the next step's coordinates (clamped to the cloud: a lane past its end rejects by i < N)
    const uint64_t rnext = coord_raw(coord, dtype, min((size_t)b * N + i + PC_WAVE, last));
    const int pix = i < N ? pixel_of_raw(raw, dtype, P) : -1;
    uint64_t same = __ballot(pix >= 0);  // ends as the lanes of this step that hold this lane's pixel
    for (int k = 0; k < bits; ++k) {
      const bool one = (pix >> k) & 1;
      const uint64_t bal = __ballot(one);
      same &= one ? bal : ~bal;
    }
    if (pix >= 0) {
      const int base = LDS ? lcur[pix] : gc[pix];
      lst[base + __popcll(same & below)] = i;
      // the group's highest lane moves the cursor, after every lane of the group has read it
      // (one wave: the load above is issued for all lanes before this store)
      if ((same >> lane) == 1ull) {
        if (LDS) lcur[pix] = base + __popcll(same);
        else gc[pix] = base + __popcll(same);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    raw = rnext;
  }
  if (LDS)
    for (int p = lane; p < P; p += PC_WAVE) gc[p] = lcur[p];
}

// PFAST: consecutive lanes take consecutive pixels of one channel (an output whose pixel stride is 1, the
// NCHW image gradient: coalesced stores); else consecutive channels of one pixel (rows / channels_last).
template <bool PFAST>
__global__ void splat_sum_kernel(const float *__restrict__ fea, const int *__restrict__ ends,
                                 const int *__restrict__ list, int B, int N, int C, int P, long long sb, long long sp,
                                 long long sc, float *__restrict__ out) {
  const size_t tot = (size_t)B * P * C;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    int c, p;
    size_t b;
    if (PFAST) {
      p = (int)(e % P);
      const size_t bc = e / P;
      c = (int)(bc % C);
      b = bc / C;
    } else {
      c = (int)(e % C);
      const size_t bp = e / C;
      p = (int)(bp % P);
      b = bp / P;
    }
    const int *en = ends + b * P;
    const int t = en[p];
    int j = p ? en[p - 1] : 0;
    const int *lst = list + b * N;
    const float *f = fea + b * (size_t)N * C + c;
    float acc = 0.f;
    // four loads in flight; the adds stay in list order
    for (; j + 4 <= t; j += 4) {
      const float v0 = f[(size_t)lst[j] * C], v1 = f[(size_t)lst[j + 1] * C];
      const float v2 = f[(size_t)lst[j + 2] * C], v3 = f[(size_t)lst[j + 3] * C];
      acc = acc + v0;
      acc = acc + v1;
      acc = acc + v2;
      acc = acc + v3;
    }
    for (; j < t; ++j) acc = acc + f[(size_t)lst[j] * C];
    out[(long long)b * sb + (long long)p * sp + (long long)c * sc] = acc;
  }
}

size_t align64(size_t v) { return (v + 63) / 64 * 64; }

bool coord_dtype_ok(int d) { return d >= PCOPS_COORD_F32 && d <= PCOPS_COORD_I64; }

}  // namespace

extern "C" int pcops_pixel_gather(const float *img, const void *coord, int coord_dtype, int B, int N, int C, int P,
                                  long long stride_b, long long stride_p, long long stride_c, float *out,
                                  pcops_stream_t stream) {
  if (B < 0 || N < 0 || C < 0 || P < 0 || !coord_dtype_ok(coord_dtype)) return PCOPS_ERR_INVALID;
  const size_t tot = (size_t)B * N * C;
  if (tot == 0) return PCOPS_OK;
  if (!coord || !out || (P > 0 && !img)) return PCOPS_ERR_INVALID;
  hipLaunchKernelGGL(pixel_gather_kernel, dim3(grid_for(tot, 256)), dim3(256), 0, (hipStream_t)stream, img, coord,
                     coord_dtype, B, N, C, P, stride_b, stride_p, stride_c, out);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

extern "C" unsigned long long pcops_pixel_splat_workspace_bytes(int B, int N, int P) {
  if (B <= 0 || P <= 0 || N < 0) return 0;
  return align64((size_t)B * P * sizeof(int)) + align64((size_t)B * N * sizeof(int));
}

extern "C" int pcops_pixel_splat(const float *fea, const void *coord, int coord_dtype, int B, int N, int C, int P,
                                 float *out, long long stride_b, long long stride_p, long long stride_c,
                                 void *workspace, unsigned long long workspace_bytes, pcops_stream_t stream) {
  if (B < 0 || N < 0 || C < 0 || P < 0 || !coord_dtype_ok(coord_dtype)) return PCOPS_ERR_INVALID;
  const size_t tot = (size_t)B * P * C;
  if (tot == 0) return PCOPS_OK;
  if (!out || (N > 0 && (!fea || !coord))) return PCOPS_ERR_INVALID;
  if (!workspace || workspace_bytes < pcops_pixel_splat_workspace_bytes(B, N, P)) return PCOPS_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int *cnt = (int *)workspace;
  int *list = (int *)((char *)workspace + align64((size_t)B * P * sizeof(int)));
  if (pc_memset_async(cnt, 0, (size_t)B * P * sizeof(int), s)) return PCOPS_ERR_LAUNCH;
  if (N > 0) {
    hipLaunchKernelGGL(splat_count_kernel, dim3(grid_for((size_t)B * N, 256)), dim3(256), 0, s, coord, coord_dtype, B,
                       N, P, cnt);
    PC_CHECK_LAUNCH();
    int bits = 1;
    while (bits < 31 && (1ll << bits) < (long long)P) ++bits;
    if (P <= kCursorLds)
      hipLaunchKernelGGL(splat_place_kernel<true>, dim3(B), dim3(PC_WAVE), 0, s, coord, coord_dtype, N, P, bits, cnt,
                         list);
    else
      hipLaunchKernelGGL(splat_place_kernel<false>, dim3(B), dim3(PC_WAVE), 0, s, coord, coord_dtype, N, P, bits, cnt,
                         list);
    PC_CHECK_LAUNCH();
  }
  // pixel-fast lanes pay one cache line per lane for every row they add: only where the lists are short
  // (on average under one point per pixel) do the coalesced stores win
  if (stride_p == 1 && stride_c != 1 && N <= P)
    hipLaunchKernelGGL(splat_sum_kernel<true>, dim3(grid_for(tot, 256)), dim3(256), 0, s, fea, cnt, list, B, N, C, P,
                       stride_b, stride_p, stride_c, out);
  else
    hipLaunchKernelGGL(splat_sum_kernel<false>, dim3(grid_for(tot, 256)), dim3(256), 0, s, fea, cnt, list, B, N, C, P,
                       stride_b, stride_p, stride_c, out);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}
