// Chamfer distance (metrics/CD/chamfer3D/chamfer3D.cu) for gfx950.
//
// Forward: both directions in ONE launch (blockIdx.x splits dir 0 = xyz1->xyz2
// and dir 1 = xyz2->xyz1), each thread owning Q queries in VGPRs and the
// target cloud streamed through a 1024-point LDS tile read by broadcast.
// Two kernels, the same results (the reference's distance bits and its
// lowest-index tie rule: strict '<' inside a chunk, strict '>' across chunks,
// chamfer3D.cu:36,126):
//   chamfer_nn_kernel      the reference's direct-difference distance per pair
//                          (3 sub + mul + 2 fma, nvcc contraction order) and one
//                          v_min; argmin recovered per 32-target sub-tile and
//                          re-derived from the winning sub-tile (7 VALU / pair);
//   chamfer_screen_kernel  ranks targets by |t|^2 - 2 a.t (3.5 VALU / pair) under
//                          a rigorous rounding margin and re-derives the winner
//                          with the direct expression (see its comment);
//   chamfer_mfma_kernel    the same screen on fp32 MFMA (opt-in, PCOPS_CHAMFER_MFMA).
// Large clouds go through pcops_chamfer_forward_ws instead: Morton-sorted clouds and a
// culled, nearest-first search per wave over 64-point tiles (the last section).
//
// Backward (chamfer3D.cu:155-195: own and partner terms both by float
// atomics, so its sums depend on arrival order): one launch in which every
// point's gradient is written exactly once, by the workgroup owning that point
// as a partner TARGET.  The workgroup scans the source cloud's NN indices, and
// the partner terms of its targets are summed in 64-bit fixed point in LDS
// (integer adds: exact and order-independent -> bitwise reproducible), then
// combined with the target's own term.  Scattered float atomics (one lane per
// 12-B row) ran at the ~0.08 TB/s one-row-per-lane atomic rate; the old
// two-kernel atomic form stays behind PCOPS_CHAMFER_BWD=atomic for A/B runs.
#include <cfloat>
#include <cstdlib>

#include "common.h"

namespace {

constexpr int kTile = 1024;
constexpr int kSub = 32;
constexpr int kThreads = 256;

// The reference's own scan (chamfer3D.cu:16-129): 512-target chunks, each seeded with its
// FIRST target and updated on strict '<', merged across chunks on strict '>'.  Its result
// equals the lowest-index minimum over the non-NaN distances -- what the fast searches
// compute -- unless a distance at a chunk start is NaN: then a NaN seed of chunk 0 pins
// (NaN, 0), and a NaN seed of a later chunk hides that whole chunk.  For a finite query that
// happens only for a target 512c with a NaN coordinate (finite - inf squares to inf, never
// NaN), so the kernels send exactly the non-finite queries and the queries of a cloud with
// such a target here.
constexpr int kRefChunk = 512;

__device__ __forceinline__ void ref_scan(const float *T, int NT, float ax, float ay, float az, float &res, int &ri) {
  for (int k2 = 0; k2 < NT; k2 += kRefChunk) {
    const int end = min(NT, k2 + kRefChunk);
    float best = sqd3(T[3 * k2] - ax, T[3 * k2 + 1] - ay, T[3 * k2 + 2] - az);
    int bi = k2;
    for (int k = k2 + 1; k < end; ++k) {
      const float d = sqd3(T[3 * k] - ax, T[3 * k + 1] - ay, T[3 * k + 2] - az);
      if (d < best) best = d, bi = k;
    }
    if (k2 == 0 || res > best) res = best, ri = bi;
  }
}

// block-uniform: does a chunk-start target (index 512c) have a NaN coordinate?
__device__ bool nan_chunk_starts(const float *T, int NT) {
  int f = 0;
  for (int c = threadIdx.x; c * kRefChunk < NT; c += blockDim.x) {
    const float *p = T + (size_t)3 * c * kRefChunk;
    f |= (p[0] != p[0]) | (p[1] != p[1]) | (p[2] != p[2]);
  }
  return __syncthreads_or(f);
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// Counted clouds (pcops_chamfer_forward_counts): the direct and the screened kernel carry a template
// flag, as the FPS kernels do -- CNT = false is the uniform instantiation (cnt1 / cnt2 unused, the
// same code as without the flag), CNT = true reads the counts.  There NAp / NTp are the padded row
// counts (the strides), NA / NT the clouds' own counts clamped to [0, padded]; a row k >= count is
// absent: never read as a query or a target, written (0, 0).  A pair with an empty side is all (0, 0).
template <bool CNT>
__device__ __forceinline__ int cloud_count(const int *cnt, int b, int n) {
  return (CNT && cnt) ? min(max(cnt[b], 0), n) : n;
}

// the block's rows [q0, q0 + rows) of a counted cloud that need no search: (0, 0)
__device__ __forceinline__ void write_absent(float *dist, int *idx, int q0, int rows, int NAp) {
  for (int q = q0 + threadIdx.x; q < min(q0 + rows, NAp); q += blockDim.x) dist[q] = 0.f, idx[q] = 0;
}

template <int Q, bool CNT = false>
__global__ __launch_bounds__(kThreads) void chamfer_nn_kernel(const float *__restrict__ xyz1,
                                                              const float *__restrict__ xyz2, int N, int M,
                                                              float *__restrict__ dist1, float *__restrict__ dist2,
                                                              int *__restrict__ idx1, int *__restrict__ idx2,
                                                              int blocks_dir0, const int *__restrict__ cnt1 = nullptr,
                                                              const int *__restrict__ cnt2 = nullptr) {
  const int b = blockIdx.y;
  const bool dir = (int)blockIdx.x >= blocks_dir0;
  const int bx = dir ? blockIdx.x - blocks_dir0 : blockIdx.x;
  const int NAp = dir ? M : N, NTp = dir ? N : M;
  const int NA = cloud_count<CNT>(dir ? cnt2 : cnt1, b, NAp), NT = cloud_count<CNT>(dir ? cnt1 : cnt2, b, NTp);
  const float *A = (dir ? xyz2 : xyz1) + (size_t)b * NAp * 3;
  const float *T = (dir ? xyz1 : xyz2) + (size_t)b * NTp * 3;
  float *dist = (dir ? dist2 : dist1) + (size_t)b * NAp;
  int *idx = (dir ? idx2 : idx1) + (size_t)b * NAp;
  if (CNT) {
    if (NT <= 0 || bx * kThreads * Q >= NA) {  // empty side, or a block of absent rows only
      write_absent(dist, idx, bx * kThreads * Q, kThreads * Q, NAp);
      return;
    }
  }
  if (NT <= 0) return;  // outputs keep the caller's zeros (chamfer3D.cu never writes them)
  const bool nanst = nan_chunk_starts(T, NT);

  const int tid = threadIdx.x;
  float ax[Q], ay[Q], az[Q], best[Q];
  int bs[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int qi = bx * kThreads * Q + i * kThreads + tid;
    const int qc = qi < NA ? qi : NA - 1;
    ax[i] = A[3 * qc];
    ay[i] = A[3 * qc + 1];
    az[i] = A[3 * qc + 2];
    best[i] = INFINITY;
    bs[i] = 0;
  }

  __shared__ float4 tile[kTile];
  for (int t0 = 0; t0 < NT; t0 += kTile) {
    const int cnt = min(kTile, NT - t0);
    for (int e = tid; e < kTile; e += kThreads) {
      float4 v;
      if (e < cnt) {
        const float *src = T + (size_t)(t0 + e) * 3;
        v = make_float4(src[0], src[1], src[2], 0.f);
      } else {
        v = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
      }
      tile[e] = v;
    }
    __syncthreads();
    const int nsub = (cnt + kSub - 1) / kSub;
    for (int sb = 0; sb < nsub; ++sb) {
      float m[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) m[i] = INFINITY;
#pragma unroll 8
      for (int kk = 0; kk < kSub; ++kk) {
        const float4 tp = tile[sb * kSub + kk];
#pragma unroll
        for (int i = 0; i < Q; ++i) m[i] = fminf(m[i], sqd3(tp.x - ax[i], tp.y - ay[i], tp.z - az[i]));
      }
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        if (m[i] < best[i]) {
          best[i] = m[i];
          bs[i] = t0 + sb * kSub;
        }
      }
    }
    __syncthreads();
  }
  // exact argmin: first target of the winning sub-tile whose distance equals best
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int qi = bx * kThreads * Q + i * kThreads + tid;
    if (qi >= NA) {
      if (CNT && qi < NAp) dist[qi] = 0.f, idx[qi] = 0;
      continue;
    }
    if (nanst || !finite3(ax[i], ay[i], az[i])) {
      float r = 0.f;
      int rk = 0;
      ref_scan(T, NT, ax[i], ay[i], az[i], r, rk);
      dist[qi] = r;
      idx[qi] = rk;
      continue;
    }
    int bk = bs[i];
    const int end = min(bs[i] + kSub, NT);
    for (int k = bs[i]; k < end; ++k) {
      const float d = sqd3(T[3 * k] - ax[i], T[3 * k + 1] - ay[i], T[3 * k + 2] - az[i]);
      if (d == best[i]) {
        bk = k;
        break;
      }
    }
    dist[qi] = best[i] < INFINITY ? best[i] : sqd3(T[3 * bk] - ax[i], T[3 * bk + 1] - ay[i], T[3 * bk + 2] - az[i]);
    idx[qi] = bk;
  }
}


// ---------------------------------------------------------------- screened
// Screened nearest-neighbour search (the default for the large launches).
// The reference's distance |a - t|^2 costs 3 sub + mul + 2 fma + min = 7 VALU
// per pair; packed f32 does not help (v_pk_* issue at half rate on gfx950,
// measured: same wall time).  The screen instead ranks targets by
//     e(t) = |t|^2 - 2 a.t      (= |a - t|^2 - |a|^2 in exact arithmetic)
// with |t|^2 precomputed per tile: 3 fma + 1/2 v_min3 = 3.5 VALU per pair.
// e is a different fp32 expression, so it only SELECTS: per 32-target
// sub-tile the minimum of e is compared with the query's running minimum plus
// a rigorous rounding margin, and the sub-tiles that may hold the exact
// argmin are remembered (4 slots per query).  After the sweep the winner is
// re-derived with the reference expression (sqd3) over those sub-tiles only,
// lowest index on equal distances -- the reference's bits and tie rule.
//
// Margin: with u = 2^-24, |t| <= Tm (running max over the tiles seen), the fp32
// e of any target is within eps = 16u (Tm^2 + |a| Tm) of its exact value, and
// the direct fp32 distance within 8u D of the exact D.  If k* is the direct
// argmin, e(k*) <= min e + 2 eps + 16u (min e + |a|^2 + eps), the slack every
// keep / prune test below allows.  A query whose slots overflow (near-ties
// across > 4 sub-tiles) or is not finite is re-derived by a full direct scan.
constexpr int kSlots = 4;
#ifndef PCOPS_CH_RD
#define PCOPS_CH_RD 8  // re-derivation: candidate targets loaded per batch (A/B builds override)
#endif
constexpr int kRd = PCOPS_CH_RD;
constexpr float kU = 5.9604645e-8f;  // 2^-24

__device__ __forceinline__ float screen_slack(float mine, float an, float eps) {
  return 2.f * eps + 16.f * kU * fmaxf(0.f, mine + an + eps);
}

template <int Q, bool CNT = false>   // CNT: see chamfer_nn_kernel
__global__ __launch_bounds__(kThreads) void chamfer_screen_kernel(const float *__restrict__ xyz1,
                                                                  const float *__restrict__ xyz2, int N, int M,
                                                                  float *__restrict__ dist1, float *__restrict__ dist2,
                                                                  int *__restrict__ idx1, int *__restrict__ idx2,
                                                                  int blocks_dir0,
                                                                  const int *__restrict__ cnt1 = nullptr,
                                                                  const int *__restrict__ cnt2 = nullptr) {
  const int b = blockIdx.y;
  const bool dir = (int)blockIdx.x >= blocks_dir0;
  const int bx = dir ? blockIdx.x - blocks_dir0 : blockIdx.x;
  const int NAp = dir ? M : N, NTp = dir ? N : M;
  const int NA = cloud_count<CNT>(dir ? cnt2 : cnt1, b, NAp), NT = cloud_count<CNT>(dir ? cnt1 : cnt2, b, NTp);
  const float *A = (dir ? xyz2 : xyz1) + (size_t)b * NAp * 3;
  const float *T = (dir ? xyz1 : xyz2) + (size_t)b * NTp * 3;
  float *dist = (dir ? dist2 : dist1) + (size_t)b * NAp;
  int *idx = (dir ? idx2 : idx1) + (size_t)b * NAp;
  if (CNT) {
    if (NT <= 0 || bx * kThreads * Q >= NA) {  // empty side, or a block of absent rows only
      write_absent(dist, idx, bx * kThreads * Q, kThreads * Q, NAp);
      return;
    }
  }
  if (NT <= 0) return;
  const bool nanst = nan_chunk_starts(T, NT);

  const int tid = threadIdx.x;
  float ax[Q], ay[Q], az[Q], an[Q], anorm[Q], mine[Q], slack[Q];
  float mx[Q], my[Q], mz[Q];
  float cm[Q][kSlots];
  int cs[Q][kSlots];
  bool over[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int qi = bx * kThreads * Q + i * kThreads + tid;
    const int qc = qi < NA ? qi : NA - 1;
    ax[i] = A[3 * qc];
    ay[i] = A[3 * qc + 1];
    az[i] = A[3 * qc + 2];
    mx[i] = -2.f * ax[i];
    my[i] = -2.f * ay[i];
    mz[i] = -2.f * az[i];
    an[i] = (ax[i] * ax[i] + ay[i] * ay[i]) + az[i] * az[i];
    anorm[i] = sqrtf(an[i]);
    mine[i] = INFINITY;
    slack[i] = INFINITY;
    over[i] = !(an[i] < INFINITY);  // NaN / inf query: direct scan
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
      cm[i][c] = INFINITY;
      cs[i][c] = -1;
    }
  }

  __shared__ float4 tile[kTile];
  __shared__ float tmax_s[kThreads / 64];
  float eps_t2 = 0.f;  // running max |t|^2 over the tiles seen (wave-uniform)
  for (int t0 = 0; t0 < NT; t0 += kTile) {
    const int cnt = min(kTile, NT - t0);
    float lmax = 0.f;
    for (int e = tid; e < kTile; e += kThreads) {
      float4 v = make_float4(0.f, 0.f, 0.f, INFINITY);  // padding: e = +inf, never a minimum
      if (e < cnt) {
        const float *src = T + (size_t)(t0 + e) * 3;
        v = make_float4(src[0], src[1], src[2], 0.f);
        v.w = (v.x * v.x + v.y * v.y) + v.z * v.z;
        lmax = fmaxf(lmax, v.w);
      }
      tile[e] = v;
    }
    lmax = wave_max_f32(lmax);
    if ((tid & 63) == 0) tmax_s[tid >> 6] = lmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) eps_t2 = fmaxf(eps_t2, tmax_s[w]);
    const float tm = sqrtf(eps_t2);
    float eps[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      eps[i] = 16.f * kU * (eps_t2 + anorm[i] * tm);
      slack[i] = screen_slack(mine[i], an[i], eps[i]);  // eps only grows: re-derive
      // |e| <= Tm^2 + 2|a|Tm: near fp32 overflow e may be +-inf / NaN and the margin
      // meaningless -> direct scan
      over[i] = over[i] || !(eps_t2 + 2.f * anorm[i] * tm < 1e38f);
    }
    const int nsub = (cnt + kSub - 1) / kSub;
    bool act = false;   // a query of this lane still screening: an overflowed one takes the full scan anyway
#pragma unroll
    for (int i = 0; i < Q; ++i) act = act || !over[i];
    for (int sb = 0; sb < nsub && act; ++sb) {
      float m[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) m[i] = INFINITY;
#pragma unroll 4
      for (int kk = 0; kk < kSub; kk += 2) {
        const float4 p0 = tile[sb * kSub + kk], p1 = tile[sb * kSub + kk + 1];
#pragma unroll
        for (int i = 0; i < Q; ++i) {
          const float e0 = __builtin_fmaf(mz[i], p0.z, __builtin_fmaf(my[i], p0.y, __builtin_fmaf(mx[i], p0.x, p0.w)));
          const float e1 = __builtin_fmaf(mz[i], p1.z, __builtin_fmaf(my[i], p1.y, __builtin_fmaf(mx[i], p1.x, p1.w)));
          m[i] = fminf(fminf(m[i], e0), e1);
        }
      }
      const int sub0 = t0 + sb * kSub;
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        if (m[i] <= mine[i] + slack[i]) {  // rare: this sub-tile may hold the argmin
          if (m[i] < mine[i]) {
            mine[i] = m[i];
            slack[i] = screen_slack(mine[i], an[i], eps[i]);
#pragma unroll
            for (int c = 0; c < kSlots; ++c)
              if (cs[i][c] >= 0 && cm[i][c] > mine[i] + slack[i]) cs[i][c] = -1;  // prune
          }
          bool placed = false;
#pragma unroll
          for (int c = 0; c < kSlots; ++c) {
            if (!placed && cs[i][c] < 0) {
              cs[i][c] = sub0;
              cm[i][c] = m[i];
              placed = true;
            }
          }
          over[i] = over[i] || !placed;
        }
      }
    }
    __syncthreads();
  }
  // exact re-derivation with the reference expression
  float bestv[Q];
  int bkv[Q];
  bool full[Q], raw[Q];   // raw: ref_scan's result, stored as it is
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int qi = bx * kThreads * Q + i * kThreads + tid;
    float best = INFINITY;
    int bk = 0;
    full[i] = raw[i] = false;
    if (qi >= NA) {
      bestv[i] = best, bkv[i] = bk;
      continue;
    }
    if (nanst || !finite3(ax[i], ay[i], az[i])) {
      ref_scan(T, NT, ax[i], ay[i], az[i], best, bk);
      bestv[i] = best, bkv[i] = bk, raw[i] = true;
      continue;
    }
    if (!over[i]) {
#pragma unroll
      for (int c = 0; c < kSlots; ++c) {
        if (cs[i][c] < 0) continue;
        const int k0 = cs[i][c], k1 = min(k0 + kSub, NT);
        // the candidate targets' coordinates in batches of kRd, every batch's loads issued
        // together (the plain loop waited out one global-load latency per target: most of
        // this kernel's time at the small launches, where it is not hidden by other waves)
        for (int kb = k0; kb < k1; kb += kRd) {
          float px[kRd], py[kRd], pz[kRd];
#pragma unroll
          for (int j = 0; j < kRd; ++j) {
            const int kc = min(kb + j, k1 - 1);
            px[j] = T[3 * kc];
            py[j] = T[3 * kc + 1];
            pz[j] = T[3 * kc + 2];
          }
#pragma unroll
          for (int j = 0; j < kRd; ++j) {
            const int k = kb + j;
            const float d = sqd3(px[j] - ax[i], py[j] - ay[i], pz[j] - az[i]);
            if (k < k1 && (d < best || (d == best && k < bk))) {
              best = d;
              bk = k;
            }
          }
        }
      }
    }
    full[i] = over[i] || !(best < INFINITY);   // slot overflow (near-coincident targets) / overflow risk
    bestv[i] = best, bkv[i] = bk;
  }
  // the full direct scan, for the queries that need it, over the targets staged through LDS by the
  // whole block (every lane reads the same target: an LDS broadcast).  Degenerate clouds -- a
  // random-init network's coarse output collapses to a blob -- overflow every query's slots, and the
  // per-lane scan of global memory it replaced waited out one load latency per target (~0.23 ms per
  // 2048-target launch in the bench step).
  bool anyf = false;
#pragma unroll
  for (int i = 0; i < Q; ++i) anyf = anyf || full[i];
  if (__syncthreads_or(anyf)) {
#pragma unroll
    for (int i = 0; i < Q; ++i)
      if (full[i]) bestv[i] = INFINITY, bkv[i] = 0;
    for (int t0 = 0; t0 < NT; t0 += kTile) {
      const int cnt = min(kTile, NT - t0);
      __syncthreads();   // the previous tile is consumed
      for (int e = tid; e < cnt; e += kThreads) {
        const float *src = T + (size_t)(t0 + e) * 3;
        tile[e] = make_float4(src[0], src[1], src[2], 0.f);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        if (!full[i]) continue;
        float best = bestv[i];
        int bk = bkv[i];
        // 8 targets' LDS reads issued together, then compared in index order
        int e = 0;
        for (; e + 8 <= cnt; e += 8) {
          float4 p[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) p[j] = tile[e + j];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = sqd3(p[j].x - ax[i], p[j].y - ay[i], p[j].z - az[i]);
            if (d < best) {
              best = d;
              bk = t0 + e + j;
            }
          }
        }
        for (; e < cnt; ++e) {
          const float4 p = tile[e];
          const float d = sqd3(p.x - ax[i], p.y - ay[i], p.z - az[i]);
          if (d < best) {
            best = d;
            bk = t0 + e;
          }
        }
        bestv[i] = best, bkv[i] = bk;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int qi = bx * kThreads * Q + i * kThreads + tid;
    if (qi >= NA) {
      if (CNT && qi < NAp) dist[qi] = 0.f, idx[qi] = 0;
      continue;
    }
    const float best = bestv[i];
    const int bk = bkv[i];
    dist[qi] = (raw[i] || best < INFINITY) ? best
                                           : sqd3(T[3 * bk] - ax[i], T[3 * bk + 1] - ay[i], T[3 * bk + 2] - az[i]);
    idx[qi] = bk;
  }
}

// ---------------------------------------------------------------- screened on MFMA
// The same screen with e(t) = |t|^2 - 2 a.t formed by the fp32 matrix cores: per wave 32 queries
// (B operand, one per lane pair: column j = lane & 31) against 32-target tiles (A operand, row
// i = target), K = 4 over t' = (x, y, z, |t|^2) and a' = (-2a, 1): two v_mfma_f32_32x32x2_f32 per
// 1024 pairs.  A lane then holds 16 of its query's 32 e values per tile (rows 8g + 4h + c); two
// tiles (64 targets, one slot's range) go through one v_min3 chain, one v_permlane32_swap with the
// other half and the VALU kernel's keep / prune logic (the two halves of a lane pair run it
// identically; the h = 0 lane re-derives and writes) -- the bookkeeping per 32-target sub-tile had
// made this form VALU-bound again.  Per pair: 4 MFMA MACs + ~1/2 VALU op instead of 3 fma + 1/2
// min on the VALU.  Margin: any fp32 evaluation
// order of the 4-term sum errs by <= ~4u (|t|^2 + 2|a||t|) <= 16u (Tm^2 + |a| Tm), the eps below,
// plus an absolute floor for flushed denormal products.
typedef float f32x16m __attribute__((ext_vector_type(16)));

template <int kSubM>   // targets per keep test / slot: kSubM / 32 MFMA tiles (default 64)
__global__ __launch_bounds__(kThreads) void chamfer_mfma_kernel(const float *__restrict__ xyz1,
                                                                const float *__restrict__ xyz2, int N, int M,
                                                                float *__restrict__ dist1, float *__restrict__ dist2,
                                                                int *__restrict__ idx1, int *__restrict__ idx2,
                                                                int blocks_dir0) {
  const int b = blockIdx.y;
  const bool dir = (int)blockIdx.x >= blocks_dir0;
  const int bx = dir ? blockIdx.x - blocks_dir0 : blockIdx.x;
  const int NA = dir ? M : N, NT = dir ? N : M;
  const float *A = (dir ? xyz2 : xyz1) + (size_t)b * NA * 3;
  const float *T = (dir ? xyz1 : xyz2) + (size_t)b * NT * 3;
  float *dist = (dir ? dist2 : dist1) + (size_t)b * NA;
  int *idx = (dir ? idx2 : idx1) + (size_t)b * NA;
  if (NT <= 0) return;
  const bool nanst = nan_chunk_starts(T, NT);

  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, w = tid >> 6;
  const int qi = bx * (kThreads / 2) + w * 32 + (lane & 31);
  const int qc = qi < NA ? qi : NA - 1;
  const float ax = A[3 * qc], ay = A[3 * qc + 1], az = A[3 * qc + 2];
  const float b1 = h ? -2.f * ay : -2.f * ax;  // B[k][j]: k = h (first MFMA), 2 + h (second)
  const float b2 = h ? 1.f : -2.f * az;
  const float an = (ax * ax + ay * ay) + az * az;
  const float anorm = sqrtf(an);
  float mine = INFINITY, slack = INFINITY;
  float cm[kSlots];
  int cs[kSlots];
  bool over = !(an < INFINITY);
#pragma unroll
  for (int c = 0; c < kSlots; ++c) {
    cm[c] = INFINITY;
    cs[c] = -1;
  }

  __shared__ float2 txz[kTile], tyw[kTile];
  __shared__ float tmax_s[kThreads / 64];
  float eps_t2 = 0.f;
  for (int t0 = 0; t0 < NT; t0 += kTile) {
    const int cnt = min(kTile, NT - t0);
    float lmax = 0.f;
    for (int e = tid; e < kTile; e += kThreads) {
      float2 xz = make_float2(0.f, 0.f), yw = make_float2(0.f, INFINITY);  // padding: e = +inf
      if (e < cnt) {
        const float *src = T + (size_t)(t0 + e) * 3;
        const float x = src[0], y = src[1], z = src[2];
        const float n2 = (x * x + y * y) + z * z;
        xz = make_float2(x, z);
        yw = make_float2(y, n2);
        lmax = fmaxf(lmax, n2);
      }
      txz[e] = xz;
      tyw[e] = yw;
    }
    lmax = wave_max_f32(lmax);
    if ((tid & 63) == 0) tmax_s[tid >> 6] = lmax;
    __syncthreads();
#pragma unroll
    for (int ww = 0; ww < kThreads / 64; ++ww) eps_t2 = fmaxf(eps_t2, tmax_s[ww]);
    const float tm = sqrtf(eps_t2);
    const float eps = 16.f * kU * (eps_t2 + anorm * tm) + 1e-35f;
    slack = screen_slack(mine, an, eps);
    over = over || !(eps_t2 + 2.f * anorm * tm < 1e38f);  // near fp32 overflow: direct scan
    const int nsub = (cnt + kSubM - 1) / kSubM;
    for (int sb = 0; sb < nsub; ++sb) {
      // kSubM / 32 independent 32 x 32 tiles, then one keep test for the kSubM targets
      const float2 *src = (h ? tyw : txz) + sb * kSubM + (lane & 31);
      float2 v[kSubM / 32];
#pragma unroll
      for (int u = 0; u < kSubM / 32; ++u) v[u] = src[32 * u];
      f32x16m acc[kSubM / 32];
#pragma unroll
      for (int u = 0; u < kSubM / 32; ++u) {
        acc[u] = f32x16m{};
        acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[u].x, b1, acc[u], 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kSubM / 32; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[u].y, b2, acc[u], 0, 0, 0);
      float m = INFINITY;
#pragma unroll
      for (int u = 0; u < kSubM / 32; ++u)
#pragma unroll
        for (int r = 0; r < 16; r += 2) m = fminf(fminf(m, acc[u][r]), acc[u][r + 1]);
      const auto pr = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
      m = fminf(__uint_as_float(pr[0]), __uint_as_float(pr[1]));
      const int sub0 = t0 + sb * kSubM;
      if (m <= mine + slack) {  // rare: this sub-tile may hold the argmin
        if (m < mine) {
          mine = m;
          slack = screen_slack(mine, an, eps);
#pragma unroll
          for (int c = 0; c < kSlots; ++c)
            if (cs[c] >= 0 && cm[c] > mine + slack) cs[c] = -1;  // prune
        }
        bool placed = false;
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
          if (!placed && cs[c] < 0) {
            cs[c] = sub0;
            cm[c] = m;
            placed = true;
          }
        }
        over = over || !placed;
      }
    }
    __syncthreads();
  }
  if (h || qi >= NA) return;
  // exact re-derivation with the reference expression (chamfer_screen_kernel's)
  float best = INFINITY;
  int bk = 0;
  if (nanst || !finite3(ax, ay, az)) {
    ref_scan(T, NT, ax, ay, az, best, bk);
    dist[qi] = best;
    idx[qi] = bk;
    return;
  }
  if (!over) {
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
      if (cs[c] < 0) continue;
      const int k0 = cs[c], k1 = min(k0 + kSubM, NT);
      for (int k = k0; k < k1; ++k) {
        const float d = sqd3(T[3 * k] - ax, T[3 * k + 1] - ay, T[3 * k + 2] - az);
        if (d < best || (d == best && k < bk)) {
          best = d;
          bk = k;
        }
      }
    }
  }
  if (over || !(best < INFINITY)) {  // full direct scan (overflow, non-finite data)
    best = INFINITY;
    bk = 0;
    for (int k = 0; k < NT; ++k) {
      const float d = sqd3(T[3 * k] - ax, T[3 * k + 1] - ay, T[3 * k + 2] - az);
      if (d < best) {
        best = d;
        bk = k;
      }
    }
  }
  dist[qi] = best < INFINITY ? best : sqd3(T[3 * bk] - ax, T[3 * bk + 1] - ay, T[3 * bk + 2] - az);
  idx[qi] = bk;
}

// own terms: grad_self[j] = 2 g_j (x_j - y_idx(j)), both directions
__global__ void chamfer_grad_own_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int B, int N,
                                        int M, const float *__restrict__ gd1, const float *__restrict__ gd2,
                                        const int *__restrict__ idx1, const int *__restrict__ idx2,
                                        float *__restrict__ g1, float *__restrict__ g2) {
  const size_t tot1 = (size_t)B * N, tot = tot1 + (size_t)B * M;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const bool dir = e >= tot1;
    const size_t pj = dir ? e - tot1 : e;
    const int NA = dir ? M : N, NT = dir ? N : M;
    const size_t b = pj / NA;
    const float *P = dir ? xyz2 : xyz1;
    const float *Tt = dir ? xyz1 : xyz2;
    const int j2 = (dir ? idx2 : idx1)[pj];
    const float g = (dir ? gd2 : gd1)[pj] * 2.f;
    float *G = dir ? g2 : g1;
    const float *p = P + pj * 3;
    const float *q = Tt + (b * NT + ((unsigned)j2 < (unsigned)NT ? j2 : 0)) * 3;
    G[pj * 3 + 0] = g * (p[0] - q[0]);
    G[pj * 3 + 1] = g * (p[1] - q[1]);
    G[pj * 3 + 2] = g * (p[2] - q[2]);
  }
}

// partner terms: grad_other[idx(j)] -= 2 g_j (x_j - y_idx(j))
__global__ void chamfer_grad_partner_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int B,
                                            int N, int M, const float *__restrict__ gd1, const float *__restrict__ gd2,
                                            const int *__restrict__ idx1, const int *__restrict__ idx2,
                                            float *__restrict__ g1, float *__restrict__ g2) {
  const size_t tot1 = (size_t)B * N, tot = tot1 + (size_t)B * M;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const bool dir = e >= tot1;
    const size_t pj = dir ? e - tot1 : e;
    const int NA = dir ? M : N, NT = dir ? N : M;
    const size_t b = pj / NA;
    const float *P = dir ? xyz2 : xyz1;
    const float *Tt = dir ? xyz1 : xyz2;
    const int j2 = (dir ? idx2 : idx1)[pj];
    if ((unsigned)j2 >= (unsigned)NT) continue;
    const float g = (dir ? gd2 : gd1)[pj] * 2.f;
    float *G = dir ? g1 : g2;
    const float *p = P + pj * 3;
    const float *q = Tt + (b * NT + j2) * 3;
    float *dst = G + (b * NT + j2) * 3;
    atomicAdd(dst + 0, -(g * (p[0] - q[0])));
    atomicAdd(dst + 1, -(g * (p[1] - q[1])));
    atomicAdd(dst + 2, -(g * (p[2] - q[2])));
  }
}

// Deterministic backward.  Direction d = 0: sources = cloud 1 (NN idx1 into cloud 2),
// targets = cloud 2; d = 1 the other way.  Block (part, d, b) owns targets [j0, j1) and writes
//   grad_T[j] = own_T[j] - sum_{i : idx_S[i] = j} c_i,   c_i = 2 gd_S[i] (s_i - t_j)
//   own_T[j]  = 2 gd_T[j] (t_j - s_{idx_T[j]})
// (the reference's expressions, chamfer3D.cu:155-174).  Pass 1 finds the largest finite |c| of
// the block's targets; the scale 2^sh makes every term and every possible sum (at most NA
// terms) fit int64, and pass 2 adds round(c * 2^sh) with LDS 64-bit integer atomics: exact and
// order-independent.  Each term is rounded to 2^-sh, so the sum of target j's n_j terms errs by
// at most n_j * 2^-(sh+1) = n_j * 2^(e+lg-63) (|c| < 2^e over the whole BLOCK, NA < 2^lg): an
// ABSOLUTE resolution set by the block's largest term, ~max|c| * 2^-48 per term at NA = 16384 --
// a target whose own terms are far below an outlier of its block gets that absolute bound, not
// fp32-relative precision (tests/test_gpu_pointops.py::test_chamfer_backward_outlier_block_bound).
// Then one rounding to fp32 (the reference's fp32 atomic sum errs by ~2^-24 of the sum of |c|
// and varies run to run).
// Non-finite terms set per-component flags (+inf / -inf / NaN, atomicOr): the sum is then
// +-inf or NaN from the flags alone, again whatever the order.
constexpr int kGThreads = 512;
constexpr int kGTargets = 2048;   // targets per block at most: 2048 x (3 x 8 + 4) B = 56 KB of LDS

// CNT (pcops_chamfer_backward_counts; CNT = false is the uniform instantiation, cnt1 / cnt2 unused): the
// target ranges are cut from the padded row count NTp -- the grid cannot depend on a count the host
// never reads -- and stop at the target cloud's count; the source scan stops at the source count,
// so the scale 2^sh is set by valid terms only and an absent row's incoming gradient is never
// read.  Absent rows of a range, and every row of a pair with an empty side, get a zero gradient.
template <bool CNT = false>
__global__ __launch_bounds__(kGThreads) void chamfer_grad_seg_kernel(
    const float *__restrict__ xyz1, const float *__restrict__ xyz2, int N, int M, const float *__restrict__ gd1,
    const float *__restrict__ gd2, const int *__restrict__ idx1, const int *__restrict__ idx2, float *__restrict__ g1,
    float *__restrict__ g2, int parts0, int parts1, const int *__restrict__ cnt1 = nullptr,
    const int *__restrict__ cnt2 = nullptr) {
  __shared__ long long acc[kGTargets * 3];
  __shared__ int flags[kGTargets];
  __shared__ float red[kGThreads / 64];
  // 1-D grid, XCD-contiguous: consecutive logical blocks -- the parts of one (batch,
  // direction), which all rescan the same source indices -- are dispatched to the same
  // XCD (hardware block h runs on XCD h % 8), so the rescans hit that XCD's L2 instead of
  // each XCD fetching the cloud from HBM
  const int per = parts0 + parts1, total = (int)gridDim.x;
  int L = blockIdx.x;
  if ((total & 7) == 0) L = (L & 7) * (total >> 3) + (L >> 3);
  const int b = L / per, x = L - b * per, tid = threadIdx.x;
  const bool dir = x >= parts0;
  const int part = dir ? x - parts0 : x;
  const int parts = dir ? parts1 : parts0;
  const int NAp = dir ? M : N, NTp = dir ? N : M;
  const int NA = cloud_count<CNT>(dir ? cnt2 : cnt1, b, NAp), NT = cloud_count<CNT>(dir ? cnt1 : cnt2, b, NTp);
  const float *S = (dir ? xyz2 : xyz1) + (size_t)b * NAp * 3;
  const float *T = (dir ? xyz1 : xyz2) + (size_t)b * NTp * 3;
  const float *gS = (dir ? gd2 : gd1) + (size_t)b * NAp;
  const int *iS = (dir ? idx2 : idx1) + (size_t)b * NAp;
  const float *gT = (dir ? gd1 : gd2) + (size_t)b * NTp;
  const int *iT = (dir ? idx1 : idx2) + (size_t)b * NTp;
  float *out = (dir ? g1 : g2) + (size_t)b * NTp * 3;
  const int R = (NTp + parts - 1) / parts;
  const int j0 = part * R, j1 = min(NA > 0 || !CNT ? NT : 0, j0 + R);
  if (CNT) {  // the range's absent rows (all of them when either side is empty)
    for (int e = max(j0, j1) * 3 + tid; e < min(NTp, j0 + R) * 3; e += kGThreads) out[e] = 0.f;
  }
  if (j0 >= j1) return;

  // pass 1: the largest finite |partner term| of this block's targets
  float mx = 0.f;
  for (int i = tid; i < NA; i += kGThreads) {
    const int j = iS[i];
    if (j < j0 || j >= j1) continue;
    const float g = gS[i] * 2.f;
    const float *p = S + (size_t)i * 3, *q = T + (size_t)j * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = fabsf(g * (p[k] - q[k]));
      if (c <= 3.4028234e38f) mx = fmaxf(mx, c);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  for (int e = tid; e < (j1 - j0) * 3; e += kGThreads) acc[e] = 0;
  for (int e = tid; e < j1 - j0; e += kGThreads) flags[e] = 0;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < kGThreads / 64; ++w) mx = fmaxf(mx, red[w]);
  int e2 = 0;
  (void)frexpf(mx, &e2);                                 // mx < 2^e2
  const int lg = 32 - __builtin_clz((unsigned)NA | 1u);  // NA < 2^lg terms per sum at most
  const int sh = mx > 0.f ? 62 - e2 - lg : 0;
  // pass 2: fixed-point adds of the finite terms, flags for the others
  for (int i = tid; i < NA; i += kGThreads) {
    const int j = iS[i];
    if (j < j0 || j >= j1) continue;
    const float g = gS[i] * 2.f;
    const float *p = S + (size_t)i * 3, *q = T + (size_t)j * 3;
    const int jj = j - j0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = g * (p[k] - q[k]);
      if (fabsf(c) <= 3.4028234e38f)
        atomicAdd(reinterpret_cast<unsigned long long *>(acc + jj * 3 + k),
                  (unsigned long long)__builtin_llrint(__builtin_ldexp((double)c, sh)));
      else
        atomicOr(flags + jj, 1 << (3 * k + (c != c ? 2 : (c > 0.f ? 0 : 1))));
    }
  }
  __syncthreads();
  // every target of the block: own term minus the partner sum, written once
  for (int jj = tid; jj < j1 - j0; jj += kGThreads) {
    const int j = j0 + jj;
    const int a = iT[j];
    const float g = gT[j] * 2.f;
    const float *t = T + (size_t)j * 3, *s2 = S + (size_t)((unsigned)a < (unsigned)NA ? a : 0) * 3;
    const int f = flags[jj];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float own = g * (t[k] - s2[k]);
      const int fk = (f >> (3 * k)) & 7;
      double sum = __builtin_ldexp((double)acc[jj * 3 + k], -sh);
      if (fk) sum = (fk & 4) || fk == 3 ? (double)NAN : (fk == 1 ? (double)INFINITY : -(double)INFINITY);
      out[(size_t)j * 3 + k] = (float)((double)own - sum);
    }
  }
}

// ---------------------------------------------------------------- spatially culled
// Large clouds (the loss's 16384^2): both clouds counting-sorted by a 16^3 Morton cell code of
// their own box (chamfer_cull_prep_kernel), targets cut into tiles of kCullTS sorted points with
// exact bounding boxes.  A wave owns 64 consecutive sorted queries (a compact region): it
// scans the tile nearest its box first, then the others outward in sorted order, skipping every
// tile whose box lies farther than the wave's largest current best distance.  Pairs are
// evaluated with the reference expression (sqd3) and the winner kept in (distance, index)
// order, lowest original index on ties -- the reference's bits and tie rule without its
// index-order scan.  Skip test: the box distance lb (fp32) is shrunk by 64u before comparing,
// which covers the fp32 rounding of both the box gaps and any pair's sqd3 (<= ~11u relative),
// so a skipped tile holds no pair at or below the best; below 1e-30 nothing is skipped
// (denormal scale).  A cloud with a non-finite coordinate disables the culling for its batch
// (every tile scanned) and sends the queries ref_scan covers there.
#ifndef PCOPS_CULL_TS
#define PCOPS_CULL_TS 64  // A/B builds: -DPCOPS_CULL_TS=32 (one point per lane: <= 64)
#endif
constexpr int kCullQB = 256, kCullTS = PCOPS_CULL_TS, kCullMaxTiles = 512, kCellBits = 4, kCells = 1 << (3 * kCellBits);

// Visited-pair counting (a separate build, -DPCOPS_COUNT_PAIRS, libpcops_count.so; never the
// product library): the (query, target) pairs the culled search evaluates, per pass --
// [0] pass-1 screen lanes (a scanned tile costs every lane of the wave kCullTS pairs: lanes
// whose own box test failed ride along), [1] pass-2 exact re-derivation rows, [2] reference
// scans.  Each lane sums its own counts and adds them once at its end; read back by
// pcops_debug_pair_counts (tools/chamfer_visited.py prices the bench's launches on them).
#ifdef PCOPS_COUNT_PAIRS
__device__ unsigned long long g_pairs[3];
#define PAIRS_DECL unsigned long long np1 = 0, np2 = 0, np3 = 0
#define PAIRS_ADD(v, n) (v += (unsigned long long)(n))
#define PAIRS_FLUSH()                   \
  do {                                  \
    atomicAdd(&g_pairs[0], np1);        \
    atomicAdd(&g_pairs[1], np2);        \
    atomicAdd(&g_pairs[2], np3);        \
  } while (0)
#else
#define PAIRS_DECL
#define PAIRS_ADD(v, n) ((void)0)
#define PAIRS_FLUSH() ((void)0)
#endif

__device__ __forceinline__ int cull_cell(float x, float y, float z, const float *g) {
  auto ax = [](float v, float lo, float sc) {
    const float t = fminf(fmaxf((v - lo) * sc, 0.f), float((1 << kCellBits) - 1));  // NaN -> 0
    return (int)t;
  };
  const int cx = ax(x, g[0], g[3]), cy = ax(y, g[1], g[4]), cz = ax(z, g[2], g[5]);
  int code = 0;
#pragma unroll
  for (int bit = 0; bit < kCellBits; ++bit)
    code |= (((cx >> bit) & 1) << (3 * bit)) | (((cy >> bit) & 1) << (3 * bit + 1)) | (((cz >> bit) & 1) << (3 * bit + 2));
  return code;
}

struct CullWs {
  float4 *srt[2], *lo[2], *hi[2];
  int *flag;
};

// grid (B, 2): cloud c (0 = xyz1, 1 = xyz2) of batch b -> sorted float4 (x, y, z, original index
// bits), tile boxes, non-finite flag.  The order inside a cell comes from LDS atomics (any order
// gives the same result, see above).
__global__ __launch_bounds__(1024) void chamfer_cull_prep_kernel(const float *__restrict__ xyz1,
                                                                 const float *__restrict__ xyz2, int N, int M,
                                                                 CullWs ws) {
  __shared__ int cnt[kCells];
  __shared__ float red[6][16];
  __shared__ float g[6];
  __shared__ int wsum[16];
  const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = c ? M : N;
  const float *pb = (c ? xyz2 : xyz1) + (size_t)b * n * 3;
  float4 *srt = ws.srt[c] + (size_t)b * n;
  const int nt = (n + kCullTS - 1) / kCullTS;
  float4 *lo = ws.lo[c] + (size_t)b * nt, *hi = ws.hi[c] + (size_t)b * nt;
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  for (int i = tid; i < n; i += 1024) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = pb[3 * i + a];
      bad |= !(fabsf(x) < INFINITY);
      v[a] = fminf(v[a], x);
      v[3 + a] = fmaxf(v[3 + a], x);
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    v[a] = a < 3 ? wave_min_f32(v[a]) : wave_max_f32(v[a]);
    if (lane == 0) red[a][w] = v[a];
  }
  for (int k = tid; k < kCells; k += 1024) cnt[k] = 0;
  bad = __syncthreads_or(bad);
  if (tid < 3) {
    float l = red[tid][0], h = red[3 + tid][0];
    for (int j = 1; j < 16; ++j) {
      l = fminf(l, red[tid][j]);
      h = fmaxf(h, red[3 + tid][j]);
    }
    const float ext = h - l;
    const bool ok = ext > 0.f && ext < INFINITY;
    g[tid] = ok ? l : 0.f;
    g[3 + tid] = ok ? float(1 << kCellBits) / ext : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 1024) atomicAdd(&cnt[cull_cell(pb[3 * i], pb[3 * i + 1], pb[3 * i + 2], g)], 1);
  __syncthreads();
  constexpr int PT = kCells / 1024;
  int loc[PT], run = 0;
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    loc[j] = run;
    run += cnt[tid * PT + j];
  }
  int incl = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int base = incl - run;
  for (int j = 0; j < w; ++j) base += wsum[j];
#pragma unroll
  for (int j = 0; j < PT; ++j) cnt[tid * PT + j] = base + loc[j];
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const float x = pb[3 * i], y = pb[3 * i + 1], z = pb[3 * i + 2];
    const int pos = atomicAdd(&cnt[cull_cell(x, y, z, g)], 1);
    srt[pos] = make_float4(x, y, z, __int_as_float(i));
  }
  __syncthreads();  // this block's sorted rows, written above, are read back below
  for (int t = tid; t < nt; t += 1024) {
    float4 l = make_float4(INFINITY, INFINITY, INFINITY, 0.f), h = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    const int e = min(n, (t + 1) * kCullTS);
    for (int k = t * kCullTS; k < e; ++k) {
      const float4 p = srt[k];
      l.x = fminf(l.x, p.x), l.y = fminf(l.y, p.y), l.z = fminf(l.z, p.z);
      h.x = fmaxf(h.x, p.x), h.y = fmaxf(h.y, p.y), h.z = fmaxf(h.z, p.z);
    }
    lo[t] = l;
    hi[t] = h;
  }
  if (tid == 0) ws.flag[b * 2 + c] = bad;
}

// float -> int preserving order (NaN aside): non-negative floats keep their bits, negative ones
// have the magnitude bits flipped
__device__ __forceinline__ int ford(float f) {
  const int b = __float_as_int(f);
  return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float ford_inv(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

__device__ __forceinline__ float box_gap(float qlo, float qhi, float tlo, float thi) {
  return fmaxf(0.f, fmaxf(tlo - qhi, qlo - thi));
}

// grid (blocks of dir 0 + blocks of dir 1, B), kCullQB threads: one sorted query per lane.  Each
// wave is an independent searcher over its 64 queries (its own box, bounds, tile buffer and
// skip decisions): no block barriers, and a 64-query box is ~4x tighter than a block's.
#ifndef PCOPS_CULL_UNR
#define PCOPS_CULL_UNR 4  // pass-1 screen loop unroll (x 2 points): 4 measured 1-2 % faster than 2 and 8 (r5)
#endif
#ifndef PCOPS_CULL_WPE
#define PCOPS_CULL_WPE 7  // occupancy hint: 72 VGPRs, 7 waves / SIMD (LDS allows 7 blocks / CU); A/B builds override
#endif
template <bool ES>
__global__ __launch_bounds__(kCullQB) __attribute__((amdgpu_waves_per_eu(PCOPS_CULL_WPE))) void chamfer_cull_kernel(const float *__restrict__ xyz1,
                                                               const float *__restrict__ xyz2, int N, int M,
                                                               CullWs ws, float *__restrict__ dist1,
                                                               float *__restrict__ dist2, int *__restrict__ idx1,
                                                               int *__restrict__ idx2, int blocks_dir0) {
  constexpr int W = kCullQB / 64, kLbRegs = kCullMaxTiles / 64;
  __shared__ float4 tiles[W][kCullTS];
  __shared__ float4 blo[kCullMaxTiles], bhi[kCullMaxTiles];  // the target tiles' boxes
  // XCD-contiguous (as chamfer_grad_seg_kernel): hardware block h runs on XCD h % 8, so the
  // logical blocks of a (batch, direction) -- which all read the same sorted target cloud and
  // write the same output rows -- are gathered onto one XCD and its L2
  const int gx = (int)gridDim.x, total = gx * (int)gridDim.y;
  int lin = (int)blockIdx.x + (int)blockIdx.y * gx;
  if ((total & 7) == 0) lin = (lin & 7) * (total >> 3) + (lin >> 3);
  const int b = lin / gx, bxl = lin - b * gx, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int dir = bxl >= blocks_dir0;
  const int bx = dir ? bxl - blocks_dir0 : bxl;
  const int NA = dir ? M : N, NT = dir ? N : M;
  const float4 *A = ws.srt[dir] + (size_t)b * NA;
  const float4 *T = ws.srt[1 - dir] + (size_t)b * NT;
  const int nt = (NT + kCullTS - 1) / kCullTS;
  const float4 *tlo = ws.lo[1 - dir] + (size_t)b * nt, *thi = ws.hi[1 - dir] + (size_t)b * nt;
  const float *Torig = (dir ? xyz1 : xyz2) + (size_t)b * NT * 3;
  float *dist = (dir ? dist2 : dist1) + (size_t)b * NA;
  int *idx = (dir ? idx2 : idx1) + (size_t)b * NA;
  const bool bad = ws.flag[b * 2] | ws.flag[b * 2 + 1];
  for (int t = tid; t < nt; t += kCullQB) blo[t] = tlo[t], bhi[t] = thi[t];
  __syncthreads();
  const bool nanst = bad && nan_chunk_starts(Torig, NT);  // block-uniform, before any wave exits
  const int q0 = (bx * W + w) * 64;
  if (q0 >= NA) return;  // whole wave past the end

  const int qs = q0 + lane;
  const bool valid = qs < NA;
  const float4 a = A[valid ? qs : NA - 1];
  // the wave's query box
  const float qx0 = wave_min_f32(a.x), qy0 = wave_min_f32(a.y), qz0 = wave_min_f32(a.z);
  const float qx1 = wave_max_f32(a.x), qy1 = wave_max_f32(a.y), qz1 = wave_max_f32(a.z);
  // lower bounds of the wave's box to every target tile, tile t = lane + 64 i in L[i]; clamped
  // to FLT_MAX so that +inf marks a tile already taken
  float L[kLbRegs];
#pragma unroll
  for (int i = 0; i < kLbRegs; ++i) {
    const int t = lane + 64 * i;
    L[i] = INFINITY;
    if (t < nt) {
      const float4 l = blo[t], h = bhi[t];
      const float gx = box_gap(qx0, qx1, l.x, h.x), gy = box_gap(qy0, qy1, l.y, h.y), gz = box_gap(qz0, qz1, l.z, h.z);
      L[i] = bad ? -INFINITY : fminf((gx * gx + gy * gy) + gz * gz, FLT_MAX) * (1.f - 64.f * kU);
    }
  }
  // take the untaken tile of smallest bound (nearest-first order; which of several equal bounds
  // is taken first changes neither the result nor the culling's soundness).  The wave argmin is
  // DPP (float bits mapped to a monotone int) + a ballot: the ds_bpermute form (12 dependent LDS
  // round trips per tile, with the mb maximum below) cost more than the tile's 64-pair screen.
  auto take = [&](float &m, int &t) {
    float lm = INFINITY;
    int mi = 0;
#pragma unroll
    for (int i = 0; i < kLbRegs; ++i)
      if (L[i] < lm) lm = L[i], mi = i;
    const int key = ford(lm);
    const int kmin = wave_min_i32_dpp(key);                 // uniform
    const int wl = (int)__builtin_ctzll(__ballot(key == kmin));
    const int wmi = __builtin_amdgcn_readlane(mi, wl);
    m = ford_inv(kmin);
    t = wl + 64 * wmi;
    if (lane == wl) {
#pragma unroll
      for (int i = 0; i < kLbRegs; ++i)
        if (i == wmi) L[i] = INFINITY;
    }
  };
  auto fetch = [&](float m, int t) {  // the tile's points, one per lane (issued a tile ahead)
    const int k = t * kCullTS + lane;
    return (m < INFINITY && lane < kCullTS && k < NT) ? T[k] : make_float4(NAN, NAN, NAN, __int_as_float(INT_MAX));
  };

  float4 *tile = tiles[w];
  // pass 1.  ES = false: per query the smallest distance (the direct expression + v_min, 6.5 VALU
  // per pair), the tile holding it and whether another scanned tile reached the same minimum.
  // ES = true: chamfer_screen_kernel's screen over the visited tiles -- e = |t|^2 - 2a.t (3 fma +
  // 1/2 v_min per pair), its rounding margin and <= kSlots candidate tiles per query -- with the
  // upper bound U = min e + |a|^2 + slack on the direct best distance as the culling bound.
  float best = INFINITY;  // ES = false: the best distance; ES = true: U
  int btile = 0;
  bool tie = false;
  const float mx = -2.f * a.x, my = -2.f * a.y, mz = -2.f * a.z;
  const float an = (a.x * a.x + a.y * a.y) + a.z * a.z, anorm = sqrtf(an);
  float mine = INFINITY, slack = INFINITY, eps_t2 = 0.f;
  float cm[kSlots];
  int cs[kSlots];
#pragma unroll
  for (int c = 0; c < kSlots; ++c) cm[c] = INFINITY, cs[c] = -1;
  bool over = bad || !(an < INFINITY);
  PAIRS_DECL;
  float mb = INFINITY;  // the wave's largest current bound (scalar)
  float m;
  int t;
  take(m, t);
  float4 pf = fetch(m, t);
  for (; !(ES && bad);) {  // (a non-finite batch: every query re-derived below by a full scan)
    if (m == INFINITY) break;         // every tile taken
    if (m > mb && m > 1e-30f) break;  // every untaken tile lies beyond every query's best
    const int tc = t;
    float4 cur = pf;
    take(m, t);  // the next tile, its points in flight while this one is scanned
    pf = fetch(m, t);
    // per-query test against the tile's box: the tile is scanned only if some query may improve
    const float4 l = blo[tc], h = bhi[tc];
    const float px = fmaxf(0.f, fmaxf(l.x - a.x, a.x - h.x)), py = fmaxf(0.f, fmaxf(l.y - a.y, a.y - h.y)),
                pz = fmaxf(0.f, fmaxf(l.z - a.z, a.z - h.z));
    const float pl = ((px * px + py * py) + pz * pz) * (1.f - 64.f * kU);
    const bool need = valid && (bad || !(pl > best) || pl <= 1e-30f);
    if (!__any(need)) continue;
    if (valid) PAIRS_ADD(np1, kCullTS);
    if (ES) cur.w = (cur.x * cur.x + cur.y * cur.y) + cur.z * cur.z;  // |t|^2 (NaN padding stays NaN)
    // one wave: its LDS accesses complete in issue order, the wave barriers keep the compiler's
    __builtin_amdgcn_wave_barrier();
    if (lane < kCullTS) tile[lane] = cur;
    __builtin_amdgcn_wave_barrier();
    float mt = INFINITY;
    if (ES) {
#pragma unroll PCOPS_CULL_UNR
      for (int kk = 0; kk < kCullTS; kk += 2) {
        const float4 p0 = tile[kk], p1 = tile[kk + 1];
        const float e0 = __builtin_fmaf(mz, p0.z, __builtin_fmaf(my, p0.y, __builtin_fmaf(mx, p0.x, p0.w)));
        const float e1 = __builtin_fmaf(mz, p1.z, __builtin_fmaf(my, p1.y, __builtin_fmaf(mx, p1.x, p1.w)));
        mt = fminf(fminf(mt, e0), e1);
      }
      // Tm^2: running max over the visited tiles of their box's farthest corner
      const float cx = fmaxf(fabsf(l.x), fabsf(h.x)), cy = fmaxf(fabsf(l.y), fabsf(h.y)),
                  cz = fmaxf(fabsf(l.z), fabsf(h.z));
      eps_t2 = fmaxf(eps_t2, ((cx * cx + cy * cy) + cz * cz) * (1.f + 8.f * kU));
      const float tm = sqrtf(eps_t2);
      const float eps = 16.f * kU * (eps_t2 + anorm * tm);
      const bool ovf = !(eps_t2 + 2.f * anorm * tm < 1e38f);  // near fp32 overflow: e may be +-inf / NaN
      over = over || ovf;                                      // -> full re-derivation, no culling
      slack = screen_slack(mine, an, eps);
      if (mt <= mine + slack) {  // this tile may hold the argmin (the screen's keep / prune)
        if (mt < mine) {
          mine = mt;
          slack = screen_slack(mine, an, eps);
#pragma unroll
          for (int c = 0; c < kSlots; ++c)
            if (cs[c] >= 0 && cm[c] > mine + slack) cs[c] = -1;
        }
        bool placed = false;
#pragma unroll
        for (int c = 0; c < kSlots; ++c)
          if (!placed && cs[c] < 0) cs[c] = tc, cm[c] = mt, placed = true;
        over = over || !placed;
      }
      best = mine + an + slack;
      if (ovf || !(best >= 0.f)) best = INFINITY;  // no valid bound: this query culls nothing
    } else {
#pragma unroll 2
      for (int kk = 0; kk < kCullTS; kk += 2) {
        const float4 p0 = tile[kk], p1 = tile[kk + 1];
        mt = fminf(fminf(mt, sqd3(p0.x - a.x, p0.y - a.y, p0.z - a.z)), sqd3(p1.x - a.x, p1.y - a.y, p1.z - a.z));
      }
      if (mt < best)
        best = mt, btile = tc, tie = false;
      else if (mt == best)
        tie = true;
    }
    mb = ford_inv(wave_max_i32(ford(valid ? best : -INFINITY)));   // DPP, uniform
  }
  if (!valid) return;
  int bidx = INT_MAX;
  auto scan_tile = [&](int u) {   // the tile's sorted rows in batches of kRd loads issued together
    const int ke = min(NT, u * kCullTS + kCullTS);
    PAIRS_ADD(np2, ke - u * kCullTS);
    for (int kb = u * kCullTS; kb < ke; kb += kRd) {
      float4 pr[kRd];
#pragma unroll
      for (int j = 0; j < kRd; ++j) pr[j] = T[min(kb + j, ke - 1)];
#pragma unroll
      for (int j = 0; j < kRd; ++j) {
        const float d = sqd3(pr[j].x - a.x, pr[j].y - a.y, pr[j].z - a.z);
        const int ti = __float_as_int(pr[j].w);
        if (kb + j < ke && (d < best || (d == best && ti < bidx))) best = d, bidx = ti;
      }
    }
  };
  // every tile whose box is within `bound` (all of them in a non-finite batch)
  auto scan_within = [&](float bound) {
    best = INFINITY;
    bidx = INT_MAX;
    for (int u = 0; u < nt; ++u) {
      if (!bad) {
        const float4 l = blo[u], h = bhi[u];
        const float px = fmaxf(0.f, fmaxf(l.x - a.x, a.x - h.x)), py = fmaxf(0.f, fmaxf(l.y - a.y, a.y - h.y)),
                    pz = fmaxf(0.f, fmaxf(l.z - a.z, a.z - h.z));
        const float pl = ((px * px + py * py) + pz * pz) * (1.f - 64.f * kU);
        if (pl > bound && pl > 1e-30f) continue;
      }
      scan_tile(u);
    }
  };
  if (nanst || !finite3(a.x, a.y, a.z)) {
    PAIRS_ADD(np3, NT);
    ref_scan(Torig, NT, a.x, a.y, a.z, best, bidx);
  } else if (ES) {
    // pass 2, the exact (distance, original index) winner: over the candidate tiles, or -- on
    // slot overflow / non-finite data / overflow risk -- over every tile within U
    const float bound = best;
    best = INFINITY;
    if (!over) {
#pragma unroll
      for (int c = 0; c < kSlots; ++c)
        if (cs[c] >= 0) scan_tile(cs[c]);
    }
    if (over || !(best < INFINITY)) scan_within(bad ? INFINITY : bound);
  } else {
    // pass 2, the exact (distance, original index) winner: the best tile alone, or -- when
    // another tile tied -- every tile whose box is within the best (the culling test above)
    const float bound = best;
    if (tie) {
      scan_within(bound);
    } else {
      best = INFINITY;
      scan_tile(btile);
    }
  }
  if (bidx == INT_MAX) bidx = 0;
  const int oq = __float_as_int(a.w);
  dist[oq] = best;
  idx[oq] = bidx;
  PAIRS_FLUSH();
}

size_t cull_ws_bytes(int B, int N, int M) {
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t nt1 = (N + kCullTS - 1) / kCullTS, nt2 = (M + kCullTS - 1) / kCullTS;
  return al((size_t)B * N * 16) + al((size_t)B * M * 16) + 2 * al((size_t)B * nt1 * 16) + 2 * al((size_t)B * nt2 * 16) +
         al((size_t)B * 8);
}

bool cull_applies(int N, int M) {
  static const bool on = [] {  // PCOPS_CHAMFER_CULL=0: the all-pairs screens only (A/B)
    const char *e = getenv("PCOPS_CHAMFER_CULL");
    return !(e && e[0] == '0');
  }();
  // measured (B = 32, surface clouds, tools/chamfer_bench.py): 512^2 0.055 vs 0.027 ms for the
  // screen, 2048^2 0.093 vs 0.075, 2048 x 16384 0.32 vs 0.54, 16384^2 0.41 vs 1.75 -> cull from
  // 2^24 pairs per cloud pair; PCOPS_CHAMFER_CULL_MIN: smallest cloud culled (A/B)
  static const int lo = [] {
    const char *e = getenv("PCOPS_CHAMFER_CULL_MIN");
    return e ? atoi(e) : 256;
  }();
  static const long long pairs = [] {  // PCOPS_CHAMFER_CULL_PAIRS: smallest N * M culled (A/B)
    const char *e = getenv("PCOPS_CHAMFER_CULL_PAIRS");
    return e ? atoll(e) : (1LL << 24);
  }();
  return on && N >= lo && M >= lo && (long long)N * M >= pairs && (N + kCullTS - 1) / kCullTS <= kCullMaxTiles &&
         (M + kCullTS - 1) / kCullTS <= kCullMaxTiles;
}

}  // namespace

#ifdef PCOPS_COUNT_PAIRS
// counting build only (not in include/pcops.h): copy the three pair counters to host memory
// `out` and zero them; synchronises the device
extern "C" int pcops_debug_pair_counts(unsigned long long *out) {
  if (hipDeviceSynchronize() != hipSuccess) return PCOPS_ERR_LAUNCH;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pairs), sizeof(unsigned long long) * 3) != hipSuccess)
    return PCOPS_ERR_LAUNCH;
  const unsigned long long zero[3] = {0, 0, 0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_pairs), zero, sizeof(zero)) != hipSuccess) return PCOPS_ERR_LAUNCH;
  return PCOPS_OK;
}
#endif

extern "C" int pcops_chamfer_forward(const float *xyz1, const float *xyz2, int B, int N, int M, float *dist1,
                                     float *dist2, int *idx1, int *idx2, pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 0) return PCOPS_ERR_INVALID;
  if (B == 0 || (N == 0 && M == 0)) return PCOPS_OK;
  if (!xyz1 || !xyz2 || (N && (!dist1 || !idx1)) || (M && (!dist2 || !idx2))) return PCOPS_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0 || M == 0) {  // reference leaves the zero-initialised outputs untouched
    if (N && (pc_memset_async(dist1, 0, sizeof(float) * B * N, s) || pc_memset_async(idx1, 0, sizeof(int) * B * N, s)))
      return PCOPS_ERR_LAUNCH;
    if (M && (pc_memset_async(dist2, 0, sizeof(float) * B * M, s) || pc_memset_async(idx2, 0, sizeof(int) * B * M, s)))
      return PCOPS_ERR_LAUNCH;
    return PCOPS_OK;
  }
  auto blocks = [&](int q) {
    return (long)B * (((N + kThreads * q - 1) / (kThreads * q)) + ((M + kThreads * q - 1) / (kThreads * q)));
  };
  // measured at B = 32 (tools/gpu_ab_chamfer.sh): the screened kernel wins at
  // every step shape; 4 queries per lane once the grid holds >= 4 blocks per CU
  // (16384^2: 1.55 ms vs 2.06 with Q = 1), 1 below that (2048^2: 0.070 ms vs
  // 0.102 with Q = 2 and 0.172 for the direct kernel)
  int Q = blocks(4) >= 1024 ? 4 : 1;
  if (const char *e = getenv("PCOPS_CHAMFER_Q")) Q = atoi(e);  // A/B experiments: 1, 2, 4, 8
  const int b0 = (N + kThreads * Q - 1) / (kThreads * Q);
  const int b1 = (M + kThreads * Q - 1) / (kThreads * Q);
  const dim3 grid(b0 + b1, B);
  const bool screen = [] {  // PCOPS_CHAMFER_SCREEN=0: the direct kernel (A/B runs, tests)
    const char *e = getenv("PCOPS_CHAMFER_SCREEN");
    return !(e && e[0] == '0');
  }();
  // PCOPS_CHAMFER_MFMA: 0 (default) = the VALU screen only -- the brief reserves the matrix cores
  // for the attention contractions; 1 = the fp32-MFMA screen for the launches the VALU screen runs
  // at Q = 1 (opt-in: B = 32, 2048^2: 0.071 -> 0.048 ms; PCN step 51.88 -> 51.58 ms, same box),
  // 2 = everywhere: at 16384^2 alone it ties the Q = 4 VALU screen (1.67 vs 1.69 ms), in the step it
  // measured 0.4-0.8 ms slower (it shares the matrix cores with the concurrent GEMMs / attention
  // of the other stream); profiles/r3_chamfer_mfma_ab.txt
  const int mfma = [] {
    const char *e = getenv("PCOPS_CHAMFER_MFMA");
    return e ? atoi(e) : 0;
  }();
  if (screen && (mfma == 2 || (mfma == 1 && Q == 1))) {
    const int m0 = (N + kThreads / 2 - 1) / (kThreads / 2), m1 = (M + kThreads / 2 - 1) / (kThreads / 2);
    // PCOPS_CHAMFER_MFMA_SUB: 32 / 64 / 128 / 256 targets per keep test (A/B).  64 measured best
    // (B = 32, 16384^2 / 2048^2: 32 -> 1.80 / 0.051 ms, 64 -> 1.64-1.67 / 0.047-0.049, 128 -> 1.84 /
    // 0.053, 256 -> 2.30 / 0.104): 72 VGPRs (7 waves / SIMD) against 104 / 136 at 128 / 256
    static const int sub = [] {
      const char *e = getenv("PCOPS_CHAMFER_MFMA_SUB");
      return e ? atoi(e) : 64;
    }();
    if (sub == 32)
      hipLaunchKernelGGL(chamfer_mfma_kernel<32>, dim3(m0 + m1, B), dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1,
                         dist2, idx1, idx2, m0);
    else if (sub == 64)
      hipLaunchKernelGGL(chamfer_mfma_kernel<64>, dim3(m0 + m1, B), dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1,
                         dist2, idx1, idx2, m0);
    else if (sub == 256)
      hipLaunchKernelGGL(chamfer_mfma_kernel<256>, dim3(m0 + m1, B), dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1,
                         dist2, idx1, idx2, m0);
    else
      hipLaunchKernelGGL(chamfer_mfma_kernel<128>, dim3(m0 + m1, B), dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1,
                         dist2, idx1, idx2, m0);
    PC_CHECK_LAUNCH();
    return PCOPS_OK;
  }
  if (screen && Q == 4)
    hipLaunchKernelGGL(chamfer_screen_kernel<4>, grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1,
                       idx2, b0);
  else if (screen && Q == 2)
    hipLaunchKernelGGL(chamfer_screen_kernel<2>, grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1,
                       idx2, b0);
  else if (screen && Q == 1)
    hipLaunchKernelGGL(chamfer_screen_kernel<1>, grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1,
                       idx2, b0);
  else if (Q == 8)
    hipLaunchKernelGGL(chamfer_nn_kernel<8>, grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2,
                       b0);
  else if (Q == 4)
    hipLaunchKernelGGL(chamfer_nn_kernel<4>, grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2,
                       b0);
  else if (Q == 2)
    hipLaunchKernelGGL(chamfer_nn_kernel<2>, grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2,
                       b0);
  else
    hipLaunchKernelGGL(chamfer_nn_kernel<1>, grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2,
                       b0);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

extern "C" unsigned long long pcops_chamfer_workspace_bytes(int B, int N, int M) {
  if (B <= 0 || N <= 0 || M <= 0 || !cull_applies(N, M)) return 0;
  return cull_ws_bytes(B, N, M);
}

// pcops_chamfer_forward with scratch: large clouds take the spatially culled search (same
// outputs bit for bit); anything else, or a short workspace, is pcops_chamfer_forward
extern "C" int pcops_chamfer_forward_ws(const float *xyz1, const float *xyz2, int B, int N, int M, float *dist1,
                                        float *dist2, int *idx1, int *idx2, void *workspace,
                                        unsigned long long workspace_bytes, pcops_stream_t stream) {
  if (B <= 0 || N <= 0 || M <= 0 || !cull_applies(N, M) || !workspace || workspace_bytes < cull_ws_bytes(B, N, M))
    return pcops_chamfer_forward(xyz1, xyz2, B, N, M, dist1, dist2, idx1, idx2, stream);
  if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2) return PCOPS_ERR_INVALID;
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  char *w = (char *)workspace;
  const size_t nt1 = (N + kCullTS - 1) / kCullTS, nt2 = (M + kCullTS - 1) / kCullTS;
  CullWs ws;
  ws.srt[0] = (float4 *)w, w += al((size_t)B * N * 16);
  ws.srt[1] = (float4 *)w, w += al((size_t)B * M * 16);
  ws.lo[0] = (float4 *)w, w += al((size_t)B * nt1 * 16);
  ws.hi[0] = (float4 *)w, w += al((size_t)B * nt1 * 16);
  ws.lo[1] = (float4 *)w, w += al((size_t)B * nt2 * 16);
  ws.hi[1] = (float4 *)w, w += al((size_t)B * nt2 * 16);
  ws.flag = (int *)w;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(chamfer_cull_prep_kernel, dim3(B, 2), dim3(1024), 0, s, xyz1, xyz2, N, M, ws);
  const int b0 = (N + kCullQB - 1) / kCullQB, b1 = (M + kCullQB - 1) / kCullQB;
  // PCOPS_CHAMFER_CULL_ES=0: the direct-expression pass 1 (A/B)
  const char *es = getenv("PCOPS_CHAMFER_CULL_ES");
  if (es && es[0] == '0')
    hipLaunchKernelGGL(chamfer_cull_kernel<false>, dim3(b0 + b1, B), dim3(kCullQB), 0, s, xyz1, xyz2, N, M, ws, dist1,
                       dist2, idx1, idx2, b0);
  else
    hipLaunchKernelGGL(chamfer_cull_kernel<true>, dim3(b0 + b1, B), dim3(kCullQB), 0, s, xyz1, xyz2, N, M, ws, dist1,
                       dist2, idx1, idx2, b0);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

// d(loss)/d(dist) of the reference's sqrt-mean Chamfer losses (loss_utils.py: chamfer_sqrt =
// (mean(sqrt(d1)) + mean(sqrt(d2))) / 2, chamfer_single_side_sqrt = mean(sqrt(d1))) in one launch,
// in autograd's own order: t = g * scale (DivBackward of "/ 2", a multiply by 0.5; 1 single-sided),
// t * (1 / n) (MeanBackward: torch divides by a CPU scalar as a multiply by its fp32 reciprocal),
// then / (2 * sqrt(d)) (SqrtBackward) -- bitwise the gradient autograd hands chamfer_3D.backward.
// s2 == nullptr: the second direction takes no gradient (zeros, as for an unused output).
__global__ void chamfer_sqm_grad_kernel(const float *__restrict__ go, float scale, const float *__restrict__ s1,
                                        long long n1, float inv1, const float *__restrict__ s2, long long n2,
                                        float inv2, float *__restrict__ gd1, float *__restrict__ gd2) {
  const float t = go[0] * scale;
  const float t1 = t * inv1, t2 = t * inv2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += stride) {
    if (i < n1)
      gd1[i] = t1 / (2.f * s1[i]);
    else
      gd2[i - n1] = s2 ? t2 / (2.f * s2[i - n1]) : 0.f;
  }
}

extern "C" int pcops_chamfer_sqrt_mean_grad(const float *grad_out, float scale, const float *s1, long long n1,
                                            const float *s2, long long n2, float *gd1, float *gd2,
                                            pcops_stream_t stream) {
  if (n1 < 0 || n2 < 0) return PCOPS_ERR_INVALID;
  if (n1 + n2 == 0) return PCOPS_OK;
  if (!grad_out || (n1 && (!s1 || !gd1)) || (n2 && !gd2)) return PCOPS_ERR_INVALID;
  const float inv1 = n1 ? 1.0f / (float)n1 : 0.f, inv2 = n2 ? 1.0f / (float)n2 : 0.f;
  long long blocks = (n1 + n2 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(chamfer_sqm_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad_out,
                     scale, s1, n1, inv1, s2, n2, inv2, gd1, gd2);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

extern "C" int pcops_chamfer_backward(const float *xyz1, const float *xyz2, int B, int N, int M,
                                      const float *graddist1, const float *graddist2, const int *idx1,
                                      const int *idx2, float *gradxyz1, float *gradxyz2, pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 0) return PCOPS_ERR_INVALID;
  if (B == 0 || (N == 0 && M == 0)) return PCOPS_OK;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0 || M == 0) {
    if (N && pc_memset_async(gradxyz1, 0, sizeof(float) * 3 * B * N, s)) return PCOPS_ERR_LAUNCH;
    if (M && pc_memset_async(gradxyz2, 0, sizeof(float) * 3 * B * M, s)) return PCOPS_ERR_LAUNCH;
    return PCOPS_OK;
  }
  if (!xyz1 || !xyz2 || !graddist1 || !graddist2 || !idx1 || !idx2 || !gradxyz1 || !gradxyz2)
    return PCOPS_ERR_INVALID;
  static const bool atomic_form = [] {  // PCOPS_CHAMFER_BWD=atomic: the two-kernel float-atomic form (A/B)
    const char *e = getenv("PCOPS_CHAMFER_BWD");
    return e && e[0] == 'a';
  }();
  if (!atomic_form) {
    // at least ceil(NT / kGTargets) target ranges per (batch, direction); more (down to 512
    // targets each) while the grid is under 2 blocks per CU
    auto parts_for = [&](int NT) {
      int p = (NT + kGTargets - 1) / kGTargets;
      while ((long)B * 2 * p < 512 && (NT + 2 * p - 1) / (2 * p) >= 512) p *= 2;
      return p;
    };
    const int p0 = parts_for(M), p1 = parts_for(N);
    hipLaunchKernelGGL(chamfer_grad_seg_kernel<>, dim3((unsigned)((long)(p0 + p1) * B)), dim3(kGThreads), 0, s, xyz1,
                       xyz2, N, M, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2, p0, p1);
    PC_CHECK_LAUNCH();
    return PCOPS_OK;
  }
  const size_t tot = (size_t)B * (N + M);
  unsigned grid = (unsigned)((tot + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(chamfer_grad_own_kernel, dim3(grid), dim3(256), 0, s, xyz1, xyz2, B, N, M, graddist1, graddist2,
                     idx1, idx2, gradxyz1, gradxyz2);
  PC_CHECK_LAUNCH();
  hipLaunchKernelGGL(chamfer_grad_partner_kernel, dim3(grid), dim3(256), 0, s, xyz1, xyz2, B, N, M, graddist1,
                     graddist2, idx1, idx2, gradxyz1, gradxyz2);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

// ---------------------------------------------------------------- counted clouds
// Clouds of unequal size in one batch: (B, N, 3) / (B, M, 3) buffers whose cloud b holds counts1[b] /
// counts2[b] points (device int32, clamped to [0, N] / [0, M]; a null pointer = that side is full).
// For its valid rows pair b gets what pcops_chamfer_forward gives (xyz1[b, :c1], xyz2[b, :c2]) --
// the same bodies, swept to the count -- and absent rows get (0, 0).  The counts are read by the
// kernels only: the grid is cut from N and M, so the dispatch depends on B, N and M alone, and a
// block whose queries are all absent ends after writing the padding.  Direct or screened search
// (PCOPS_CHAMFER_SCREEN / PCOPS_CHAMFER_Q as in pcops_chamfer_forward); no MFMA and no culled form.
extern "C" int pcops_chamfer_forward_counts(const float *xyz1, const float *xyz2, const int *counts1,
                                            const int *counts2, int B, int N, int M, float *dist1, float *dist2,
                                            int *idx1, int *idx2, pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 0) return PCOPS_ERR_INVALID;
  if (B == 0 || (N == 0 && M == 0)) return PCOPS_OK;
  if (!counts1 && !counts2) return PCOPS_ERR_INVALID;
  if (!xyz1 || !xyz2 || (N && (!dist1 || !idx1)) || (M && (!dist2 || !idx2))) return PCOPS_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0 || M == 0) {
    if (N && (pc_memset_async(dist1, 0, sizeof(float) * B * N, s) || pc_memset_async(idx1, 0, sizeof(int) * B * N, s)))
      return PCOPS_ERR_LAUNCH;
    if (M && (pc_memset_async(dist2, 0, sizeof(float) * B * M, s) || pc_memset_async(idx2, 0, sizeof(int) * B * M, s)))
      return PCOPS_ERR_LAUNCH;
    return PCOPS_OK;
  }
  auto blocks = [&](int q) {
    return (long)B * (((N + kThreads * q - 1) / (kThreads * q)) + ((M + kThreads * q - 1) / (kThreads * q)));
  };
  int Q = blocks(4) >= 1024 ? 4 : 1;   // pcops_chamfer_forward's rule
  if (const char *e = getenv("PCOPS_CHAMFER_Q")) Q = atoi(e);
  const char *se = getenv("PCOPS_CHAMFER_SCREEN");
  const bool screen = !(se && se[0] == '0');
  if (Q != 1 && Q != 2 && Q != 4 && !(Q == 8 && !screen)) Q = 1;
  const int b0 = (N + kThreads * Q - 1) / (kThreads * Q);
  const int b1 = (M + kThreads * Q - 1) / (kThreads * Q);
  const dim3 grid(b0 + b1, B);
#define PC_CH_CNT(KERNEL, QQ)                                                                                 \
  hipLaunchKernelGGL((KERNEL<QQ, true>), grid, dim3(kThreads), 0, s, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2, \
                     b0, counts1, counts2)
  if (screen && Q == 4)
    PC_CH_CNT(chamfer_screen_kernel, 4);
  else if (screen && Q == 2)
    PC_CH_CNT(chamfer_screen_kernel, 2);
  else if (screen)
    PC_CH_CNT(chamfer_screen_kernel, 1);
  else if (Q == 8)
    PC_CH_CNT(chamfer_nn_kernel, 8);
  else if (Q == 4)
    PC_CH_CNT(chamfer_nn_kernel, 4);
  else if (Q == 2)
    PC_CH_CNT(chamfer_nn_kernel, 2);
  else
    PC_CH_CNT(chamfer_nn_kernel, 1);
#undef PC_CH_CNT
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

// pcops_chamfer_backward over counted clouds: chamfer_grad_seg_kernel's scheme (bitwise
// reproducible), see chamfer_grad_seg_kernel.  graddist rows of absent points are never read.
extern "C" int pcops_chamfer_backward_counts(const float *xyz1, const float *xyz2, const int *counts1,
                                             const int *counts2, int B, int N, int M, const float *graddist1,
                                             const float *graddist2, const int *idx1, const int *idx2,
                                             float *gradxyz1, float *gradxyz2, pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 0) return PCOPS_ERR_INVALID;
  if (B == 0 || (N == 0 && M == 0)) return PCOPS_OK;
  if (!counts1 && !counts2) return PCOPS_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0 || M == 0) {
    if ((N && !gradxyz1) || (M && !gradxyz2)) return PCOPS_ERR_INVALID;
    if (N && pc_memset_async(gradxyz1, 0, sizeof(float) * 3 * B * N, s)) return PCOPS_ERR_LAUNCH;
    if (M && pc_memset_async(gradxyz2, 0, sizeof(float) * 3 * B * M, s)) return PCOPS_ERR_LAUNCH;
    return PCOPS_OK;
  }
  if (!xyz1 || !xyz2 || !graddist1 || !graddist2 || !idx1 || !idx2 || !gradxyz1 || !gradxyz2)
    return PCOPS_ERR_INVALID;
  auto parts_for = [&](int NT) {   // pcops_chamfer_backward's rule, on the padded sizes
    int p = (NT + kGTargets - 1) / kGTargets;
    while ((long)B * 2 * p < 512 && (NT + 2 * p - 1) / (2 * p) >= 512) p *= 2;
    return p;
  };
  const int p0 = parts_for(M), p1 = parts_for(N);
  hipLaunchKernelGGL(chamfer_grad_seg_kernel<true>, dim3((unsigned)((long)(p0 + p1) * B)), dim3(kGThreads), 0, s, xyz1,
                     xyz2, N, M, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2, p0, p1, counts1, counts2);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}

// d(loss)/d(dist) of the counted Chamfer losses, loss = mean_b l_b with l_b the reference's loss on
// cloud pair b cut to its counts, in one launch: t = g * scale (0.5 for chamfer_sqrt's "/ 2", else
// 1), t * (1 / B), t * (1 / c[b]), then / (2 sqrt(d)) when root -- autograd's order for the chain of
// B = 1 calls.  0 on absent rows, on a pair with an empty side, and on all of direction 2 when
// !both (single-sided losses).  d1 / d2 are the SQUARED distances of the counted forward.
namespace {
__global__ void chamfer_counts_mean_grad_kernel(const float *__restrict__ go, float scale, float inv_b,
                                                const float *__restrict__ d1, const float *__restrict__ d2,
                                                const int *__restrict__ cnt1, const int *__restrict__ cnt2, int N,
                                                int M, long long n1, long long n2, int root, int both,
                                                float *__restrict__ gd1, float *__restrict__ gd2) {
  const float t = go[0] * scale * inv_b;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += stride) {
    const bool dir = i >= n1;
    const long long e = dir ? i - n1 : i;
    const int NAp = dir ? M : N;
    const int b = (int)(e / NAp), k = (int)(e - (long long)b * NAp);
    const int c1 = cloud_count<true>(cnt1, b, N), c2 = cloud_count<true>(cnt2, b, M);
    const int ca = dir ? c2 : c1;
    float v = 0.f;
    if (k < ca && c1 > 0 && c2 > 0 && (!dir || both)) {
      v = t * (1.0f / (float)ca);
      if (root) v = v / (2.f * sqrtf((dir ? d2 : d1)[e]));
    }
    (dir ? gd2 : gd1)[e] = v;
  }
}
}  // namespace

extern "C" int pcops_chamfer_counts_mean_grad(const float *grad_out, float scale, const float *dist1,
                                              const float *dist2, const int *counts1, const int *counts2, int B,
                                              int N, int M, int root, int both, float *gd1, float *gd2,
                                              pcops_stream_t stream) {
  if (B < 0 || N < 0 || M < 0) return PCOPS_ERR_INVALID;
  const long long n1 = (long long)B * N, n2 = (long long)B * M;
  if (n1 + n2 == 0) return PCOPS_OK;
  if (!counts1 && !counts2) return PCOPS_ERR_INVALID;
  if (!grad_out || (n1 && (!dist1 || !gd1)) || (n2 && (!gd2 || (both && !dist2)))) return PCOPS_ERR_INVALID;
  long long blocks = (n1 + n2 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(chamfer_counts_mean_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     grad_out, scale, 1.0f / (float)B, dist1, dist2, counts1, counts2, N, M, n1, n2, root, both, gd1,
                     gd2);
  PC_CHECK_LAUNCH();
  return PCOPS_OK;
}
