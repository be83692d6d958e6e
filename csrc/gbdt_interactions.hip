// SHAP interaction values for the histogram GBDT (gfx950): HistGBDT.predict_interactions, the
// pair-term companion of csrc/gbdt_shap.hip's contribution kernel.
//
// ---- formula
// Notation as in gbdt_shap.hip: a path of class k has a leaf value v and m <= 10 merged elements
// (feature f_l, zero fraction z_l, o_l in {0, 1} the interval test on the row; NaN fails every
// left and passes every right condition).  out is fp32 [N, K, F + 1, F + 1]:
//   i != j, both < F:  out[n, k, i, j] = sum over the paths that hold both features of
//       0.5 * v * (o_i - z_i) * (o_j - z_j) * W_ij,
//       W_ij = int_0^1 prod_{l != i, j} (o_l t + z_l (1 - t)) dt
//     (the Shapley interaction index; s! (m-2-s)! / (m-1)! is the Beta integral of
//     t^s (1-t)^(m-2-s); W_ij = 1 for m = 2; a path with m = 1 has no such term);
//   diagonal:  out[n, k, i, i] = phi_i - sum_{j != i} out[n, k, i, j], phi_i the contribution,
//     per path v * (o_i - z_i) * W_i with W_i = int_0^1 prod_{l != i} (...) dt;
//   bias:  out[n, k, F, F] = bias[k] (summed on the host in fp64), the rest of row and column F
//     is 0.
// Every integrand has degree <= m - 1: the Gauss-Legendre rule with Q = ceil(m / 2) nodes that
// gbdt_path.h carries is exact for W_i and W_ij.  No division, nothing special at z = 0.
//
// ---- table (kubedl_amd/models/gbdt.py, _pair_table)
// Per class k and per feature i that a path of the class splits on, the host lists the paths
// that hold i, in the path table's order, with element i ROTATED TO SLOT 0 and the others
// behind it in their order.  The 16-byte slot format is gbdt_shap.hip's, unchanged:
//   header { v bits, m, 0, 0 }, m elements { feature | has_left << 30, lo, hi, z bits },
//   ceil(m / 4) slots of (1 - z) bits (rounded from fp64), four per slot, in the rotated order.
// A path of m elements appears m times, so the table holds about sum m^2 slots where the
// contribution table holds sum m.  Each (class, feature) list is cut into chunks of at most
// kChunkSlots slots of WHOLE paths (chunk_off); list (k, i) owns chunks
// [feat_chunk[k * F + i], feat_chunk[k * F + i + 1]) -- an empty range for a feature no path
// of the class uses.
//
// ---- work split
// grid = (row tiles, F + 1, K): a block owns R rows, one class k and one conditioning feature i,
// i.e. the R x (F + 1) tile out[row0 .. row0 + R, k, i, :].  A lane owns one row and that row's
// F + 1 accumulators (row i of the row's matrix).  The block streams list (k, i)'s chunks
// through LDS; all lanes work on the same path (broadcast LDS reads), m is block-uniform and
// selects a fully unrolled body (pair_term<M>) whose per-element arrays have static indices
// and live in registers; the Gauss-Legendre constants are compile-time indices.  With element 0
// (feature i) fixed, per node q the product of the factors of elements 1 .. m-1 is W_i's
// integrand, and prefix and suffix products over those same m - 1 factors give W_ij's for every
// j: O(m Q) per path, as in the contribution kernel, but a row now walks sum m paths per class
// where that kernel walks the paths once.  The path adds 0.5 v d_i d_j W_ij to accumulator f_j
// and v d_i W_i - sum_j (those terms) to accumulator i.  No atomics: a row's terms are added
// in table order, so two calls are bit-equal.  The tile is then written cooperatively, F + 1
// contiguous floats per row (column F as 0); the row pitch of out is K (F + 1)^2 floats, and
// every output offset is 64-bit.
// A block whose list is empty (a feature no path uses, or row F) writes its tile -- zeros, and
// bias[k] at [F, F] -- without staging rows or walking anything: the same launch.
//
// ---- LDS (160 KiB per CU) of a block of R rows: the contribution kernel's budget
//   path chunk   kChunkSlots * 16 B = 8 KiB
//   row tile     R * (F | 1) * 4 B          (lane-private rows, odd stride: conflict-free)
//   accumulators R * ((F + 1) | 1) * 4 B    (lane-private rows, odd stride, row-major)
// R is the one of 256 / 128 / 64 with the most waves per CU by that budget (gbdt_path.h,
// pick_rows), so F = 28 gives 256 rows (67 KiB), F = 100: 128, F = 200: 64.  From F = 304 on 64
// rows no longer fit and the no-staging variant runs (kept rather than refused, as in the
// contribution kernel): rows are read from global memory and a lane's accumulators are its
// output row out[n, k, i, :] itself.  F + 1 is a grid dimension: F >= 65535 is refused.
// All of this is derived from the budget, not measured; no occupancy figure and no split between
// VALU and LDS time has been measured.  Measured (profiles/gbdt_interactions_bench.txt): 2M x 28
// rows, 100 depth-6 trees (6,304 paths, a 2,177 KiB per-feature table) in eight row blocks:
// 265 ms, 3.7x the contribution kernel on the same model.
#include "common.h"
#include "gbdt_path.h"
#include "kdl_api.h"

namespace kdl {
namespace {

using namespace gbdt_path;

// One row's terms of one path of exactly M elements whose element 0 is the conditioning
// feature.  ``p``: the path's slots in the LDS chunk (the same address in every lane);
// ``x``: the row; ``acc``: its F + 1 accumulators (row f[0] of the row's matrix).
template <int M, int Q = (M + 1) / 2>
__device__ __forceinline__ void pair_term(const int4* __restrict__ p, const float* __restrict__ x, int F,
                                          float* __restrict__ acc) {
  const float v = __int_as_float(p[0].x);
  int f[M];
  float z[M], d[M], step[M], W[M];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    f[j] = elem_feature(p[1 + j]);
    ok = ok && f[j] < F;
  }
  if (!ok) return;  // block-uniform: a broken table adds nothing
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int4 e = p[1 + j];
    const float omz = elem_one_minus_z(p[1 + M + j / 4], j);
    const bool o = elem_inside(e, x[f[j]]);
    z[j] = __int_as_float(e.w);
    d[j] = o ? omz : -z[j];  // o - z
    step[j] = o ? 1.f : 0.f;
    W[j] = 0.f;
  }
  // W[0] = W_i (all of elements 1 .. M-1), W[j] = W_ij (elements 1 .. M-1 without j)
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const float t = kGlT[Q - 1][q], u = kGlU[Q - 1][q];
    float fac[M], pre[M];
#pragma unroll
    for (int j = 1; j < M; ++j) fac[j] = fmaf(z[j], u, step[j] * t);  // o t + z (1 - t)
    float suf = kGlW[Q - 1][q];
    if constexpr (M > 1) {
      pre[1] = 1.f;
#pragma unroll
      for (int j = 2; j < M; ++j) pre[j] = pre[j - 1] * fac[j - 1];
#pragma unroll
      for (int j = M - 1; j >= 1; --j) {
        W[j] = fmaf(pre[j], suf, W[j]);
        suf *= fac[j];
      }
    }
    W[0] += suf;
  }
  const float vd = v * d[0];
  const float hvd = 0.5f * vd;  // exact
  float diag = vd * W[0];
#pragma unroll
  for (int j = 1; j < M; ++j) {
    const float off = hvd * d[j] * W[j];
    acc[f[j]] += off;
    diag -= off;
  }
  acc[f[0]] += diag;
}

template <int R, bool STAGE>
__global__ __launch_bounds__(R) void forest_interactions_kernel(const float* __restrict__ X, int64_t N, int F,
                                                                int stride, int astride,
                                                                const int4* __restrict__ paths, int num_slots,
                                                                const int32_t* __restrict__ chunk_off,
                                                                int num_chunks,
                                                                const int32_t* __restrict__ feat_chunk,
                                                                const float* __restrict__ bias, int K,
                                                                float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int4* chunk = reinterpret_cast<int4*>(lds_raw);                              // [kChunkSlots]
  float* xs = reinterpret_cast<float*>(lds_raw + kChunkSlots * sizeof(int4));  // [R][stride] (STAGE)
  float* accs = xs + R * stride;                                               // [R][astride] (STAGE)
  const int tid = threadIdx.x;
  const int fi = blockIdx.y;  // the conditioning feature, F: the bias row
  const int k = blockIdx.z;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * R;
  const int cnt = (N - row0) < R ? static_cast<int>(N - row0) : R;  // >= 1: grid.x is ceil(N / R)
  const bool active = tid < cnt;
  const int F1 = F + 1;
  const int64_t pitch = static_cast<int64_t>(K) * F1 * F1;              // floats per row of X
  float* tile = out + row0 * pitch + (static_cast<int64_t>(k) * F1 + fi) * F1;  // out[row0, k, fi, 0]
  int c0 = 0, c1 = 0;
  if (fi < F) {
    c0 = feat_chunk[k * F + fi];
    c1 = feat_chunk[k * F + fi + 1];
    if (c0 < 0) c0 = 0;
    if (c1 > num_chunks) c1 = num_chunks;
  }
  if (c0 >= c1) {  // block-uniform: no path of the class holds the feature, or the bias row
    const float corner = fi == F ? bias[k] : 0.f;
    const int total = cnt * F1;
    for (int i = tid; i < total; i += R) {
      const int r = i / F1;
      const int j = i - r * F1;
      tile[r * pitch + j] = j == F ? corner : 0.f;
    }
    return;
  }
  const float* x;
  float* acc;
  if constexpr (STAGE) {
    stage_rows<R>(X + row0 * F, cnt, F, stride, xs);
    x = xs + tid * stride;
    acc = accs + tid * astride;
    for (int i = 0; i < F; ++i) acc[i] = 0.f;
  } else {
    x = X + (row0 + (active ? tid : 0)) * F;
    acc = tile + (active ? tid : 0) * pitch;  // the output row itself
    if (active) {
      for (int i = 0; i < F1; ++i) acc[i] = 0.f;
    }
  }
  for (int c = c0; c < c1; ++c) {  // block-uniform
    const int base = chunk_off[c];
    const int n = chunk_off[c + 1] - base;
    if (base < 0 || n <= 0 || n > kChunkSlots || n > num_slots - base) continue;
    __syncthreads();  // the previous chunk's paths are done (first chunk: the row tile is staged)
    for (int i = tid; i < n; i += R) chunk[i] = paths[base + i];
    __syncthreads();
    int p = 0;
    while (p < n) {
      const int m = chunk[p].y;
      const int len = 1 + m + (m + 3) / 4;
      if (m < 1 || m > kMaxPath || len > n - p) break;  // a broken chunk ends here
      if (active) {
        const int4* q = chunk + p;
        switch (m) {
          case 1: pair_term<1>(q, x, F, acc); break;
          case 2: pair_term<2>(q, x, F, acc); break;
          case 3: pair_term<3>(q, x, F, acc); break;
          case 4: pair_term<4>(q, x, F, acc); break;
          case 5: pair_term<5>(q, x, F, acc); break;
          case 6: pair_term<6>(q, x, F, acc); break;
          case 7: pair_term<7>(q, x, F, acc); break;
          case 8: pair_term<8>(q, x, F, acc); break;
          case 9: pair_term<9>(q, x, F, acc); break;
          default: pair_term<10>(q, x, F, acc); break;
        }
      }
      p += len;
    }
  }
  if constexpr (STAGE) {
    __syncthreads();  // every lane's accumulators are final
    const int total = cnt * F1;
    for (int i = tid; i < total; i += R) {
      const int r = i / F1;
      const int j = i - r * F1;
      tile[r * pitch + j] = j < F ? accs[r * astride + j] : 0.f;
    }
  }
}

size_t interactions_lds(int R, bool stage, int stride, int astride) {
  return static_cast<size_t>(kChunkSlots) * sizeof(int4) +
         (stage ? static_cast<size_t>(R) * (stride + astride) * sizeof(float) : 0);
}

template <int R, bool STAGE>
hipError_t launch_interactions(const float* X, int64_t N, int F, int stride, int astride, const int32_t* paths,
                               int num_slots, const int32_t* chunk_off, int num_chunks, const int32_t* feat_chunk,
                               const float* bias, int K, float* out, size_t lds, hipStream_t s) {
  static bool attr_set = false;  // > 64 KiB of dynamic LDS must be opted into once
  if (!attr_set) {
    RETURN_IF_HIP_ERR(hipFuncSetAttribute(reinterpret_cast<const void*>(forest_interactions_kernel<R, STAGE>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    attr_set = true;
  }
  const int64_t blocks = (N + R - 1) / R;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((forest_interactions_kernel<R, STAGE>),
                     dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(F + 1), static_cast<unsigned>(K)),
                     dim3(R), lds, s, X, N, F, stride, astride, reinterpret_cast<const int4*>(paths), num_slots,
                     chunk_off, num_chunks, feat_chunk, bias, K, out);
  return hipGetLastError();
}

}  // namespace

int gbdt_interactions_chunk_slots() { return kChunkSlots; }

int gbdt_interactions_rows_per_block(int F) {
  return pick_rows(interactions_lds(0, false, 0, 0), static_cast<size_t>((F | 1) + ((F + 1) | 1)) * sizeof(float));
}

hipError_t gbdt_interactions(const float* X, int64_t N, int F, const int32_t* paths, int num_slots,
                             const int32_t* chunk_off, int num_chunks, const int32_t* feat_chunk, const float* bias,
                             int K, float* out, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  if (F < 1 || F >= 65535 || K < 1 || K > 32 || num_slots < 0 || num_chunks < 0) return hipErrorInvalidValue;
  const int stride = F | 1, astride = (F + 1) | 1;
  const int R = gbdt_interactions_rows_per_block(F);
  const size_t lds = interactions_lds(R, R != 0, stride, astride);
#define INTERACTIONS_ARGS \
  X, N, F, stride, astride, paths, num_slots, chunk_off, num_chunks, feat_chunk, bias, K, out, lds, s
  switch (R) {
    case 256: return launch_interactions<256, true>(INTERACTIONS_ARGS);
    case 128: return launch_interactions<128, true>(INTERACTIONS_ARGS);
    case 64: return launch_interactions<64, true>(INTERACTIONS_ARGS);
    default: return launch_interactions<256, false>(INTERACTIONS_ARGS);
  }
#undef INTERACTIONS_ARGS
}

}  // namespace kdl
