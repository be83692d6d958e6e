// Interventional (marginal) TreeSHAP for the histogram GBDT (gfx950):
// HistGBDT.set_background(X, interventional=True) and
// HistGBDT.predict_contribs(X, perturbation="interventional").
//
// Notation of csrc/gbdt_shap.hip: a path of class k has a leaf value v and m <= 10 merged
// elements, element l a feature f_l and an interval test o_l(row) in {0, 1} (NaN fails every
// left and passes every right condition).  full = 2^m - 1 and mask(row) has bit l = o_l(row).
// For a row x and a background row z the hybrid row h(S) takes the features in S from x and
// the others from z; the path's game S -> v [h(S) reaches the leaf] is a conjunction, so with
// mx = mask(x), mz = mask(z):
//   (mx | mz) != full: the path adds nothing;
//   otherwise D = mx & ~mz, a = popcount(D), E = mz & ~mx, b = popcount(E):
//     every element of D gets +v (a-1)! b! / (a+b)!, every element of E gets -v a! (b-1)! / (a+b)!
//     (elements with both bits set are dummies),
// and phi[n, k, f_l] is the mean over the background rows of the sum over class k's paths.
//
// The design point: for a fixed path and x, a background row matters only through mz.  The
// background is reduced once to hist[path][mask], the number of background rows with that mask
// (2^m counters per path, each path's counters sum to B), and the explain kernel walks, per
// path, the DISTINCT masks with their weight w = count / B.  Its cost per row is the sum over
// paths of the path's number of distinct masks, independent of B.
//
// ---- kernel A: mask histogram (path_masks_kernel)
// Mask table (int32 [slots, 4], 16-byte slots): per path a header { v bits, m, first counter, 0 }
// and m elements { feature | has_left << 30, lo bits, hi bits, 0 }.  A path's 2^m counters start
// at its ``first counter`` in the dense histogram; paths are laid out in table order, so the
// counters of a run of paths are contiguous.  The host cuts the table into chunks of whole paths
// such that a chunk has at most kMaskChunkSlots slots AND at most kMaskChunkCounters counters
// (chunk_off, cnt_off; one m = 10 path alone needs 1,024 counters).  One lane per background
// row, the row tile in LDS at stride F | 1 (the cover kernel's), the chunk's slots (8 KiB) and
// its int32 counters (16 KiB) beside it.  A lane forms mask(z) with m interval tests and counts
// it with one LDS atomic; the chunk's non-zero counters are flushed once with 64-bit integer
// global atomics.  Integer sums: order independent and bit-reproducible; several ranks merge
// the dense histogram with an integer all-reduce.
//
// ---- kernel B: explain (forest_contribs_iv_kernel)
// Explain table (int32 [slots, 4]): per path
//   header     { v bits, m, r, full }
//   m elements { feature | has_left << 30, lo bits, hi bits, 0 }
//   ceil(r / 2) record slots { mask, w bits, mask, w bits }: the r masks with a count > 0 and
//              w = count / B rounded once from fp64
// class-major, cut into chunks of at most kChunkSlots slots holding whole paths (chunk_off,
// class_chunk, as in gbdt_shap.hip).  A path with more records than a chunk holds is stored as
// several table paths with the same elements: the sum is linear in the records.  Paths with
// m = 0 only feed the bias column, which the host sums in fp64.
//
// Work split and LDS are forest_contribs_kernel's: one lane owns a row for one class, F + 1
// lane-private LDS accumulators at an odd stride beside the lane's row, blocks of 256 / 128 / 64
// rows by LDS budget and a no-staging variant for large F.  All lanes of a block work on the
// same path: m is block-uniform and selects a fully unrolled body (path_iv<M>).  The lane forms
// mx with M interval tests, then walks the path's records by LDS broadcast reads.  For a record
// with (mx | mask) == full it takes sp = w * kWp[a][b] and sn = w * kWn[a][b] from two 11 x 11
// tables in constant memory (exact factorial ratios, rounded once from fp64) and adds +sp / -sn
// into M register accumulators by bit tests on D and E.  After the last record: one LDS add of
// v * acc_l per element.  No division, no atomics, terms are added in table order: the result
// is bit-reproducible.  Not measured here: the split between the record walk's VALU work and
// the (lane-divergent) constant-table reads.
#include "common.h"
#include "gbdt_path.h"
#include "kdl_api.h"

namespace kdl {
namespace {

using namespace gbdt_path;

constexpr int kMaskChunkSlots = 512;      // kernel A: 16-byte mask-table slots per LDS chunk
constexpr int kMaskChunkCounters = 4096;  // kernel A: int32 counters per LDS chunk (>= 2^kMaxPath)
static_assert(kMaskChunkCounters >= (1 << kMaxPath), "a single path of kMaxPath elements must fit");

// Shapley weights of a conjunction game, [a][b] with a + b <= kMaxPath (0 elsewhere):
// wp = (a-1)! b! / (a+b)! for an element of D (a >= 1), wn = a! (b-1)! / (a+b)! for one of E
// (b >= 1).  The factorials are exact in fp64; each ratio is rounded once to fp32.
struct IvWeights {
  float wp[kMaxPath + 1][kMaxPath + 1];
  float wn[kMaxPath + 1][kMaxPath + 1];
};

constexpr IvWeights make_iv_weights() {
  IvWeights t{};
  double fact[kMaxPath + 1] = {1.0};
  for (int i = 1; i <= kMaxPath; ++i) fact[i] = fact[i - 1] * i;
  for (int a = 0; a <= kMaxPath; ++a) {
    for (int b = 0; a + b <= kMaxPath; ++b) {
      if (a >= 1) t.wp[a][b] = static_cast<float>(fact[a - 1] * fact[b] / fact[a + b]);
      if (b >= 1) t.wn[a][b] = static_cast<float>(fact[a] * fact[b - 1] / fact[a + b]);
    }
  }
  return t;
}

__constant__ IvWeights kIvW = make_iv_weights();

// ------------------------------------------------------------------ kernel A: mask histogram
template <int R, bool STAGE>
__global__ __launch_bounds__(R) void path_masks_kernel(const float* __restrict__ X, int64_t N, int F, int stride,
                                                       const int4* __restrict__ table, int num_slots,
                                                       const int32_t* __restrict__ chunk_off,
                                                       const int32_t* __restrict__ cnt_off, int num_chunks,
                                                       int64_t num_counters,
                                                       unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int4* chunk = reinterpret_cast<int4*>(lds_raw);                                      // [kMaskChunkSlots]
  int* cnt_lds = reinterpret_cast<int*>(lds_raw + kMaskChunkSlots * sizeof(int4));     // [kMaskChunkCounters]
  float* xs = reinterpret_cast<float*>(cnt_lds + kMaskChunkCounters);                  // [R][stride] (STAGE)
  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * R;
  const int cnt = (N - row0) < R ? static_cast<int>(N - row0) : R;  // >= 1: the grid is ceil(N / R)
  const bool active = tid < cnt;
  const float* x;
  if constexpr (STAGE) {
    stage_rows<R>(X + row0 * F, cnt, F, stride, xs);
    x = xs + tid * stride;
  } else {
    x = X + (row0 + (active ? tid : 0)) * F;
  }
  for (int c = 0; c < num_chunks; ++c) {  // block-uniform
    const int base = chunk_off[c];
    const int n = chunk_off[c + 1] - base;
    const int64_t cbase = cnt_off[c];
    const int nc = cnt_off[c + 1] - cnt_off[c];
    if (base < 0 || n <= 0 || n > kMaskChunkSlots || n > num_slots - base) continue;
    if (cbase < 0 || nc <= 0 || nc > kMaskChunkCounters || nc > num_counters - cbase) continue;
    __syncthreads();  // the previous chunk's flush is done (first chunk: the row tile is staged)
    for (int i = tid; i < n; i += R) chunk[i] = table[base + i];
    for (int i = tid; i < nc; i += R) cnt_lds[i] = 0;
    __syncthreads();
    int p = 0;
    while (p < n) {
      const int4 h = chunk[p];
      const int m = h.y;
      const int64_t first = static_cast<int64_t>(h.z) - cbase;  // the path's first counter in the chunk
      // a broken chunk ends here: nothing is counted outside the chunk's counters
      if (m < 1 || m > kMaxPath || 1 + m > n - p || first < 0 || first + (1 << m) > nc) break;
      bool ok = true;
      for (int j = 0; j < m; ++j) ok = ok && elem_feature(chunk[p + 1 + j]) < F;
      if (ok && active) {
        int mask = 0;
        for (int j = 0; j < m; ++j) {
          const int4 e = chunk[p + 1 + j];
          mask |= static_cast<int>(elem_inside(e, x[elem_feature(e)])) << j;
        }
        atomicAdd(cnt_lds + static_cast<int>(first) + mask, 1);
      }
      p += 1 + m;
    }
    __syncthreads();
    for (int i = tid; i < nc; i += R) {
      const int v = cnt_lds[i];
      if (v) atomicAdd(hist + cbase + i, static_cast<unsigned long long>(v));
    }
  }
}

// ------------------------------------------------------------------ kernel B: explain
// One row's terms of one table path of exactly M elements and ``r`` records.  ``p``: the path's
// slots in the LDS chunk (the same address in every lane: broadcast reads); ``x``: the row;
// ``acc``: its accumulators.
template <int M>
__device__ __forceinline__ void path_iv(const int4* __restrict__ p, int r, const float* __restrict__ x, int F,
                                        float* __restrict__ acc) {
  constexpr int full = (1 << M) - 1;
  int f[M];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    f[j] = elem_feature(p[1 + j]);
    ok = ok && f[j] < F;
  }
  if (!ok) return;  // block-uniform: a broken table adds nothing
  int mx = 0;
#pragma unroll
  for (int j = 0; j < M; ++j) mx |= static_cast<int>(elem_inside(p[1 + j], x[f[j]])) << j;
  float s[M];
#pragma unroll
  for (int j = 0; j < M; ++j) s[j] = 0.f;
  const int4* rec = p + 1 + M;
  auto add = [&](int mask, float w) {
    mask &= full;
    if ((mx | mask) != full) return;
    const int D = mx & ~mask, E = mask & ~mx;
    const int a = __popc(D), b = __popc(E);  // a + b <= M
    const float sp = w * kIvW.wp[a][b];
    const float sn = w * kIvW.wn[a][b];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      if ((D >> j) & 1) s[j] += sp;
      if ((E >> j) & 1) s[j] -= sn;
    }
  };
  for (int i = 0; i < r; i += 2) {
    const int4 q = rec[i >> 1];
    add(q.x, __int_as_float(q.y));
    if (i + 1 < r) add(q.z, __int_as_float(q.w));
  }
  const float v = __int_as_float(p[0].x);
#pragma unroll
  for (int j = 0; j < M; ++j) acc[f[j]] += v * s[j];
}

template <int R, bool STAGE>
__global__ __launch_bounds__(R) void forest_contribs_iv_kernel(const float* __restrict__ X, int64_t N, int F,
                                                               int stride, int astride,
                                                               const int4* __restrict__ table, int num_slots,
                                                               const int32_t* __restrict__ chunk_off,
                                                               int num_chunks,
                                                               const int32_t* __restrict__ class_chunk,
                                                               const float* __restrict__ bias, int K,
                                                               float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int4* chunk = reinterpret_cast<int4*>(lds_raw);                              // [kChunkSlots]
  float* xs = reinterpret_cast<float*>(lds_raw + kChunkSlots * sizeof(int4));  // [R][stride] (STAGE)
  float* accs = xs + R * stride;                                               // [R][astride] (STAGE)
  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * R;
  const int cnt = (N - row0) < R ? static_cast<int>(N - row0) : R;  // >= 1: the grid is ceil(N / R)
  const bool active = tid < cnt;
  const int F1 = F + 1;
  const float* x;
  if constexpr (STAGE) {
    stage_rows<R>(X + row0 * F, cnt, F, stride, xs);
    x = xs + tid * stride;
  } else {
    x = X + (row0 + (active ? tid : 0)) * F;
  }
  for (int k = 0; k < K; ++k) {
    float* acc;
    if constexpr (STAGE) {
      acc = accs + tid * astride;
    } else {
      acc = out + ((row0 + (active ? tid : 0)) * K + k) * F1;  // the output row itself (64-bit offset)
    }
    if (STAGE || active) {
      for (int i = 0; i < F; ++i) acc[i] = 0.f;
    }
    int c0 = class_chunk[k], c1 = class_chunk[k + 1];
    if (c0 < 0) c0 = 0;
    if (c1 > num_chunks) c1 = num_chunks;
    for (int c = c0; c < c1; ++c) {  // block-uniform
      const int base = chunk_off[c];
      const int n = chunk_off[c + 1] - base;
      if (base < 0 || n <= 0 || n > kChunkSlots || n > num_slots - base) continue;
      __syncthreads();  // the previous chunk's paths are done (first chunk: the row tile is staged)
      for (int i = tid; i < n; i += R) chunk[i] = table[base + i];
      __syncthreads();
      int p = 0;
      while (p < n) {
        const int m = chunk[p].y;
        const int r = chunk[p].z;
        if (m < 1 || m > kMaxPath || r < 0 || r > 2 * kChunkSlots) break;  // a broken chunk ends here
        const int len = 1 + m + (r + 1) / 2;
        if (len > n - p) break;
        if (active) {
          const int4* q = chunk + p;
          switch (m) {
            case 1: path_iv<1>(q, r, x, F, acc); break;
            case 2: path_iv<2>(q, r, x, F, acc); break;
            case 3: path_iv<3>(q, r, x, F, acc); break;
            case 4: path_iv<4>(q, r, x, F, acc); break;
            case 5: path_iv<5>(q, r, x, F, acc); break;
            case 6: path_iv<6>(q, r, x, F, acc); break;
            case 7: path_iv<7>(q, r, x, F, acc); break;
            case 8: path_iv<8>(q, r, x, F, acc); break;
            case 9: path_iv<9>(q, r, x, F, acc); break;
            default: path_iv<10>(q, r, x, F, acc); break;
          }
        }
        p += len;
      }
    }
    const float b = bias[k];  // written without walking anything
    if constexpr (STAGE) {
      __syncthreads();  // every lane's accumulators are final
      // the tile's cnt rows of class k, F1 contiguous floats each
      const int total = cnt * F1;
      for (int i = tid; i < total; i += R) {
        const int r = i / F1;
        const int fi = i - r * F1;
        out[((row0 + r) * K + k) * F1 + fi] = fi < F ? accs[r * astride + fi] : b;
      }
      __syncthreads();  // before the next class clears them
    } else {
      if (active) acc[F] = b;
    }
  }
}

size_t masks_lds(int R, bool stage, int stride) {
  return static_cast<size_t>(kMaskChunkSlots) * sizeof(int4) + static_cast<size_t>(kMaskChunkCounters) * sizeof(int) +
         (stage ? static_cast<size_t>(R) * stride * sizeof(float) : 0);
}

size_t contribs_iv_lds(int R, bool stage, int stride, int astride) {
  return static_cast<size_t>(kChunkSlots) * sizeof(int4) +
         (stage ? static_cast<size_t>(R) * (stride + astride) * sizeof(float) : 0);
}

template <int R, bool STAGE>
hipError_t launch_masks(const float* X, int64_t N, int F, int stride, const int32_t* table, int num_slots,
                        const int32_t* chunk_off, const int32_t* cnt_off, int num_chunks, int64_t num_counters,
                        int64_t* hist, size_t lds, hipStream_t s) {
  static bool attr_set = false;  // > 64 KiB of dynamic LDS must be opted into once
  if (!attr_set) {
    RETURN_IF_HIP_ERR(hipFuncSetAttribute(reinterpret_cast<const void*>(path_masks_kernel<R, STAGE>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    attr_set = true;
  }
  const int64_t blocks = (N + R - 1) / R;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((path_masks_kernel<R, STAGE>), dim3(static_cast<unsigned>(blocks)), dim3(R), lds, s, X, N, F,
                     stride, reinterpret_cast<const int4*>(table), num_slots, chunk_off, cnt_off, num_chunks,
                     num_counters, reinterpret_cast<unsigned long long*>(hist));
  return hipGetLastError();
}

template <int R, bool STAGE>
hipError_t launch_contribs_iv(const float* X, int64_t N, int F, int stride, int astride, const int32_t* table,
                              int num_slots, const int32_t* chunk_off, int num_chunks, const int32_t* class_chunk,
                              const float* bias, int K, float* out, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    RETURN_IF_HIP_ERR(hipFuncSetAttribute(reinterpret_cast<const void*>(forest_contribs_iv_kernel<R, STAGE>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    attr_set = true;
  }
  const int64_t blocks = (N + R - 1) / R;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((forest_contribs_iv_kernel<R, STAGE>), dim3(static_cast<unsigned>(blocks)), dim3(R), lds, s, X,
                     N, F, stride, astride, reinterpret_cast<const int4*>(table), num_slots, chunk_off, num_chunks,
                     class_chunk, bias, K, out);
  return hipGetLastError();
}

}  // namespace

int gbdt_path_masks_chunk_slots() { return kMaskChunkSlots; }
int gbdt_path_masks_chunk_counters() { return kMaskChunkCounters; }
int gbdt_path_masks_rows_per_block(int F) {
  return pick_rows(masks_lds(0, false, 0), static_cast<size_t>(F | 1) * sizeof(float));
}
int gbdt_contribs_iv_chunk_slots() { return kChunkSlots; }
int gbdt_contribs_iv_rows_per_block(int F) {
  return pick_rows(contribs_iv_lds(0, false, 0, 0), static_cast<size_t>((F | 1) + ((F + 1) | 1)) * sizeof(float));
}

hipError_t gbdt_path_masks(const float* X, int64_t N, int F, const int32_t* table, int num_slots,
                           const int32_t* chunk_off, const int32_t* cnt_off, int num_chunks, int64_t num_counters,
                           int64_t* hist, hipStream_t s) {
  if (N <= 0 || num_chunks <= 0) return hipSuccess;
  if (F < 1 || F > (1 << 20) || num_slots < 0 || num_counters < 0) return hipErrorInvalidValue;  // cnt * F stays an int
  const int stride = F | 1;
  const int R = gbdt_path_masks_rows_per_block(F);
  const size_t lds = masks_lds(R, R != 0, stride);
#define MASKS_ARGS X, N, F, stride, table, num_slots, chunk_off, cnt_off, num_chunks, num_counters, hist, lds, s
  switch (R) {
    case 256: return launch_masks<256, true>(MASKS_ARGS);
    case 128: return launch_masks<128, true>(MASKS_ARGS);
    case 64: return launch_masks<64, true>(MASKS_ARGS);
    default: return launch_masks<256, false>(MASKS_ARGS);
  }
#undef MASKS_ARGS
}

hipError_t gbdt_contribs_iv(const float* X, int64_t N, int F, const int32_t* table, int num_slots,
                            const int32_t* chunk_off, int num_chunks, const int32_t* class_chunk, const float* bias,
                            int K, float* out, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  if (F < 1 || F >= (1 << 20) || K < 1 || K > 32 || num_slots < 0 || num_chunks < 0) return hipErrorInvalidValue;
  const int stride = F | 1, astride = (F + 1) | 1;
  const int R = gbdt_contribs_iv_rows_per_block(F);
  const size_t lds = contribs_iv_lds(R, R != 0, stride, astride);
#define CONTRIBS_IV_ARGS \
  X, N, F, stride, astride, table, num_slots, chunk_off, num_chunks, class_chunk, bias, K, out, lds, s
  switch (R) {
    case 256: return launch_contribs_iv<256, true>(CONTRIBS_IV_ARGS);
    case 128: return launch_contribs_iv<128, true>(CONTRIBS_IV_ARGS);
    case 64: return launch_contribs_iv<64, true>(CONTRIBS_IV_ARGS);
    default: return launch_contribs_iv<256, false>(CONTRIBS_IV_ARGS);
  }
#undef CONTRIBS_IV_ARGS
}

}  // namespace kdl
