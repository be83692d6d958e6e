// Feature contributions for the histogram GBDT (gfx950): HistGBDT.set_background (the cover
// pass) and HistGBDT.predict_contribs (exact path-dependent TreeSHAP).
//
// ---- cover pass (forest_cover_kernel)
// counts[node] += the number of rows of X that reach the node, for every node of trees
// [t0, t1), under predict's routing rule (``x[feature] <= threshold ? left : left + 1``).
// The shape is the predict kernel's: one lane per row, the row tile in LDS at stride F | 1,
// whole trees streamed through an 8 KiB LDS chunk (kChunkNodes GbdtNodes).  Beside the chunk
// sits an int32 counter per chunk node (2 KiB): a lane counts every node it steps onto with an
// LDS atomic, the root is counted once per block (every row of the block passes it), and the
// chunk's counters are flushed once with 64-bit integer global atomics.  A tree larger than
// the chunk is walked in global memory and counted there directly.  The walk makes the same
// ``parent < child < tree size`` and ``feature < F`` checks as predict's: a broken table
// cannot send a lane out of bounds.  Integer sums: order independent and bit-reproducible.
//
// ---- contributions (forest_contribs_kernel)
// The host decomposes every tree into its root-to-leaf paths (kubedl_amd/models/gbdt.py,
// _path_table).  A path is a leaf value v and m <= 10 merged elements, one per distinct
// feature on it: the feature, the interval the row must satisfy (``!(x <= lo)`` for the
// largest right-turn threshold, ``x <= hi`` for the smallest left-turn threshold; lo = NaN
// means "no right turn", a flag bit means "has a left turn", so NaN fails every left and
// passes every right condition) and the zero fraction z = prod cover[child] / cover[parent]
// over that feature's splits.  With o_j in {0, 1} the interval test on the row, the path adds
//     phi[f_i] += v * (o_i - z_i) * W_i,   W_i = int_0^1 prod_{j != i} (o_j t + z_j (1 - t)) dt
// (the Shapley weight k! (m-1-k)! / m! is the Beta integral of t^k (1-t)^(m-1-k)).  The
// integrand has degree m - 1, so a Gauss-Legendre rule with Q = ceil(m / 2) nodes on [0, 1] is
// exact; the products without factor i come from prefix and suffix products (O(m Q) per path,
// no division, nothing special at z = 0).  ``1 - z`` is carried beside z, rounded from fp64:
// formed in fp32 it would lose all its digits where z is close to 1.
//
// Path table (int32 [slots, 4], 16-byte slots, copied with int4 moves):
//   header   { v bits, m, 0, 0 }
//   m elements { feature | has_left << 30, lo bits, hi bits, z bits }
//   ceil(m / 4) slots of (1 - z) bits, four per slot
// Paths of one class are contiguous (class-major, then tree, then leaf order) and cut into
// chunks of at most kChunkSlots slots holding WHOLE paths (chunk_off); class k owns chunks
// [class_chunk[k], class_chunk[k + 1]).  A chunk never has to hold a whole tree, so a
// depth-10 tree needs no global-memory path.  Paths with m = 0 (single-leaf trees) are not in
// the table: they only feed the bias column, out[n, k, F] = bias[k], which does not depend on
// the row and is summed on the host in fp64.
//
// Work split: one lane owns one row for the whole forest of one class; the classes are the
// outermost loop, so a block holds (F + 1) accumulators per row, not K (F + 1).  No atomics;
// a row's terms are added in table order, so the output is reproducible run to run.  All lanes
// of a block work on the same path at the same time: the path's slots are LDS broadcast reads,
// m is block-uniform and selects a fully unrolled body (path_term<M>, M = 1..10) in which
// every per-element array has static indices and lives in registers; the Gauss-Legendre nodes
// and weights are compile-time indices into constant memory.
//
// LDS (160 KiB per CU) of a block of R rows:
//   path chunk   kChunkSlots * 16 B = 8 KiB
//   row tile     R * (F | 1) * 4 B          (lane-private rows, odd stride: conflict-free)
//   accumulators R * ((F + 1) | 1) * 4 B    (lane-private rows, odd stride; the feature index
//                is a run-time value, so they cannot be registers.  Row-major rather than
//                [F + 1][R]: both are conflict-free while every lane adds to the same feature,
//                and this one is also conflict-free and coalesced when the block writes the
//                tile out cooperatively)
// R is the one of 256 / 128 / 64 with the most waves per CU by that budget (ties: the larger).
// Derived, not measured: F = 28 gives 256-row blocks of 67 KiB, two per CU (8 waves; 128 rows:
// 37.7 KiB, four blocks, the same 8 waves); F = 100: 128 rows, 109 KiB; F = 200: 64 rows,
// 109 KiB; from F = 304 on 64 rows no longer fit and the no-staging variant runs: rows are read
// from global memory and the accumulators are the output rows themselves (lane-private, in
// L2).  Nothing here is tuned for large F.  The kernel should be bound by fp32 VALU work (about
// 4 m Q + 8 m operations per row and path), not by HBM.  Measured (profiles/
// gbdt_contribs_bench.txt): 2M x 28 rows, 100 depth-6 trees (6,304 paths): 71.6 ms, the cover
// pass over 65,536 rows 0.18 ms; the split between VALU and LDS time has not been measured.
#include "common.h"
#include "gbdt_node.h"
#include "kdl_api.h"

namespace kdl {
namespace {

constexpr int kChunkNodes = 512;  // cover pass: GbdtNodes per LDS chunk (predict's)
constexpr int kChunkSlots = 512;  // contributions: 16-byte path slots per LDS chunk
constexpr int kMaxPath = 10;      // merged elements per path (the grower's depth limit)
constexpr int kLdsMax = 160 * 1024;

// Gauss-Legendre on [0, 1], rules of 1..5 nodes, row Q - 1: node t, 1 - t, weight
__constant__ float kGlT[5][5] = {
    {0.5f},
    {0.21132486540518713f, 0.7886751345948129f},
    {0.1127016653792583f, 0.5f, 0.8872983346207417f},
    {0.06943184420297371f, 0.33000947820757187f, 0.6699905217924281f, 0.9305681557970262f},
    {0.04691007703066802f, 0.23076534494715845f, 0.5f, 0.7692346550528415f, 0.9530899229693319f}};
__constant__ float kGlU[5][5] = {
    {0.5f},
    {0.7886751345948129f, 0.21132486540518713f},
    {0.8872983346207417f, 0.5f, 0.1127016653792583f},
    {0.9305681557970262f, 0.6699905217924281f, 0.33000947820757187f, 0.06943184420297371f},
    {0.9530899229693319f, 0.7692346550528415f, 0.5f, 0.23076534494715845f, 0.04691007703066802f}};
__constant__ float kGlW[5][5] = {
    {1.0f},
    {0.5f, 0.5f},
    {0.2777777777777778f, 0.4444444444444444f, 0.2777777777777778f},
    {0.1739274225687269f, 0.32607257743127305f, 0.32607257743127305f, 0.1739274225687269f},
    {0.11846344252809454f, 0.23931433524968324f, 0.28444444444444444f, 0.23931433524968324f,
     0.11846344252809454f}};

// stage the block's row tile: coalesced read of cnt * F contiguous floats, row stride ``stride``
template <int R>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int cnt, int F, int stride,
                                           float* __restrict__ xs) {
  const int total = cnt * F;
  for (int i = threadIdx.x; i < total; i += R) {
    const int r = i / F;
    xs[r * stride + (i - r * F)] = src[i];
  }
}

// ------------------------------------------------------------------ cover pass
// one row through one tree of ``n`` nodes: every node stepped onto (not the root) is counted
template <typename Count>
__device__ __forceinline__ void walk_count(const GbdtNode* __restrict__ nodes, int n, const float* __restrict__ x,
                                           int F, Count count) {
  int i = 0;
  GbdtNode nd = load_node(nodes);
  while (nd.feature >= 0) {
    if (nd.feature >= F) return;
    const int nx = nd.left + (x[nd.feature] <= nd.threshold ? 0 : 1);
    if (nx <= i || nx >= n) return;
    i = nx;
    count(i);
    nd = load_node(nodes + i);
  }
}

template <int R, bool STAGE>
__global__ __launch_bounds__(R) void forest_cover_kernel(const float* __restrict__ X, int64_t N, int F, int stride,
                                                         const GbdtNode* __restrict__ nodes, int num_nodes,
                                                         const int32_t* __restrict__ tree_off, int t0, int t1,
                                                         unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  GbdtNode* chunk = reinterpret_cast<GbdtNode*>(lds_raw);                                    // [kChunkNodes]
  int* cnt_lds = reinterpret_cast<int*>(lds_raw + kChunkNodes * sizeof(GbdtNode));           // [kChunkNodes]
  float* xs = reinterpret_cast<float*>(cnt_lds + kChunkNodes);                               // [R][stride] (STAGE)
  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * R;
  const int cnt = (N - row0) < R ? static_cast<int>(N - row0) : R;  // >= 1: the grid is ceil(N / R)
  const bool active = tid < cnt;
  const float* x;
  if constexpr (STAGE) {
    stage_rows<R>(X + row0 * F, cnt, F, stride, xs);
    x = xs + tid * stride;
    __syncthreads();
  } else {
    x = X + (row0 + (active ? tid : 0)) * F;
  }
  int t = t0;
  while (t < t1) {  // block-uniform, as in forest_predict_kernel
    const int base = tree_off[t];
    int e = t;
    int end = base;
    while (e < t1 && base >= 0) {
      const int nxt = tree_off[e + 1];
      if (nxt - base > kChunkNodes || nxt < end || nxt > num_nodes) break;
      end = nxt;
      ++e;
    }
    if (e == t) {
      // tree t alone is larger than the chunk: walk and count it in global memory
      const int n = tree_off[t + 1] - base;
      if (base >= 0 && n > 0 && n <= num_nodes - base) {
        unsigned long long* c = counts + base;
        if (tid == 0) atomicAdd(c, static_cast<unsigned long long>(cnt));
        if (active) walk_count(nodes + base, n, x, F, [c](int i) { atomicAdd(c + i, 1ull); });
      }
      ++t;
      continue;
    }
    __syncthreads();  // the previous chunk's flush is done
    {
      const int4* src = reinterpret_cast<const int4*>(nodes + base);
      int4* dst = reinterpret_cast<int4*>(chunk);
      for (int i = tid; i < end - base; i += R) {
        dst[i] = src[i];
        cnt_lds[i] = 0;
      }
    }
    __syncthreads();
    for (int u = t; u < e; ++u) {
      const int o = tree_off[u] - base;
      const int n = tree_off[u + 1] - base - o;
      if (n <= 0) continue;
      int* c = cnt_lds + o;
      if (tid == 0) atomicAdd(c, cnt);
      if (active) walk_count(chunk + o, n, x, F, [c](int i) { atomicAdd(c + i, 1); });
    }
    __syncthreads();
    for (int i = tid; i < end - base; i += R) {
      const int v = cnt_lds[i];
      if (v) atomicAdd(counts + base + i, static_cast<unsigned long long>(v));
    }
    t = e;
  }
}

// ------------------------------------------------------------------ contributions
// One row's terms of one path of exactly M elements.  ``p``: the path's slots in the LDS chunk
// (the same address in every lane: broadcast reads); ``x``: the row; ``acc``: its accumulators.
template <int M, int Q = (M + 1) / 2>
__device__ __forceinline__ void path_term(const int4* __restrict__ p, const float* __restrict__ x, int F,
                                          float* __restrict__ acc) {
  const float v = __int_as_float(p[0].x);
  int f[M];
  float z[M], d[M], step[M], W[M];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int4 e = p[1 + j];
    f[j] = e.x & 0x3fffffff;
    ok = ok && f[j] < F;
  }
  if (!ok) return;  // block-uniform: a broken table adds nothing
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int4 e = p[1 + j];
    const int4 r = p[1 + M + j / 4];
    const float omz = __int_as_float(j % 4 == 0 ? r.x : j % 4 == 1 ? r.y : j % 4 == 2 ? r.z : r.w);
    const float xv = x[f[j]];
    const bool has_left = (e.x >> 30) & 1;
    const bool o = !(xv <= __int_as_float(e.y)) && (!has_left || xv <= __int_as_float(e.z));
    z[j] = __int_as_float(e.w);
    d[j] = o ? omz : -z[j];  // o - z
    step[j] = o ? 1.f : 0.f;
    W[j] = 0.f;
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const float t = kGlT[Q - 1][q], u = kGlU[Q - 1][q];
    float fac[M], pre[M];
#pragma unroll
    for (int j = 0; j < M; ++j) fac[j] = fmaf(z[j], u, step[j] * t);  // o t + z (1 - t)
    pre[0] = kGlW[Q - 1][q];
#pragma unroll
    for (int j = 1; j < M; ++j) pre[j] = pre[j - 1] * fac[j - 1];
    float suf = 1.f;
#pragma unroll
    for (int j = M - 1; j >= 0; --j) {
      W[j] = fmaf(pre[j], suf, W[j]);
      suf *= fac[j];
    }
  }
#pragma unroll
  for (int j = 0; j < M; ++j) acc[f[j]] += v * d[j] * W[j];
}

template <int R, bool STAGE>
__global__ __launch_bounds__(R) void forest_contribs_kernel(const float* __restrict__ X, int64_t N, int F, int stride,
                                                            int astride, const int4* __restrict__ paths,
                                                            int num_slots, const int32_t* __restrict__ chunk_off,
                                                            int num_chunks, const int32_t* __restrict__ class_chunk,
                                                            const float* __restrict__ bias, int K,
                                                            float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int4* chunk = reinterpret_cast<int4*>(lds_raw);                                   // [kChunkSlots]
  float* xs = reinterpret_cast<float*>(lds_raw + kChunkSlots * sizeof(int4));       // [R][stride] (STAGE)
  float* accs = xs + R * stride;                                                    // [R][astride] (STAGE)
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
      acc = out + ((row0 + (active ? tid : 0)) * K + k) * F1;  // the output row itself
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
            case 1: path_term<1>(q, x, F, acc); break;
            case 2: path_term<2>(q, x, F, acc); break;
            case 3: path_term<3>(q, x, F, acc); break;
            case 4: path_term<4>(q, x, F, acc); break;
            case 5: path_term<5>(q, x, F, acc); break;
            case 6: path_term<6>(q, x, F, acc); break;
            case 7: path_term<7>(q, x, F, acc); break;
            case 8: path_term<8>(q, x, F, acc); break;
            case 9: path_term<9>(q, x, F, acc); break;
            default: path_term<10>(q, x, F, acc); break;
          }
        }
        p += len;
      }
    }
    const float b = bias[k];
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

size_t cover_lds(int R, bool stage, int stride) {
  return static_cast<size_t>(kChunkNodes) * (sizeof(GbdtNode) + sizeof(int)) +
         (stage ? static_cast<size_t>(R) * stride * sizeof(float) : 0);
}

size_t contribs_lds(int R, bool stage, int stride, int astride) {
  return static_cast<size_t>(kChunkSlots) * sizeof(int4) +
         (stage ? static_cast<size_t>(R) * (stride + astride) * sizeof(float) : 0);
}

// the R of 256 / 128 / 64 with the most waves per CU for ``fixed + R * per_row`` bytes of LDS
// (ties: the larger R); 0: not even 64 rows fit
int pick_rows(size_t fixed, size_t per_row) {
  int best = 0, best_waves = 0;
  for (int R = 256; R >= 64; R >>= 1) {
    const size_t lds = fixed + R * per_row;
    if (lds > static_cast<size_t>(kLdsMax)) continue;
    int blocks = static_cast<int>(kLdsMax / lds);
    const int cap = 32 / (R / 64);  // 32 waves per CU
    if (blocks > cap) blocks = cap;
    const int waves = blocks * (R / 64);
    if (waves > best_waves) {
      best_waves = waves;
      best = R;
    }
  }
  return best;
}

template <int R, bool STAGE>
hipError_t launch_cover(const float* X, int64_t N, int F, int stride, const GbdtNode* nodes, int num_nodes,
                        const int32_t* tree_off, int t0, int t1, int64_t* counts, size_t lds, hipStream_t s) {
  static bool attr_set = false;  // > 64 KiB of dynamic LDS must be opted into once
  if (!attr_set) {
    RETURN_IF_HIP_ERR(hipFuncSetAttribute(reinterpret_cast<const void*>(forest_cover_kernel<R, STAGE>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    attr_set = true;
  }
  const int64_t blocks = (N + R - 1) / R;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((forest_cover_kernel<R, STAGE>), dim3(static_cast<unsigned>(blocks)), dim3(R), lds, s, X, N, F,
                     stride, nodes, num_nodes, tree_off, t0, t1, reinterpret_cast<unsigned long long*>(counts));
  return hipGetLastError();
}

template <int R, bool STAGE>
hipError_t launch_contribs(const float* X, int64_t N, int F, int stride, int astride, const int32_t* paths,
                           int num_slots, const int32_t* chunk_off, int num_chunks, const int32_t* class_chunk,
                           const float* bias, int K, float* out, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    RETURN_IF_HIP_ERR(hipFuncSetAttribute(reinterpret_cast<const void*>(forest_contribs_kernel<R, STAGE>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    attr_set = true;
  }
  const int64_t blocks = (N + R - 1) / R;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((forest_contribs_kernel<R, STAGE>), dim3(static_cast<unsigned>(blocks)), dim3(R), lds, s, X, N,
                     F, stride, astride, reinterpret_cast<const int4*>(paths), num_slots, chunk_off, num_chunks,
                     class_chunk, bias, K, out);
  return hipGetLastError();
}

}  // namespace

int gbdt_contribs_chunk_slots() { return kChunkSlots; }

int gbdt_contribs_rows_per_block(int F) {
  return pick_rows(contribs_lds(0, false, 0, 0), static_cast<size_t>((F | 1) + ((F + 1) | 1)) * sizeof(float));
}

hipError_t gbdt_cover(const float* X, int64_t N, int F, const GbdtNode* nodes, int num_nodes, const int32_t* tree_off,
                      int t0, int t1, int64_t* counts, hipStream_t s) {
  if (N <= 0 || t1 <= t0) return hipSuccess;
  if (F < 1 || F > (1 << 20) || t0 < 0) return hipErrorInvalidValue;  // cnt * F stays an int
  const int stride = F | 1;
  const int R = pick_rows(cover_lds(0, false, 0), static_cast<size_t>(stride) * sizeof(float));
  const size_t lds = cover_lds(R, R != 0, stride);
  switch (R) {
    case 256: return launch_cover<256, true>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, counts, lds, s);
    case 128: return launch_cover<128, true>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, counts, lds, s);
    case 64: return launch_cover<64, true>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, counts, lds, s);
    default: return launch_cover<256, false>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, counts, lds, s);
  }
}

hipError_t gbdt_contribs(const float* X, int64_t N, int F, const int32_t* paths, int num_slots,
                         const int32_t* chunk_off, int num_chunks, const int32_t* class_chunk, const float* bias,
                         int K, float* out, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  if (F < 1 || F >= (1 << 20) || K < 1 || K > 32 || num_slots < 0 || num_chunks < 0) return hipErrorInvalidValue;
  const int stride = F | 1, astride = (F + 1) | 1;
  const int R = gbdt_contribs_rows_per_block(F);
  const size_t lds = contribs_lds(R, R != 0, stride, astride);
#define CONTRIBS_ARGS X, N, F, stride, astride, paths, num_slots, chunk_off, num_chunks, class_chunk, bias, K, out, lds, s
  switch (R) {
    case 256: return launch_contribs<256, true>(CONTRIBS_ARGS);
    case 128: return launch_contribs<128, true>(CONTRIBS_ARGS);
    case 64: return launch_contribs<64, true>(CONTRIBS_ARGS);
    default: return launch_contribs<256, false>(CONTRIBS_ARGS);
  }
#undef CONTRIBS_ARGS
}

}  // namespace kdl
