// Forest inference for the histogram GBDT (gfx950): HistGBDT.predict and the
// validation margin of HistGBDT.fit(eval_set=...).
//
// Semantics (those of HistGBDT.predict_margin, the torch reference): for every
// row n and every tree t of [t0, t1) in tree order, walk from the root with
// ``x[feature] <= threshold ? left : left + 1`` (NaN compares false and goes
// right; a +inf threshold sends everything but NaN left) to the first leaf and
// add its value to margin[n, t % K] in fp32.  ONE LANE owns a row's K
// accumulators from the first tree to the last: no atomics, no split of a
// row's trees across lanes or blocks, so the sums are taken in the reference's
// order and the result is bit-identical to it.
//
// Forest: GbdtNode (kdl_api.h), 16 aligned bytes per node (the compiler reads
// feature / threshold + left per step and the value at the leaf); children are
// an adjacent pair (right = left + 1) with indices relative to the tree's
// first node and larger than the parent's.
// The walk checks ``parent < child < tree size`` and ``feature < F`` on every
// step: a table that breaks them cannot send a lane out of bounds or into a
// cycle, and a tree whose offsets leave the table is skipped (such a tree adds
// nothing or 0; the Python packer rejects such a table before it gets here).
//
// Block = R rows, one lane per row (R = 256 / 128 / 64 threads).
//   * the block's row tile is staged in LDS once (coalesced read of R * F
//     contiguous floats) with row stride F | 1: the 32 lanes of a ds_read_b32
//     group read 32 different rows, usually at the same column near the root,
//     and an odd stride spreads those over all 32 banks (stride 28 would put
//     them on 8).  A row's random feature reads then cost an LDS access, not a
//     strided global one (F * 4 bytes apart: one 128-byte line per lane).
//   * the node table streams through an 8 KiB LDS chunk (kChunkNodes = 512
//     nodes) holding WHOLE trees: four depth-6 trees (127 nodes each) per
//     chunk, i.e. two barriers and one 8 KiB cooperative copy per four trees.
//     A tree larger than the chunk (depth >= 9; a depth-10 heap is 32 KiB) is
//     walked straight from global memory / L2 instead -- every block reads the
//     same 32 KiB, so it stays cache resident.
//   * a lane walks the chunk's trees FOUR AT A TIME (walk_many): four
//     independent chains of dependent LDS reads in flight, the leaves then added
//     in tree order.  Measured on 2M x 28, 100 depth-6 trees: 1.40 ms one tree
//     at a time, 0.86 ms two, 0.80 ms four (profiles/gbdt_predict_walks.txt).
//   * K == 1 keeps the accumulator in a register; K > 1 keeps K of them per
//     lane in LDS ([K][R], lane-private and conflict-free) because the class
//     of a tree is a run-time index.
//
// Sizes against the CU's 160 KiB of LDS.  The walk is a chain of dependent LDS
// reads (node, then feature value, per level), so it is latency bound and wants
// waves: at F = 28, K = 1 a 256-row block uses 8 KiB + 256 * 29 * 4 = 37.7 KiB
// -> 4 blocks = 16 waves per CU (4 per SIMD).  A 16 KiB chunk halves the
// barriers per tree (and would feed eight walks at once) but drops that to 3
// blocks: measured 0.89-0.92 ms against 0.80 (10 KiB: 0.90); a 4 KiB chunk buys
// no fifth block (the row tile alone is 29.7 KiB), holds two trees, and
// measured 0.93 ms.  For other F and K the launcher picks the R with the most
// waves per CU (ties: the larger R, fewer node copies per row): F = 200 gives
// 128-row blocks of 110 KiB, one per CU.  When not even 64
// rows fit (F > ~600) the rows stay in global memory (the no-staging variant).
// Large F therefore runs at 1-2 waves per CU; nothing here is tuned for it.
#include "common.h"
#include "kdl_api.h"

namespace kdl {
namespace {

constexpr int kChunkNodes = 512;
constexpr int kWalks = 4;  // trees of a chunk walked at once per lane
constexpr int kChunkBytes = kChunkNodes * static_cast<int>(sizeof(GbdtNode));
constexpr int kLdsMax = 160 * 1024;
static_assert(sizeof(GbdtNode) == 16, "GbdtNode is one 16-byte load");

__device__ __forceinline__ GbdtNode load_node(const GbdtNode* p) {
  const int4 v = *reinterpret_cast<const int4*>(p);
  GbdtNode n;
  n.feature = v.x;
  n.threshold = __int_as_float(v.y);
  n.left = v.z;
  n.value = __int_as_float(v.w);
  return n;
}

// one row through one tree of ``n`` nodes; false: the table is broken at this walk
__device__ __forceinline__ bool walk(const GbdtNode* __restrict__ nodes, int n, const float* __restrict__ x, int F,
                                     float* leaf) {
  int i = 0;
  GbdtNode nd = load_node(nodes);
  while (nd.feature >= 0) {
    if (nd.feature >= F) return false;
    const int nx = nd.left + (x[nd.feature] <= nd.threshold ? 0 : 1);
    if (nx <= i || nx >= n) return false;
    i = nx;
    nd = load_node(nodes + i);
  }
  *leaf = nd.value;
  return true;
}

// one row through U trees of the LDS chunk at once: U independent chains of dependent reads
// in flight per lane, branch-free (a walk that has reached its leaf re-reads it until the
// lane's last walk ends; a broken step ends its walk with the value 0).  The leaves come
// back per tree, so the caller still adds them in tree order.
template <int U>
__device__ __forceinline__ void walk_many(const GbdtNode* __restrict__ chunk, const int (&o)[U], const int (&n)[U],
                                          const float* __restrict__ x, int F, float (&leaf)[U]) {
  int i[U];
  GbdtNode nd[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    i[u] = 0;
    nd[u] = load_node(chunk + o[u]);
  }
  bool any;
  do {
    float xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int f = nd[u].feature;
      xv[u] = x[static_cast<unsigned>(f) < static_cast<unsigned>(F) ? f : 0];
    }
    any = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int f = nd[u].feature;
      const bool split = f >= 0;
      const int nx = nd[u].left + (xv[u] <= nd[u].threshold ? 0 : 1);
      const bool ok = f < F && nx > i[u] && nx < n[u];
      i[u] = (split && ok) ? nx : i[u];
      GbdtNode nn = load_node(chunk + o[u] + i[u]);
      if (split && !ok) {
        nn.feature = -1;
        nn.value = 0.f;
      }
      nd[u] = nn;
      any |= nn.feature >= 0;
    }
  } while (any);
#pragma unroll
  for (int u = 0; u < U; ++u) leaf[u] = nd[u].value;
}

template <int R, bool STAGE, bool KONE>
__global__ __launch_bounds__(R) void forest_predict_kernel(const float* __restrict__ X, int64_t N, int F, int stride,
                                                           const GbdtNode* __restrict__ nodes, int num_nodes,
                                                           const int32_t* __restrict__ tree_off, int t0, int t1,
                                                           int K, float* __restrict__ margin) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  GbdtNode* chunk = reinterpret_cast<GbdtNode*>(lds_raw);               // [kChunkNodes]
  float* acc = reinterpret_cast<float*>(lds_raw + kChunkBytes);         // [K][R] (K > 1)
  float* xs = acc + (KONE ? 0 : K * R);                                 // [R][stride] (STAGE)
  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * R;
  const int cnt = (N - row0) < R ? static_cast<int>(N - row0) : R;  // >= 1: the grid is ceil(N / R)
  const bool active = tid < cnt;
  const float* x;
  if constexpr (STAGE) {
    const float* src = X + row0 * F;
    const int total = cnt * F;
    for (int i = tid; i < total; i += R) {
      const int r = i / F;
      xs[r * stride + (i - r * F)] = src[i];
    }
    x = xs + tid * stride;
  } else {
    x = X + (row0 + (active ? tid : 0)) * F;
  }
  float a0 = 0.f;
  if (active) {
    float* m = margin + (row0 + tid) * K;
    if (KONE) {
      a0 = m[0];
    } else {
      for (int k = 0; k < K; ++k) acc[k * R + tid] = m[k];
    }
  }
  // (the first chunk's barrier below also orders the row tile's stores before the walks)
  if (STAGE) __syncthreads();
  int t = t0;
  int k = t0 % K;
  while (t < t1) {  // block-uniform: t, e and the offsets are the same in every lane
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
      // tree t alone is larger than the chunk: walk it from global memory
      const int n = tree_off[t + 1] - base;
      float v;
      if (active && base >= 0 && n > 0 && n <= num_nodes - base && walk(nodes + base, n, x, F, &v)) {
        if (KONE) a0 += v; else acc[k * R + tid] += v;
      }
      ++t;
      k = (k + 1 == K) ? 0 : k + 1;
      continue;
    }
    __syncthreads();  // the previous chunk's walks are done
    {
      const int4* src = reinterpret_cast<const int4*>(nodes + base);
      int4* dst = reinterpret_cast<int4*>(chunk);
      for (int i = tid; i < end - base; i += R) dst[i] = src[i];
    }
    __syncthreads();
    int u = t;
    for (; u + kWalks <= e; u += kWalks) {  // kWalks trees at once, then the rest one by one
      int o[kWalks], n[kWalks];
      bool full = true;
#pragma unroll
      for (int j = 0; j < kWalks; ++j) {
        o[j] = tree_off[u + j] - base;
        n[j] = tree_off[u + j + 1] - base - o[j];
        full = full && n[j] > 0;
      }
      if (!full) break;  // an empty tree: one at a time below
      if (active) {
        float v[kWalks];
        walk_many<kWalks>(chunk, o, n, x, F, v);
#pragma unroll
        for (int j = 0; j < kWalks; ++j) {  // in tree order
          if (KONE) a0 += v[j]; else acc[((k + j) % K) * R + tid] += v[j];
        }
      }
      k = (k + kWalks) % K;
    }
    for (; u < e; ++u) {
      const int o = tree_off[u] - base;
      const int n = tree_off[u + 1] - base - o;
      float v;
      if (active && n > 0 && walk(chunk + o, n, x, F, &v)) {
        if (KONE) a0 += v; else acc[k * R + tid] += v;
      }
      k = (k + 1 == K) ? 0 : k + 1;
    }
    t = e;
  }
  if (active) {
    float* m = margin + (row0 + tid) * K;
    if (KONE) {
      m[0] = a0;
    } else {
      for (int kk = 0; kk < K; ++kk) m[kk] = acc[kk * R + tid];
    }
  }
}

__global__ __launch_bounds__(256) void heap_to_nodes_kernel(const float* __restrict__ packed, int heap,
                                                            GbdtNode* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= heap) return;
  const int f = static_cast<int>(packed[i]);
  const bool split = f >= 0 && 2 * i + 2 < heap;
  int4 v;
  v.x = split ? f : -1;
  v.y = __float_as_int(packed[2 * heap + i]);
  v.z = split ? 2 * i + 1 : -1;
  v.w = __float_as_int(packed[3 * heap + i]);
  *reinterpret_cast<int4*>(out + i) = v;
}

size_t predict_lds(int R, bool stage, int stride, int K) {
  return static_cast<size_t>(kChunkBytes) + (K > 1 ? static_cast<size_t>(K) * R * sizeof(float) : 0) +
         (stage ? static_cast<size_t>(R) * stride * sizeof(float) : 0);
}

template <int R, bool STAGE, bool KONE>
hipError_t launch_predict(const float* X, int64_t N, int F, int stride, const GbdtNode* nodes, int num_nodes,
                          const int32_t* tree_off, int t0, int t1, int K, float* margin, size_t lds, hipStream_t s) {
  static bool attr_set = false;  // > 64 KiB of dynamic LDS must be opted into once
  if (!attr_set) {
    RETURN_IF_HIP_ERR(hipFuncSetAttribute(reinterpret_cast<const void*>(forest_predict_kernel<R, STAGE, KONE>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    attr_set = true;
  }
  const int64_t blocks = (N + R - 1) / R;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((forest_predict_kernel<R, STAGE, KONE>), dim3(static_cast<unsigned>(blocks)), dim3(R), lds, s,
                     X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, K, margin);
  return hipGetLastError();
}

template <bool KONE>
hipError_t dispatch_predict(int R, const float* X, int64_t N, int F, int stride, const GbdtNode* nodes, int num_nodes,
                            const int32_t* tree_off, int t0, int t1, int K, float* margin, size_t lds,
                            hipStream_t s) {
  switch (R) {
    case 256: return launch_predict<256, true, KONE>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, K, margin, lds, s);
    case 128: return launch_predict<128, true, KONE>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, K, margin, lds, s);
    case 64: return launch_predict<64, true, KONE>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, K, margin, lds, s);
    default: return launch_predict<256, false, KONE>(X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, K, margin, lds, s);
  }
}

}  // namespace

int gbdt_predict_chunk_nodes() { return kChunkNodes; }

int gbdt_predict_rows_per_block(int F, int K) {
  const int stride = F | 1;
  int best = 0, best_waves = 0;
  for (int R = 256; R >= 64; R >>= 1) {
    const size_t lds = predict_lds(R, true, stride, K);
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
  return best;  // 0: the rows do not fit, no staging
}

hipError_t gbdt_predict(const float* X, int64_t N, int F, const GbdtNode* nodes, int num_nodes,
                        const int32_t* tree_off, int t0, int t1, int K, float* margin, hipStream_t s) {
  if (N <= 0 || t1 <= t0) return hipSuccess;
  if (F < 1 || K < 1 || K > 32 || t0 < 0) return hipErrorInvalidValue;
  if (F > (1 << 20)) return hipErrorInvalidValue;  // cnt * F stays an int
  const int stride = F | 1;
  const int R = gbdt_predict_rows_per_block(F, K);
  const size_t lds = predict_lds(R ? R : 256, R != 0, stride, K);
if (K == 1) return dispatch_predict<true>(R, X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, K, margin, lds, s);
  return dispatch_predict<false>(R, X, N, F, stride, nodes, num_nodes, tree_off, t0, t1, K, margin, lds, s);
}

hipError_t gbdt_heap_to_nodes(const float* packed, int heap, GbdtNode* out, hipStream_t s) {
  if (heap <= 0) return hipSuccess;
  hipLaunchKernelGGL(heap_to_nodes_kernel, dim3((heap + 255) / 256), dim3(256), 0, s, packed, heap, out);
  return hipGetLastError();
}

}  // namespace kdl
