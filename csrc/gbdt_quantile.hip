// Exact segmented quantile select for the GBDT's adaptive leaves (gfx950):
// reg:absoluteerror / reg:quantileerror set every leaf to the alpha-quantile of
// the residuals of its rows, and the base margin to the alpha-quantile of y.
//
// Definition.  Positions 0..n-1 hold one fp32 key each; segment s owns the
// positions [seg_lo[s], seg_hi[s]) (disjoint ranges, clamped to [0, n]; on several
// ranks every rank holds a shard of every segment).  With n_s the segment's count
// over all ranks the result is sorted(keys of s)[t_s], t_s = max(ceil(alpha * n_s)
// - 1, 0), the product and the ceil in fp64; 0.0f for n_s = 0.  Keys are NaN-free
// (the caller's contract).
//
// Method: a most-significant-digit radix select over the order-preserving image
// of the float (all bits flipped when the sign bit is set, else the sign bit
// flipped: unsigned order = float order, -0 just below +0).  Per pass
//   count: hist[s][d] += #rows of s whose higher digits equal the segment's prefix
//          and whose next digit is d (int64 counts; all-reduced between the two
//          kernels when there are several ranks),
//   step:  one wave per segment scans the 256 counts for the digit that holds rank
//          t_s, appends it to the prefix, takes the counts below it off t_s and
//          zeroes the histogram for the next pass (self-cleaning workspace).
// After the last pass the prefix is the answer's bit pattern.  Counts are integers:
// the result does not depend on the order of the atomics, on the chunking or on the
// number of ranks.  No host synchronisation, no vendor sort or scan.
//
// Digits: 8 bits, 4 passes.  The table that the ranks all-reduce per pass is
// [S][256] int64 (2 MiB at S = 1024; 11-bit digits would make it 16 MiB for one
// pass less), and a block keeps one 1 KiB int32 counter set PER WAVE (4 KiB of LDS;
// 8 KiB each with 11 bits), so waves never contend with each other.
//
// Work split: a chunk is <= kChunk consecutive positions of one segment
// (quantile_plan_kernel: chunks per segment, exclusive prefix -- the scheme of
// hist_plan_kernel / hist_build_wq_kernel in gbdt.hip); block -> (segment, chunk)
// by binary search over the prefix.  The grower's leaves are such ranges: a node
// that stops splitting keeps its positions [lo, hi) through every later level
// (partition_kernel copies the rows of non-split nodes in place), so
// leaf_plan_kernel only collects (lo, hi) of the tree's leaves, compacted in heap
// order (the same order on every rank: the ranks grow identical trees).
//
// Pass 0 forms the key -- the residual y[rows[p]] - pred[rows[p] * ld + k], one
// fp32 subtraction, or y[p] itself without a row order -- and stores its image in
// position order, so the gathers through ``rows`` happen once and later passes
// stream 4 bytes per position.
//
// Contention: with all keys equal every lane of a wave wants one counter in every
// pass.  Before the LDS add a wave peels its two most wanted digits: the digit of
// the first live lane is broadcast, the lanes that hold it are counted by a ballot
// and one lane adds the population count.  All-equal keys therefore cost one LDS
// add per wave and row group, two values two; what is left goes to the wave's own
// counters lane by lane.
#include "common.h"
#include "kdl_api.h"

namespace kdl {
namespace {

constexpr int kChunk = 2048;   // positions per chunk (8 per thread)
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kDigits = 256;
constexpr int kPasses = 4;
constexpr int kItems = kChunk / kBlock;
constexpr int kMaxSeg = 1024;  // segments per call: one thread each in the plan kernels

__device__ __forceinline__ uint32_t key_image(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_value(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// exclusive scan of one int per thread over a 1024-thread block; *total = the block's sum
__device__ __forceinline__ int block_excl_scan1024(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int x = wave_incl_scan(v);
  __syncthreads();  // wsum reuse across calls
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k < w) pre += wsum[k];
    tot += wsum[k];
  }
  *total = tot;
  return pre + x - v;
}

// chunk_off[s] = chunks of the segments before s, chunk_off[S] = all chunks (S <= 1024, one block)
__device__ __forceinline__ void plan_chunks(const int32_t* seg_lo, const int32_t* seg_hi, int S, int n,
                                            int32_t* chunk_off, int* wsum) {
  const int s = threadIdx.x;
  int c = 0;
  if (s < S) {
    const int lo = clampi(seg_lo[s], 0, n), hi = clampi(seg_hi[s], 0, n);
    c = hi > lo ? (hi - lo + kChunk - 1) / kChunk : 0;
  }
  int total;
  const int ex = block_excl_scan1024(c, wsum, &total);
  if (s < S) chunk_off[s] = ex;
  if (s == 0) chunk_off[S] = total;
}

__global__ __launch_bounds__(1024) void quantile_plan_kernel(const int32_t* __restrict__ seg_lo,
                                                             const int32_t* __restrict__ seg_hi, int S, int n,
                                                             int32_t* __restrict__ chunk_off) {
  __shared__ int wsum[16];
  plan_chunks(seg_lo, seg_hi, S, n, chunk_off, wsum);
}

// The current tree's leaves as segments: heap node h (level d, index i) is a leaf when it
// exists and has no split feature; leaf j in heap order gets (lo, hi) of its level and
// seg_node[j] = h.  The S - #leaves slots behind them are empty with seg_node = -1.
__global__ __launch_bounds__(1024) void leaf_plan_kernel(GbdtLevelSegs lv, const int32_t* __restrict__ t_feat, int D,
                                                         int n, int S, int32_t* seg_lo, int32_t* seg_hi,
                                                         int32_t* __restrict__ seg_node,
                                                         int32_t* __restrict__ chunk_off) {
  __shared__ int wsum[16];
  const int heap = (1 << (D + 1)) - 1;
  int carry = 0;
  for (int h0 = 0; h0 < heap; h0 += 1024) {
    const int h = h0 + threadIdx.x;
    int leaf = 0, lo = 0, hi = 0;
    if (h < heap) {
      const int d = 31 - __clz(h + 1), i = h + 1 - (1 << d);
      leaf = (lv.exists[d][i] != 0 && t_feat[h] < 0) ? 1 : 0;
      lo = lv.lo[d][i];
      hi = lv.hi[d][i];
    }
    int total;
    const int j = carry + block_excl_scan1024(leaf, wsum, &total);
    if (leaf && j < S) {
      seg_lo[j] = lo;
      seg_hi[j] = hi;
      seg_node[j] = h;
    }
    carry += total;
  }
  for (int j = carry + static_cast<int>(threadIdx.x); j < S; j += 1024) {
    seg_lo[j] = 0;
    seg_hi[j] = 0;
    seg_node[j] = -1;
  }
  __syncthreads();  // the bounds above are read back by other threads of this block
  plan_chunks(seg_lo, seg_hi, S, n, chunk_off, wsum);
}

// cnt[digit] += 1 for every active lane of the wave, equal digits aggregated (file header)
__device__ __forceinline__ void wave_count(int* cnt, int digit, bool active) {
  const int lane = threadIdx.x & 63;
  unsigned long long live = __ballot(active);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (live == 0) break;  // wave-uniform
    const int leader = __ffsll(live) - 1;
    const int d0 = __shfl(digit, leader, 64);
    const unsigned long long same = __ballot(active && digit == d0);
    if (lane == leader) atomicAdd(&cnt[d0], __popcll(same));
    active = active && digit != d0;
    live &= ~same;
  }
  if (active) atomicAdd(&cnt[digit], 1);
}

// One pass's digit histogram.  PASS0: form the keys (rows == nullptr: key = y[p]) and store
// their images; later passes read the images and count the rows that match the prefix.
template <bool PASS0>
__global__ __launch_bounds__(kBlock) void quantile_count_kernel(
    int pass, const float* __restrict__ y, const float* __restrict__ pred, int ld, int k,
    const int32_t* __restrict__ rows, uint32_t* __restrict__ ukeys, int n, const int32_t* __restrict__ seg_lo,
    const int32_t* __restrict__ seg_hi, const int32_t* __restrict__ chunk_off, int S,
    const uint32_t* __restrict__ prefix, unsigned long long* __restrict__ hist) {
  __shared__ int cnt[kWaves][kDigits];
  const int t = threadIdx.x, w = t >> 6;
  const int total = chunk_off[S];
  const int shift = 24 - 8 * pass;
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
#pragma unroll
    for (int i = 0; i < kWaves; ++i) cnt[i][t] = 0;
    int a = 0, b = S;  // chunk_off[a] <= c < chunk_off[b]
    while (b - a > 1) {
      const int m = (a + b) >> 1;
      if (chunk_off[m] <= c) a = m; else b = m;
    }
    const int s = a;
    const int lo = clampi(seg_lo[s], 0, n), hi = clampi(seg_hi[s], 0, n);
    const int p0 = lo + (c - chunk_off[s]) * kChunk;
    const int p1 = min(hi, p0 + kChunk);
    const uint32_t pre = PASS0 ? 0u : prefix[s];
    __syncthreads();
    uint32_t u[kItems];
    if (PASS0) {
      int row[kItems];
      float yv[kItems], pv[kItems];
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const int p = p0 + i * kBlock + t;
        row[i] = p < p1 ? (rows != nullptr ? rows[p] : p) : -1;
      }
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        yv[i] = row[i] >= 0 ? y[row[i]] : 0.f;
        pv[i] = (row[i] >= 0 && pred != nullptr) ? pred[static_cast<int64_t>(row[i]) * ld + k] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const int p = p0 + i * kBlock + t;
        u[i] = key_image(pred != nullptr ? yv[i] - pv[i] : yv[i]);
        if (p < p1) ukeys[p] = u[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const int p = p0 + i * kBlock + t;
        u[i] = p < p1 ? ukeys[p] : 0u;
      }
    }
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
      const int p = p0 + i * kBlock + t;
      const bool match = PASS0 || (u[i] >> (shift + 8)) == pre;
      wave_count(cnt[w], static_cast<int>((u[i] >> shift) & 255u), p < p1 && match);
    }
    __syncthreads();
    int v = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) v += cnt[i][t];
    if (v) atomicAdd(hist + static_cast<int64_t>(s) * kDigits + t, static_cast<unsigned long long>(v));
    // (the next chunk's zeroing touches cnt[.][t] only: this thread's own reads above)
  }
}

// One wave per segment: the digit of this pass, the rank inside it, the histogram zeroed.
// target[s] < 0 marks an empty segment.  After the last pass out[seg_node[s]] = scale * q
// (seg_node given: the grower's val array, slots with node -1 skipped) or out[s] = q.
__global__ __launch_bounds__(kBlock) void quantile_step_kernel(int pass, double alpha,
                                                               unsigned long long* __restrict__ hist, int S,
                                                               uint32_t* __restrict__ prefix,
                                                               long long* __restrict__ target,
                                                               const int32_t* __restrict__ seg_node, float scale,
                                                               float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (s >= S) return;  // wave-uniform
  unsigned long long* h = hist + static_cast<int64_t>(s) * kDigits + lane * 4;
  long long c[4], ls = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = static_cast<long long>(h[j]);
    h[j] = 0ull;
    ls += c[j];
  }
  const long long incl = wave_incl_scan(ls);
  const long long total = __shfl(incl, 63, 64);
  uint32_t pre = 0u;
  long long t;
  if (pass == 0) {
    t = -1;
    if (total > 0) {
      t = static_cast<long long>(ceil(alpha * static_cast<double>(total))) - 1;
      t = t < 0 ? 0 : (t > total - 1 ? total - 1 : t);
    }
  } else {
    pre = prefix[s];
    t = target[s];
  }
  const bool last = pass == kPasses - 1;
  const int node = seg_node != nullptr ? seg_node[s] : s;
  if (t < 0) {
    if (lane == 0) {
      if (pass == 0) {
        prefix[s] = 0u;
        target[s] = -1;
      }
      if (last && node >= 0) out[node] = 0.f;
    }
    return;
  }
  long long below = incl - ls;
  if (t >= below && t < incl) {  // exactly one lane
    int digit = lane * 4;
    bool go = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      go = go && t >= below + c[j];
      if (go) {
        below += c[j];
        ++digit;
      }
    }
    const uint32_t np = (pre << 8) | static_cast<uint32_t>(digit);
    prefix[s] = np;
    target[s] = t - below;
    if (last && node >= 0) {
      const float q = key_value(np);
      out[node] = seg_node != nullptr ? scale * q : q;
    }
  }
}

hipError_t launch_count(int pass, const float* y, const float* pred, int ld, int k, const int32_t* rows,
                        uint32_t* ukeys, int n, const int32_t* seg_lo, const int32_t* seg_hi,
                        const int32_t* chunk_off, int S, const uint32_t* prefix, int64_t* hist, hipStream_t s) {
  const int max_chunks = (n + kChunk - 1) / kChunk + S;  // disjoint ranges: at most one partial chunk each
  auto* hp = reinterpret_cast<unsigned long long*>(hist);
  if (pass == 0)
    hipLaunchKernelGGL(quantile_count_kernel<true>, dim3(max_chunks), dim3(kBlock), 0, s, pass, y, pred, ld, k, rows,
                       ukeys, n, seg_lo, seg_hi, chunk_off, S, prefix, hp);
  else
    hipLaunchKernelGGL(quantile_count_kernel<false>, dim3(max_chunks), dim3(kBlock), 0, s, pass, y, pred, ld, k,
                       rows, ukeys, n, seg_lo, seg_hi, chunk_off, S, prefix, hp);
  return hipGetLastError();
}

}  // namespace

int gbdt_quantile_chunk_rows() { return kChunk; }
int gbdt_quantile_digits() { return kDigits; }
int gbdt_quantile_passes() { return kPasses; }
int gbdt_quantile_max_segments() { return kMaxSeg; }

hipError_t gbdt_quantile_plan(const int32_t* seg_lo, const int32_t* seg_hi, int S, int n, int32_t* chunk_off,
                              hipStream_t s) {
  if (S < 1 || S > kMaxSeg || n < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantile_plan_kernel, dim3(1), dim3(1024), 0, s, seg_lo, seg_hi, S, n, chunk_off);
  return hipGetLastError();
}

hipError_t gbdt_quantile_leaf_plan(const GbdtLevelSegs& lv, const int32_t* t_feat, int D, int n, int S,
                                   int32_t* seg_lo, int32_t* seg_hi, int32_t* seg_node, int32_t* chunk_off,
                                   hipStream_t s) {
  if (D < 0 || D >= kGbdtLevels || S < (1 << D) || S > kMaxSeg || n < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(leaf_plan_kernel, dim3(1), dim3(1024), 0, s, lv, t_feat, D, n, S, seg_lo, seg_hi, seg_node,
                     chunk_off);
  return hipGetLastError();
}

hipError_t gbdt_quantile_count(int pass, const float* y, const float* pred, int ld, int k, const int32_t* rows,
                               uint32_t* ukeys, int n, const int32_t* seg_lo, const int32_t* seg_hi,
                               const int32_t* chunk_off, int S, const uint32_t* prefix, int64_t* hist,
                               hipStream_t s) {
  if (pass < 0 || pass >= kPasses || S < 1 || S > kMaxSeg || n < 0) return hipErrorInvalidValue;
  if (pred != nullptr && (ld < 1 || k < 0 || k >= ld)) return hipErrorInvalidValue;
  return launch_count(pass, y, pred, ld, k, rows, ukeys, n, seg_lo, seg_hi, chunk_off, S, prefix, hist, s);
}

hipError_t gbdt_quantile_step(int pass, double alpha, int64_t* hist, int S, uint32_t* prefix, int64_t* target,
                              const int32_t* seg_node, float scale, float* out, hipStream_t s) {
  if (pass < 0 || pass >= kPasses || S < 1 || S > kMaxSeg || !(alpha >= 0.0 && alpha <= 1.0))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantile_step_kernel, dim3((S + kWaves - 1) / kWaves), dim3(kBlock), 0, s, pass, alpha,
                     reinterpret_cast<unsigned long long*>(hist), S, prefix, reinterpret_cast<long long*>(target),
                     seg_node, scale, out);
  return hipGetLastError();
}

}  // namespace kdl
