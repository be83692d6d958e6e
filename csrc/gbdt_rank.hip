// Learning-to-rank gradients for the histogram GBDT (gfx950): the LambdaMART pair kernels of
// ``rank:pairwise`` / ``rank:ndcg`` and the DCG kernel of the ``ndcg@k`` metric.  The semantics
// (groups, gain, position, discount table, inv_idcg, pair terms) are defined once, in the module
// docstring of kubedl_amd/models/gbdt.py.
//
// A row's g and h are sums over every other row of its query group, and (rank:ndcg) the weights
// depend on each row's position under the current scores.  The work is split by a plan that the
// host builds once per fit from the group sizes (HistGBDT._rank_setup), one int32[4] record per
// unit of work:
//   wave slot   { first_row, n_q, inv_idcg bits, group }    groups of n_q <= 64, four to a block
//   block item  { first_row, n_q, inv_idcg bits, i0 }        rows [i0, i0 + 256) of a larger group
// Both lists are ordered by group size, largest first, so the four waves of a block run groups of
// nearly the same length and the long items start first.  Nothing of the plan is recomputed per
// round.
//
// No atomics anywhere: row i's g and h are accumulated by ONE lane, in registers, over j = 0 ..
// n_q - 1 in ascending order, whichever path serves the group -- bit-reproducible run to run and
// independent of the grid.  Every unordered pair is therefore evaluated twice, once from each side.
//
// ---- wave path (rank_wave_kernel): positions and lambdas fused, one launch
// Lane i keeps (s_i, G_i) in registers.  Pass 1 walks j with a v_readlane broadcast of lane j's
// score (j is wave-uniform, the value arrives in an SGPR) and counts
//   pos_i = #{ j : s_j > s_i or (s_j == s_i and j < i) },
// lane i reads D[pos_i], pass 2 walks j again with the broadcasts of (s_j, G_j, D_j).  No LDS, no
// barrier.
//
// ---- block path: rank_positions_kernel, then lambda_pairs_kernel, same (group, i-tile) items
// positions: the group's scores stream through LDS in j-chunks of 1,024 floats; the tile's 256
// lanes read them at a uniform address (an LDS broadcast, no bank conflict) and count as above;
// disc[row] = D[pos] goes to a per-fit workspace.  lambdas: per j-chunk the block stages 16-byte
// records { s_j, G_j, disc_j, y_j } in LDS (16 KiB), the inner loop is one 128-bit broadcast read
// per j.  The chunk loop means a group can be of any size; a 5,000-row group is 20 near-equal
// items.  rank:pairwise is the same code with w = 1 (template parameter) and no positions launch.
//
// What moved from the first design: the gain is carried as the INTEGER 2^y - 1 (uint32), not as a
// float.  |G_i - G_j| is then exact in integer arithmetic and rounded once by the conversion (at
// y >= 25 a float gain is already rounded, and the difference of two rounded gains would lose more),
// and G_i != G_j / G_i > G_j stand for the label comparisons, so the wave path broadcasts three
// values per j, not four.  The wave path also writes disc[row] (one coalesced store per group): the
// tests compare positions exactly through it on both paths.
//
// ---- one pair term (pair_term): rho and 1 - rho without cancellation or overflow
//   d = s_hi - s_lo,  a = expf(-|d|) in (0, 1],  r = 1 / (1 + a),  sm = a * r
//   rho = d > 0 ? sm : r,   rho (1 - rho) = sm * r   (either sign of d)
// a never overflows; where it underflows to 0, r is exactly 1 and sm exactly 0: rho is exactly 0 or
// 1 for d of large magnitude and no inf / inf can arise.  ``1 - rho`` is never formed by
// subtraction (it would lose every digit where rho is close to 1).  expf is the device library's
// (documented maximum error 1 ulp), the division is the correctly rounded one.  The file is built
// without packed fp32 operations, so every product and sum rounds once: tests/test_gbdt_rank.py
// counts them.
//
// ---- metric (rank_ndcg_kernel)
// One 256-lane block per group: positions as in the block path, then sum_i [pos_i < k] G_i D[pos_i]
// in fp64 (a fixed reduction tree per 256-row tile, the tiles added in row order), dcg[q] written by
// one lane.  The division by IDCG@k and the mean over groups are fp64 torch ops on [Q].
//
// Every kernel checks its plan record against N before it touches a row, and clamps the position
// to the discount table: a broken plan cannot send a lane out of bounds.
#include "common.h"
#include "kdl_api.h"

namespace kdl {
namespace {

constexpr int kTile = 256;     // rows of one block item (and lanes of every block here)
constexpr int kChunk = 1024;   // j rows per LDS chunk
constexpr float kMinHess = 1e-16f;

__device__ __forceinline__ uint32_t rank_gain(int y) { return (1u << (y & 31)) - 1u; }  // 2^y - 1, y in [0, 31]

__device__ __forceinline__ float lane_bcast(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ __forceinline__ uint32_t lane_bcast(uint32_t v, int j) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), j));
}

template <bool NDCG>
__device__ __forceinline__ void pair_term(float si, uint32_t gi, float di, float sj, uint32_t gj, float dj,
                                          float inv_idcg, float& g, float& h) {
  const bool i_hi = gi > gj;
  const float d = i_hi ? si - sj : sj - si;  // s_hi - s_lo
  const float a = expf(-fabsf(d));
  const float r = 1.0f / (1.0f + a);
  const float sm = a * r;
  const float rho = d > 0.f ? sm : r;
  float w;
  if (NDCG) {
    w = static_cast<float>(i_hi ? gi - gj : gj - gi) * fabsf(di - dj) * inv_idcg;
  } else {
    w = gi != gj ? 1.f : 0.f;
  }
  const float t = rho * w;
  g += i_hi ? -t : t;
  h += sm * r * w;
}

// ------------------------------------------------------------------ wave path
template <bool NDCG>
__global__ __launch_bounds__(256) void rank_wave_kernel(const float* __restrict__ score,
                                                        const int32_t* __restrict__ label,
                                                        const int4* __restrict__ plan, int slots, int64_t N,
                                                        const float* __restrict__ dtab, int dlen,
                                                        float* __restrict__ disc, float* __restrict__ g,
                                                        float* __restrict__ h) {
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= slots) return;
  const int lane = threadIdx.x & 63;
  const int4 p = plan[slot];
  const int first = __builtin_amdgcn_readfirstlane(p.x);
  const int n = __builtin_amdgcn_readfirstlane(p.y);
  const float inv_idcg = __int_as_float(__builtin_amdgcn_readfirstlane(p.z));
  if (first < 0 || n < 1 || n > kWave || static_cast<int64_t>(first) + n > N) return;
  const bool valid = lane < n;
  const float si = valid ? score[first + lane] : 0.f;
  const uint32_t gi = valid ? rank_gain(label[first + lane]) : 0u;
  float di = 0.f;
  if (NDCG) {
    int pos = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = lane_bcast(si, j);
      pos += (sj > si || (sj == si && j < lane)) ? 1 : 0;
    }
    di = dtab[min(pos, dlen - 1)];
    if (valid) disc[first + lane] = di;
  }
  float ga = 0.f, ha = 0.f;
  for (int j = 0; j < n; ++j) {
    const float sj = lane_bcast(si, j);
    const uint32_t gj = lane_bcast(gi, j);
    const float dj = NDCG ? lane_bcast(di, j) : 0.f;
    pair_term<NDCG>(si, gi, di, sj, gj, dj, inv_idcg, ga, ha);
  }
  if (valid) {
    g[first + lane] = ga;
    h[first + lane] = fmaxf(ha, kMinHess);
  }
}

// ------------------------------------------------------------------ block path
// pos of row i (score si) among the n scores at sg; every lane of the block calls it (barriers)
__device__ __forceinline__ int tile_positions(const float* __restrict__ sg, int n, int i, float si, float* sh) {
  int pos = 0;
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int cn = min(kChunk, n - c0);
    for (int t = threadIdx.x; t < cn; t += kTile) sh[t] = sg[c0 + t];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cn; ++j) {
      const float sj = sh[j];
      pos += (sj > si || (sj == si && c0 + j < i)) ? 1 : 0;
    }
    __syncthreads();
  }
  return pos;
}

// a block item's record, checked: false = skip the item (uniform over the block)
__device__ __forceinline__ bool load_item(const int4* __restrict__ plan, int64_t N, int& first, int& n, float& inv_idcg,
                                          int& i0) {
  const int4 p = plan[blockIdx.x];
  first = p.x;
  n = p.y;
  inv_idcg = __int_as_float(p.z);
  i0 = p.w;
  return first >= 0 && n >= 1 && static_cast<int64_t>(first) + n <= N && i0 >= 0 && i0 < n;
}

__global__ __launch_bounds__(kTile) void rank_positions_kernel(const float* __restrict__ score,
                                                               const int4* __restrict__ plan, int64_t N,
                                                               const float* __restrict__ dtab, int dlen,
                                                               float* __restrict__ disc) {
  __shared__ float sh[kChunk];
  int first, n, i0;
  float inv_idcg;
  if (!load_item(plan, N, first, n, inv_idcg, i0)) return;
  const int i = i0 + threadIdx.x;
  const bool valid = i < n;
  const float si = valid ? score[first + i] : 0.f;
  const int pos = tile_positions(score + first, n, i, si, sh);
  if (valid) disc[first + i] = dtab[min(pos, dlen - 1)];
}

template <bool NDCG>
__global__ __launch_bounds__(kTile) void lambda_pairs_kernel(const float* __restrict__ score,
                                                             const int32_t* __restrict__ label,
                                                             const int4* __restrict__ plan, int64_t N,
                                                             const float* __restrict__ disc, float* __restrict__ g,
                                                             float* __restrict__ h) {
  __shared__ int4 sh[kChunk];  // { s_j bits, G_j, disc_j bits, y_j }
  int first, n, i0;
  float inv_idcg;
  if (!load_item(plan, N, first, n, inv_idcg, i0)) return;
  const int i = i0 + threadIdx.x;
  const bool valid = i < n;
  const float si = valid ? score[first + i] : 0.f;
  const uint32_t gi = valid ? rank_gain(label[first + i]) : 0u;
  const float di = (NDCG && valid) ? disc[first + i] : 0.f;
  float ga = 0.f, ha = 0.f;
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int cn = min(kChunk, n - c0);
    for (int t = threadIdx.x; t < cn; t += kTile) {
      const int row = first + c0 + t;
      const int yj = label[row];
      sh[t] = make_int4(__float_as_int(score[row]), static_cast<int>(rank_gain(yj)),
                        NDCG ? __float_as_int(disc[row]) : 0, yj);
    }
    __syncthreads();
    for (int j = 0; j < cn; ++j) {
      const int4 r = sh[j];
      pair_term<NDCG>(si, gi, di, __int_as_float(r.x), static_cast<uint32_t>(r.y), __int_as_float(r.z), inv_idcg, ga,
                      ha);
    }
    __syncthreads();
  }
  if (valid) {
    g[first + i] = ga;
    h[first + i] = fmaxf(ha, kMinHess);
  }
}

// ------------------------------------------------------------------ metric
__global__ __launch_bounds__(kTile) void rank_ndcg_kernel(const float* __restrict__ score,
                                                          const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ group_ptr, int64_t N,
                                                          const float* __restrict__ dtab, int dlen, int k,
                                                          double* __restrict__ dcg) {
  __shared__ float sh[kChunk];
  __shared__ double red[kTile / kWave];
  const int q = blockIdx.x;
  const int first = group_ptr[q];
  const int n = group_ptr[q + 1] - first;
  double acc = 0.0;  // lane 0's
  if (first >= 0 && n >= 1 && static_cast<int64_t>(first) + n <= N) {
    for (int i0 = 0; i0 < n; i0 += kTile) {
      const int i = i0 + threadIdx.x;
      const bool valid = i < n;
      const float si = valid ? score[first + i] : 0.f;
      const int pos = tile_positions(score + first, n, i, si, sh);
      double term = 0.0;
      if (valid && (k <= 0 || pos < k))
        term = static_cast<double>(rank_gain(label[first + i])) * static_cast<double>(dtab[min(pos, dlen - 1)]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);  // (not wave_sum: it compiles to other code here)
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = term;
      __syncthreads();
      if (threadIdx.x == 0) acc += (red[0] + red[1]) + (red[2] + red[3]);
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) dcg[q] = acc;
}

}  // namespace

hipError_t gbdt_rank_grad_hess(const float* score, const int32_t* label, int64_t N, const int32_t* plan_wave,
                               int wave_slots, const int32_t* plan_block, int block_items, const float* dtab, int dlen,
                               float* disc, bool ndcg, float* g, float* h, hipStream_t s) {
  const int4* pw = reinterpret_cast<const int4*>(plan_wave);
  const int4* pb = reinterpret_cast<const int4*>(plan_block);
  if (wave_slots > 0) {
    const int grid = (wave_slots + 3) / 4;
    if (ndcg)
      hipLaunchKernelGGL(rank_wave_kernel<true>, dim3(grid), dim3(256), 0, s, score, label, pw, wave_slots, N, dtab,
                         dlen, disc, g, h);
    else
      hipLaunchKernelGGL(rank_wave_kernel<false>, dim3(grid), dim3(256), 0, s, score, label, pw, wave_slots, N, dtab,
                         dlen, disc, g, h);
    RETURN_IF_HIP_ERR(hipGetLastError());
  }
  if (block_items > 0) {
    if (ndcg) {
      hipLaunchKernelGGL(rank_positions_kernel, dim3(block_items), dim3(kTile), 0, s, score, pb, N, dtab, dlen, disc);
      RETURN_IF_HIP_ERR(hipGetLastError());
      hipLaunchKernelGGL(lambda_pairs_kernel<true>, dim3(block_items), dim3(kTile), 0, s, score, label, pb, N, disc, g,
                         h);
    } else {
      hipLaunchKernelGGL(lambda_pairs_kernel<false>, dim3(block_items), dim3(kTile), 0, s, score, label, pb, N, disc,
                         g, h);
    }
    RETURN_IF_HIP_ERR(hipGetLastError());
  }
  return hipSuccess;
}

hipError_t gbdt_rank_ndcg(const float* score, const int32_t* label, int64_t N, const int32_t* group_ptr, int Q,
                          const float* dtab, int dlen, int k, double* dcg, hipStream_t s) {
  if (Q <= 0) return hipSuccess;
  hipLaunchKernelGGL(rank_ndcg_kernel, dim3(Q), dim3(kTile), 0, s, score, label, group_ptr, N, dtab, dlen, k, dcg);
  return hipGetLastError();
}

int gbdt_rank_wave_max() { return kWave; }
int gbdt_rank_tile_rows() { return kTile; }
int gbdt_rank_chunk_rows() { return kChunk; }

}  // namespace kdl
