// CTR (XDLJob) evaluation kernels for gfx950: a streaming, mergeable,
// bit-reproducible AUC.
//
// State: hist int64 [2, 65536] (row 0 negatives, row 1 positives) + invalid
// int64 [1].  A row's bucket is the top 16 bits of the ORDERED bit pattern of
// its fp32 logit (-0 -> +0; sign set: ~b, else b | 0x80000000), a
// non-decreasing function of the logit, so the tie-aware Mann-Whitney count
// over the buckets differs from the exact one only on pairs sharing a bucket.
// Every value is an integer sum: independent of arrival order, no float atomics.
//
// auc_accumulate: one global atomic per row is the slow shape (every adder on a
//   few hot lines), so each block first counts its rows in a block-private LDS
//   histogram over the two hot key windows -- exponent fields 112..131 of each
//   sign (2^-15 <= |x| < 32): 2 x 2560 buckets, one 32-bit word per bucket
//   packing the negative count (low 16 bits) and the positive count (high 16);
//   a block takes at most kAucMaxRows < 65536 rows, so neither half overflows --
//   then adds only the non-zero entries to global memory (consecutive lanes,
//   consecutive int64 words).  Rows outside the windows (zeros, denormals, tiny
//   values, |x| >= 32, infinities) add directly; NaN logits count in `invalid`.
// auc_finalize: one block; thread t owns buckets [64 t, 64 t + 64): a block-wide
//   exclusive suffix scan of its positive sums, then
//   U2 = sum_b neg[b] * (2 * sum_{c > b} pos[c] + pos[b]) walking its buckets
//   downwards, and a 64-bit block reduction of (U2, P, N).
//
// The launchers enqueue kernels only (no memset / memcpy: csrc/ctr.hip's rule).
#include "common.h"
#include "kdl_api.h"

namespace kdl {
namespace {

constexpr int kAucBuckets = 65536;
constexpr int kAucExpLo = 112, kAucExpN = 20;          // exponent fields 112..131
constexpr int kAucWin = kAucExpN * 128;                // 2560 buckets per sign
constexpr int kAucNegKey0 = 0x7fff - ((kAucExpLo + kAucExpN) * 128 - 1);  // 15872
constexpr int kAucPosKey0 = 0x8000 + kAucExpLo * 128;                      // 47104
constexpr int kAucThreads = 1024;
constexpr int kAucMinRows = 4 * kAucThreads;           // one float4 round of the block
constexpr int kAucMaxRows = 63 * kAucThreads;          // 64512 < 65536: the packed halves cannot overflow
constexpr int kAucBlocks = 256;                        // one block per CU when n allows

typedef unsigned long long u64;

__device__ __forceinline__ void auc_row(float x, float y, unsigned* __restrict__ lds, u64* __restrict__ hist) {
  if (x != x) {
    atomicAdd(&lds[2 * kAucWin], 1u);
    return;
  }
  unsigned b = __float_as_uint(x);
  if (x == 0.f) b = 0u;  // -0 ties with +0
  const unsigned neg_sign = b >> 31;
  const unsigned key = (neg_sign ? ~b : (b | 0x80000000u)) >> 16;
  const unsigned pos = y > 0.5f ? 1u : 0u;
  const unsigned e = (b >> 23) & 0xffu;
  if (e - static_cast<unsigned>(kAucExpLo) < static_cast<unsigned>(kAucExpN)) {
    // key in [15872, 18431] (negative logits) or [47104, 49663] (positive)
    const unsigned li = neg_sign ? key - kAucNegKey0 : key - kAucPosKey0 + kAucWin;
    atomicAdd(&lds[li], pos ? 0x10000u : 1u);
  } else {
    atomicAdd(&hist[pos * kAucBuckets + key], static_cast<u64>(1));
  }
}

__global__ __launch_bounds__(kAucThreads) void auc_accumulate_kernel(
    const float* __restrict__ logit, const float* __restrict__ y, int64_t n, int64_t rows_per_block, bool vec4,
    u64* __restrict__ hist, u64* __restrict__ invalid) {
  __shared__ unsigned lds[2 * kAucWin + 1];
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * kAucWin + 1; i += kAucThreads) lds[i] = 0u;
  __syncthreads();
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > n) r1 = n;
  if (vec4) {  // rows_per_block % 4 == 0 and both bases 16-byte aligned
    const int64_t full = r0 + (r1 - r0) / 4 * 4;
    for (int64_t i = r0 + 4 * tid; i < full; i += 4 * kAucThreads) {
      const float4 xv = *reinterpret_cast<const float4*>(logit + i);
      const float4 yv = *reinterpret_cast<const float4*>(y + i);
      auc_row(xv.x, yv.x, lds, hist);
      auc_row(xv.y, yv.y, lds, hist);
      auc_row(xv.z, yv.z, lds, hist);
      auc_row(xv.w, yv.w, lds, hist);
    }
    for (int64_t i = full + tid; i < r1; i += kAucThreads) auc_row(logit[i], y[i], lds, hist);
  } else {
    for (int64_t i = r0 + tid; i < r1; i += kAucThreads) auc_row(logit[i], y[i], lds, hist);
  }
  __syncthreads();
  for (int i = tid; i < 2 * kAucWin; i += kAucThreads) {
    const unsigned v = lds[i];
    if (v == 0u) continue;
    const int key = i < kAucWin ? i + kAucNegKey0 : i - kAucWin + kAucPosKey0;
    if (v & 0xffffu) atomicAdd(&hist[key], static_cast<u64>(v & 0xffffu));
    if (v >> 16) atomicAdd(&hist[kAucBuckets + key], static_cast<u64>(v >> 16));
  }
  if (tid == 0 && lds[2 * kAucWin] != 0u) atomicAdd(invalid, static_cast<u64>(lds[2 * kAucWin]));
}

constexpr int kFinPerThread = kAucBuckets / kAucThreads;  // 64 buckets per thread
constexpr int kFinWaves = kAucThreads / kWave;

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += static_cast<u64>(__shfl_xor(static_cast<long long>(v), o, 64));
  return v;
}

// unsigned arithmetic throughout: P, N < 2^31 (the caller's precondition) keeps
// every term and the total below 2 P N < 2^63; past it the sums wrap instead
// of being undefined
__global__ __launch_bounds__(kAucThreads) void auc_finalize_kernel(const u64* __restrict__ hist,
                                                                   u64* __restrict__ out) {
  __shared__ u64 wtot[kFinWaves];
  __shared__ u64 red[3][kFinWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const u64* neg = hist + static_cast<int64_t>(tid) * kFinPerThread;
  const u64* pos = neg + kAucBuckets;
  // one pass over the thread's buckets, downwards: u2 counts against the
  // positives of its OWN higher buckets; the positives of higher threads
  // (`above`, known after the scan) add 2 * above * n_sum
  u64 p_sum = 0, n_sum = 0, u2 = 0;
  for (int j = kFinPerThread - 2; j >= 0; j -= 2) {
    const ulonglong2 pv = *reinterpret_cast<const ulonglong2*>(pos + j);
    const ulonglong2 nv = *reinterpret_cast<const ulonglong2*>(neg + j);
    u2 += nv.y * (2 * p_sum + pv.y);
    p_sum += pv.y;
    u2 += nv.x * (2 * p_sum + pv.x);
    p_sum += pv.x;
    n_sum += nv.x + nv.y;
  }
  // inclusive suffix scan of p_sum inside the wave, then across the waves
  u64 s = p_sum;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const u64 v = static_cast<u64>(__shfl_down(static_cast<long long>(s), o, 64));
    if (lane + o < kWave) s += v;
  }
  if (lane == 0) wtot[wave] = s;
  __syncthreads();
  u64 above = s - p_sum;  // positives in the buckets of higher threads
  for (int w = wave + 1; w < kFinWaves; ++w) above += wtot[w];
  u2 += 2 * above * n_sum;
  u2 = wave_sum_u64(u2);
  p_sum = wave_sum_u64(p_sum);
  n_sum = wave_sum_u64(n_sum);
  if (lane == 0) {
    red[0][wave] = u2;
    red[1][wave] = p_sum;
    red[2][wave] = n_sum;
  }
  __syncthreads();
  if (tid < 3) {
    u64 a = 0;
    for (int w = 0; w < kFinWaves; ++w) a += red[tid][w];
    out[tid] = a;
  }
}

}  // namespace

int64_t auc_rows_per_block(int64_t n) {
  int64_t r = ((n + kAucBlocks - 1) / kAucBlocks + 3) / 4 * 4;
  if (r < kAucMinRows) r = kAucMinRows;
  if (r > kAucMaxRows) r = kAucMaxRows;
  return r;
}

hipError_t auc_accumulate(const float* logit, const float* y, int64_t n, int64_t* hist, int64_t* invalid,
                          hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t rpb = auc_rows_per_block(n);
  const int64_t grid = (n + rpb - 1) / rpb;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  const bool vec4 = (reinterpret_cast<uintptr_t>(logit) % 16 == 0) && (reinterpret_cast<uintptr_t>(y) % 16 == 0);
  hipLaunchKernelGGL(auc_accumulate_kernel, dim3(static_cast<unsigned>(grid)), dim3(kAucThreads), 0, s, logit, y, n,
                     rpb, vec4, reinterpret_cast<u64*>(hist), reinterpret_cast<u64*>(invalid));
  return hipGetLastError();
}

hipError_t auc_finalize(const int64_t* hist, int64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(auc_finalize_kernel, dim3(1), dim3(kAucThreads), 0, s, reinterpret_cast<const u64*>(hist),
                     reinterpret_cast<u64*>(out));
  return hipGetLastError();
}

}  // namespace kdl
