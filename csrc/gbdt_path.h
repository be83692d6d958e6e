// What a kernel over a root-to-leaf path table needs (the slot format of csrc/gbdt_shap.hip's
// header): the format's limits, the Gauss-Legendre rules, the row-tile staging, a path element's
// interval test and the block size by LDS budget.  csrc/gbdt_interactions.hip is built on it.
// csrc/gbdt_shap.hip still carries its own copies of the same definitions: moved onto this header
// its contribution kernel measured 0.5 % slower (71.97 against 71.57 ms, alternating builds), so
// that file is left as it was until someone finds out why.
// Device helpers are force-inlined and the constant tables are per translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace kdl {
namespace gbdt_path {

constexpr int kChunkSlots = 512;  // 16-byte path slots per LDS chunk
constexpr int kMaxPath = 10;      // merged elements per path (the grower's depth limit)
constexpr int kLdsMax = 160 * 1024;

// Gauss-Legendre on [0, 1], rules of 1..5 nodes, row Q - 1: node t, 1 - t, weight
static __constant__ float kGlT[5][5] = {
    {0.5f},
    {0.21132486540518713f, 0.7886751345948129f},
    {0.1127016653792583f, 0.5f, 0.8872983346207417f},
    {0.06943184420297371f, 0.33000947820757187f, 0.6699905217924281f, 0.9305681557970262f},
    {0.04691007703066802f, 0.23076534494715845f, 0.5f, 0.7692346550528415f, 0.9530899229693319f}};
static __constant__ float kGlU[5][5] = {
    {0.5f},
    {0.7886751345948129f, 0.21132486540518713f},
    {0.8872983346207417f, 0.5f, 0.1127016653792583f},
    {0.9305681557970262f, 0.6699905217924281f, 0.33000947820757187f, 0.06943184420297371f},
    {0.9530899229693319f, 0.7692346550528415f, 0.5f, 0.23076534494715845f, 0.04691007703066802f}};
static __constant__ float kGlW[5][5] = {
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

// element slot { feature | has_left << 30, lo bits, hi bits, z bits }: the feature
__device__ __forceinline__ int elem_feature(const int4& e) { return e.x & 0x3fffffff; }

// the element's interval test on the row's value: ``!(x <= lo)`` and, with a left turn, ``x <= hi``
// (NaN fails every left and passes every right condition; lo = NaN: no right turn)
__device__ __forceinline__ bool elem_inside(const int4& e, float xv) {
  const bool has_left = (e.x >> 30) & 1;
  return !(xv <= __int_as_float(e.y)) && (!has_left || xv <= __int_as_float(e.z));
}

// (1 - z) of element j from the path's trailing slots, four per slot
__device__ __forceinline__ float elem_one_minus_z(const int4& r, int j) {
  return __int_as_float(j % 4 == 0 ? r.x : j % 4 == 1 ? r.y : j % 4 == 2 ? r.z : r.w);
}

// the R of 256 / 128 / 64 with the most waves per CU for ``fixed + R * per_row`` bytes of LDS
// (ties: the larger R); 0: not even 64 rows fit
inline int pick_rows(size_t fixed, size_t per_row) {
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

}  // namespace gbdt_path
}  // namespace kdl
