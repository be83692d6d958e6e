// MFMA operand types and fragment reads shared by the bf16 MFMA kernels
// (v_mfma_f32_32x32x16_bf16: 8 bf16 per lane per operand, 16 fp32 accumulators
// per lane).
#pragma once

#include <hip/hip_runtime.h>

namespace kdl {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s_t lds_v4s_t;

// ds_read_b64_tr_b16 of the LDS address p: per 16-lane group a 4-row x
// 16-column block of bf16, lane i gets column i's 4 rows -- the operand layout
// of an MFMA whose reduction index is the LDS row.  Device pass only: the host
// pass has no such builtin, and a reference to it there makes clang drop the
// kernel's host stub.
__device__ __forceinline__ v4s_t tr_read(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(p));
#else
  return v4s_t{};
#endif
}

// two transposed reads (rows k..k+3 and k+4..k+7) = one lane's 8-deep K run
__device__ __forceinline__ bf16x8_t frag8(v4s_t lo, v4s_t hi) {
  const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
  return __builtin_bit_cast(bf16x8_t, make_uint4(a.x, a.y, b.x, b.y));
}

}  // namespace kdl
