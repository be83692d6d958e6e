// Device-side read of a forest node, shared by the kernels that walk trees
// (csrc/gbdt_predict.hip, csrc/gbdt_shap.hip).  GbdtNode itself is declared in
// kdl_api.h, which the host-only bindings read too.
#pragma once

#include <hip/hip_runtime.h>

#include "kdl_api.h"

namespace kdl {

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

}  // namespace kdl
