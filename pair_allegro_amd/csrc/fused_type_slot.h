// Model type -> the type a fused kernel sees, applied by the writers of fused-side types and by nothing else: k_pack_xt (edges.hip: AtomXT.mt, from which the
// single-pass edge build takes the packed edge types and the centre records), k_centre_info / k_pack_small and k_edge_types (fused_common.h: the same behind the
// stand-alone packing kernels and the two-pass edge build).
#pragma once
#include <hip/hip_runtime.h>

namespace ahip {
// The type itself, or under a subset of active types (engine.h: Model::active) its compact slot from the byte table `slot` (a wave-uniform pointer; null = no
// subset, and the code executed is the code without one).  An inactive type (0xFF) takes slot 0, so every later index stays in range, and leaves 1 + the model
// type in the host-mapped word `bad` (engine.h: inactive_word), which the host reports like the f16x2 alarm word beside it.
__device__ __forceinline__ int fused_type_slot(const unsigned char *__restrict__ slot, int mt, int *bad) {
  if (!slot) return mt;
  const int s = slot[mt];
  if (s == 0xFF) { *bad = mt + 1; return 0; }
  return s;
}
}  // namespace ahip
