// wr_jit.h — nam_wn_reg_kernel compiled for one model's own layer shapes, at load time, with an on-disk cache.
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>

#include "plan.h"

namespace namhip
{

// Compiles kernel_wn_reg.hip with `shapes` as its shape tables (WrShapeSet::header_text) into a gfx950 code object —
// or finds the one a previous load of the same shapes (by any process) left in the cache. Host-only: needs hipcc and the
// kernel sources, not a GPU. Returns the code object's path; "" on failure with the reason in `why`.
//   sources:  $NAM_HIP_JIT_SRC, else <directory of libnam_hip.so>/../csrc (the in-tree layout)
//   compiler: $NAM_HIP_HIPCC, else /opt/rocm/bin/hipcc
//   cache:    $NAM_HIP_JIT_CACHE, else <directory of libnam_hip.so>/jit (in-tree: travels with the library), else
//             /tmp/nam_hip_jit_<uid>
//   NAM_HIP_JIT=0 switches the per-model compile off (models outside the ahead-of-time shapes then run the
//   run-time-flag instantiations or the op interpreter).
std::string wr_jit_build(const WrShapeSet& shapes, std::string& why);
bool wr_jit_enabled();

// The functions (hipFunction_t) of a per-model code object on a device: hipModuleLoad is per device, so they are loaded once per
// path and device and kept for the life of the process (a handful of entries).
// The dense forms are the ones built for two wavefronts per SIMD (kernel_wn_reg.hip: nam_wn_reg_jit2d / 4d); nullptr = not usable:
// the code object has none, the compiler did not fit it into 256 registers WITHOUT scratch, or NAM_HIP_WR_DENSE=0.
struct WrJitFunctions
{
  int rc = 0; // NAM_HIP_OK, or the code of the failed load (its text: nam_hip_last_error); the functions are null then
  hipFunction_t fn = nullptr, fn2 = nullptr, fn4 = nullptr; // nam_wn_reg_jit, nam_wn_reg_jit2 (two stages), nam_wn_reg_jit4
  hipFunction_t fn2d = nullptr, fn4d = nullptr; // the dense forms
  int dense_forms() const { return (fn2d ? 2 : 0) | (fn4d ? 4 : 0); } // (launch_policy.h: WrShapeQuery::dense_forms)
  hipFunction_t pick(int stages, bool dense) const { return stages == 4 ? (dense && fn4d ? fn4d : fn4) : stages == 2 ? (dense && fn2d ? fn2d : fn2) : fn; }
};
WrJitFunctions wr_jit_functions(const std::string& path, int device);

} // namespace namhip
