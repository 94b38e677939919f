// Wave-wide (wave64) reductions and scans shared by the device code of several translation units.
#pragma once
#include <hip/hip_runtime.h>

namespace tacex {

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Wave-wide inclusive scans on the VALU (DPP row shifts / broadcasts, no LDS round trips like ds_bpermute): lane 63 ends up
// with the reduction over the wave.  Sequence of LLVM's AMDGPU atomic optimizer for wave64 on gfx9.
#define TACEX_DPP_SCAN(v, IDENT, OP, T_AS_INT, INT_AS_T)                                                              \
  do {                                                                                                                \
    v = OP(v, INT_AS_T(__builtin_amdgcn_update_dpp(T_AS_INT(IDENT), T_AS_INT(v), 0x111, 0xf, 0xf, false)));           \
    v = OP(v, INT_AS_T(__builtin_amdgcn_update_dpp(T_AS_INT(IDENT), T_AS_INT(v), 0x112, 0xf, 0xf, false)));           \
    v = OP(v, INT_AS_T(__builtin_amdgcn_update_dpp(T_AS_INT(IDENT), T_AS_INT(v), 0x114, 0xf, 0xf, false)));           \
    v = OP(v, INT_AS_T(__builtin_amdgcn_update_dpp(T_AS_INT(IDENT), T_AS_INT(v), 0x118, 0xf, 0xf, false)));           \
    v = OP(v, INT_AS_T(__builtin_amdgcn_update_dpp(T_AS_INT(IDENT), T_AS_INT(v), 0x142, 0xa, 0xf, false)));           \
    v = OP(v, INT_AS_T(__builtin_amdgcn_update_dpp(T_AS_INT(IDENT), T_AS_INT(v), 0x143, 0xc, 0xf, false)));           \
  } while (0)
__device__ __forceinline__ int dpp_id_int(int x) { return x; }
__device__ __forceinline__ int dpp_add_int(int a, int b) { return a + b; }
__device__ __forceinline__ int wave_scan_add_lane63(int v) {
  TACEX_DPP_SCAN(v, 0, dpp_add_int, dpp_id_int, dpp_id_int);
  return v;
}
__device__ __forceinline__ float wave_scan_min_lane63(float v) {
  TACEX_DPP_SCAN(v, INFINITY, fminf, __float_as_int, __int_as_float);
  return v;
}
__device__ __forceinline__ float wave_scan_max_lane63(float v) {
  TACEX_DPP_SCAN(v, -INFINITY, fmaxf, __float_as_int, __int_as_float);
  return v;
}

}  // namespace tacex
