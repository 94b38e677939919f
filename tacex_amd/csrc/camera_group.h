// The sensor camera model's arithmetic on ONE group of four consecutive pixels: the Philox draws, the colour response, the fixed
// pattern, read + shot noise, the clamps and the 8-bit packing, with the stores of a finished group.  ONE copy, included by
// camera_model.hip (tacex_camera_model) and lens_model.hip (tacex_lens_camera_model gathers a group through the lens and hands it
// here in the same launch).  The contract is the comment of tacex_camera_model in include/tacex_hip.h; both translation units are
// compiled with -ffp-contract=off, so every product and sum below rounds on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "tacex_philox.h"

namespace tacex {

// sum of the four bytes of a word (0..1020)
TACEX_HD inline int32_t camera_byte_sum(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int32_t)__builtin_amdgcn_sad_u8(w, 0u, 0u);  // v_sad_u8: sum of |byte - 0| in one instruction
#else
  return (int32_t)((w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24));
#endif
}

// The 12 integer draws of one 4-pixel group: sample j = 3 p + c takes word j % 4 of the Philox call with counter
// (group, j / 4 [+ 4 for the fixed pattern], frame, call [0 for the fixed pattern]); d = byte sum - 510 (mean 0, variance 21845).
TACEX_HD inline void camera_noise_draw(uint32_t key0, uint32_t key1, uint32_t frame, uint32_t call, uint32_t group, bool fixed_pattern,
                                       int32_t out[12]) {
  const uint32_t key[2] = {key0, key1};
#pragma unroll
  for (uint32_t q = 0; q < 3; ++q) {
    const uint32_t ctr[4] = {group, fixed_pattern ? 4u + q : q, frame, fixed_pattern ? 0u : call};
    uint32_t r[4];
    philox4x32_10(ctr, key, r);
#pragma unroll
    for (int w = 0; w < 4; ++w) out[4 * q + w] = camera_byte_sum(r[w]) - 510;
  }
}

// what a launch knows of the camera: the profile table and the address of the draws
struct CameraTable {
  const float* profiles;  // (P,16)
  const int32_t* ids;     // (B,) or nullptr
  int num_profiles;
  uint32_t key0, key1, frame_offset, call;
};

struct CameraProfileRow {
  float m[9], o[3], read, shot, fixed;
};

// the row of `frame` (wave-uniform: a workgroup stays inside one frame)
__device__ inline CameraProfileRow load_camera_profile(const CameraTable& t, unsigned int frame) {
  CameraProfileRow p;
  const int id = t.ids ? t.ids[frame] : 0;  // (written out, not stage_row(): profiles/stage_layer_isa.md)
  if (id >= 0 && id < t.num_profiles) {
    const float* __restrict__ row = t.profiles + (size_t)id * 16;
#pragma unroll
    for (int k = 0; k < 9; ++k) p.m[k] = row[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p.o[k] = row[9 + k];
    p.read = row[12]; p.shot = row[13]; p.fixed = row[14];
  } else {  // an id outside [0, P): the identity profile
#pragma unroll
    for (int k = 0; k < 9; ++k) p.m[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    p.o[0] = p.o[1] = p.o[2] = 0.0f;
    p.read = p.shot = p.fixed = 0.0f;
  }
  return p;
}

// one group: px[12] (4 pixels x RGB, in place) -> values in [0, 1]; `frame` is frame_offset + b
__device__ inline void camera_group(const CameraTable& t, const CameraProfileRow& p, uint32_t frame, uint32_t group, float px[12]) {
  const float S = 0x1.bb688cp-8f;  // float32(1 / sqrt(21845.0)) = 0.006765875, bits 0x3bddb446
  int32_t d[12], df[12];
  camera_noise_draw(t.key0, t.key1, frame, t.call, group, false, d);
  const bool fixed = p.fixed != 0.0f;  // uniform over the workgroup
  if (fixed) camera_noise_draw(t.key0, t.key1, frame, 0u, group, true, df);
  const float fs = p.fixed * S, rr = p.read * p.read;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float r = px[3 * q], g = px[3 * q + 1], b = px[3 * q + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = ((p.m[3 * c] * r + p.m[3 * c + 1] * g) + p.m[3 * c + 2] * b) + p.o[c];
      if (fixed) v = v * (1.0f + fs * (float)df[3 * q + c]);
      v = fminf(fmaxf(v, 0.0f), 1.0f);
      const float sig = sqrtf(rr + p.shot * v);
      v = v + (sig * S) * (float)d[3 * q + c];
      px[3 * q + c] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
  }
}

__device__ inline uint32_t camera_u8(float v) { return (uint32_t)floorf(255.0f * v + 0.5f); }  // v in [0, 1] -> 0..255

// Stores of a whole group whose first value is value v0 of the batch (v0 % 4 == 0 and `out` 16-byte aligned): three 16-byte
// stores (float32), or one 12-byte store of the packed bytes (uint8): a wave writes 3072 / 768 contiguous bytes.
template <bool kU8>
__device__ inline void store_group_vec(void* out, size_t v0, const float px[12]) {
  if constexpr (kU8) {
    struct alignas(4) Bytes12 { uint32_t x, y, z; };  // one global_store_dwordx3
    uint32_t w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      w[i] = camera_u8(px[4 * i]) | (camera_u8(px[4 * i + 1]) << 8) | (camera_u8(px[4 * i + 2]) << 16) | (camera_u8(px[4 * i + 3]) << 24);
    *reinterpret_cast<Bytes12*>(static_cast<uint8_t*>(out) + v0) = Bytes12{w[0], w[1], w[2]};
  } else {
    float4* dst = reinterpret_cast<float4*>(static_cast<float*>(out) + v0);
#pragma unroll
    for (int i = 0; i < 3; ++i) dst[i] = make_float4(px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3]);
  }
}

// Stores of the first n (<= 12) values of a group, any alignment: dword / byte stores.
template <bool kU8>
__device__ inline void store_group_scalar(void* out, size_t v0, const float px[12], int n) {
  if constexpr (kU8) {
    uint8_t* dst = static_cast<uint8_t*>(out) + v0;
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < n) dst[i] = (uint8_t)camera_u8(px[i]);
  } else {
    float* dst = static_cast<float*>(out) + v0;
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < n) dst[i] = px[i];
  }
}

}  // namespace tacex
