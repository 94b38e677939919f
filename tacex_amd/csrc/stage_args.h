// What the per-env stages of the optical path and the library height-map sources share on the C side (camera_model.hip,
// lens_model.hip, contact_field.hip, gel_memory.hip, relief_source.hip, volume_source.hip, sdf_scene.hip): the refusals every entry point opens with, the launch geometry of "blocks stay inside one frame", and the
// lookup of a frame's row in a profile table.  No arithmetic lives here: the four units are pinned bit for bit on their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_rows.h"
#include "tacex_internal.h"

namespace tacex {

// Refusals (set_error, the caller returns 2): true when the argument is refused.  Chained with || in the order of the checks:
//   if (null_arg(fn, "rgb_dev", rgb_dev) || not_positive(fn, "num_frames", num_frames)) return 2;
inline bool null_arg(const char* fn, const char* name, const void* p) {
  if (p) return false;
  set_error("%s: null %s", fn, name);
  return true;
}
inline bool not_positive(const char* fn, const char* name, int v) {
  if (v > 0) return false;
  set_error("%s: %s = %d", fn, name, v);
  return true;
}

// The height-map sources whose frame outputs come from the row kernel's statements (relief_source.hip, volume_source.hip, sdf_scene.hip): a frame
// of whole float4 groups whose row and column minima fit LDS, and a map that float4 stores may write.
inline bool not_frame_rows_geometry(const char* fn, int height, int width) {
  if (width % 4 != 0) { set_error("%s: width = %d (must be a multiple of 4)", fn, width); return true; }
  if (height <= kFrameRowsMaxH && width <= kFrameRowsMaxH) return false;
  set_error("%s: height x width = %d x %d (at most %d each)", fn, height, width, kFrameRowsMaxH);
  return true;
}
inline bool not_aligned16(const char* fn, const char* name, const void* p) {
  if ((uintptr_t)p % 16 == 0) return false;
  set_error("%s: %s must be 16-byte aligned", fn, name);
  return true;
}

// A launch whose workgroups each stay inside ONE frame (the frame's id and row are then wave-uniform): `items` per frame over
// blocks of `block` threads, the frames side by side in grid.x.
struct FrameLaunch {
  unsigned int blocks_per_frame, grid;
};
// false when `counted` (the per-frame count the kernel indexes with 32 bits) or the grid does not fit 2^31 - 1
inline bool frame_launch(long long items, long long counted, int block, int num_frames, FrameLaunch* g) {
  const long long bpf = (items + block - 1) / block;
  if (counted > 0x7fffffffll || bpf * num_frames > 0x7fffffffll) return false;
  g->blocks_per_frame = (unsigned int)bpf;
  g->grid = (unsigned int)(bpf * num_frames);
  return true;
}
inline int refuse_image_launch(const char* fn, int num_frames, int height, int width) {
  set_error("%s: num_frames x height x width = %d x %d x %d exceeds one launch", fn, num_frames, height, width);
  return 2;
}
inline int refuse_points_launch(const char* fn, int num_frames, int num_points) {
  set_error("%s: num_frames x num_points = %d x %d exceeds one launch", fn, num_frames, num_points);
  return 2;
}

// The row of `frame` in a (num_rows, width) table: ids (B,) or nullptr (row 0); nullptr for an id outside [0, num_rows) - the
// caller's default profile (identity, all zero, "nothing in contact").  `table` is never null (the entry points refuse that), and
// saying so keeps "is there a row" the test of the id alone; `frame` indexes with the caller's own integer type.  With both, a
// kernel compiles to the instructions it had with the lookup written out, but for the polarity of that one wave-uniform test.
// contact_field.hip and gel_memory.hip use it; load_camera_profile (camera_group.h) and load_lens_row (lens_model.hip) keep the
// lookup written out, because the other polarity moved the schedule of the fused lens + camera kernel and one of its timings
// (profiles/stage_layer_isa.md).
template <class Index>
__device__ inline const float* stage_row(const float* table, const int32_t* ids, int num_rows, int width, Index frame) {
  __builtin_assume(table != nullptr);
  const int id = ids ? ids[frame] : 0;
  return (id >= 0 && id < num_rows) ? table + (size_t)id * width : nullptr;
}

}  // namespace tacex
