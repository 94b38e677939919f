/*
 * tacex_hip.h - C ABI of libtacex_hip.so, the MI355X (gfx950) implementation of the TacEx tactile hot path.
 *
 * The reference (DH-Ng/TacEx) has no FFI: its hot path is PyTorch code behind the Python plugin classes
 * GelSightSimulator / GelSightSensor.  This header is the boundary the build introduces UNDER those
 * classes; each entry point names the reference code it replaces.  Short names:
 *   TT = source/tacex/tacex/simulation_approaches/gpu_taxim/sim/taxim_torch.py
 *   TS = source/tacex/tacex/simulation_approaches/gpu_taxim/taxim_sim.py
 *   GS = source/tacex/tacex/gelsight_sensor.py
 *   MM = source/tacex/tacex/simulation_approaches/fots/sim/marker_motion.py
 *   FS = source/tacex/tacex/simulation_approaches/fots/fots_marker_sim.py
 *   US/UO/UA = source/tacex_uipc/tacex_uipc/{sim/uipc_sim.py,objects/uipc_object.py,sim/uipc_attachments.py}
 *   VT = source/tacex/tacex/simulation_approaches/fem_based/sim/tactile_sensor_sapienipc_modified.py
 *
 * Conventions
 *   - plain C types only; every `*_dev` pointer is DEVICE memory owned by the caller (PyTorch, usually);
 *   - no allocation, no synchronisation inside a compute call: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream);
 *   - one context per device, not thread-safe per context;
 *   - every function returns 0 on success, non-zero on error; tacex_last_error() gives the message
 *     (the Python layer turns it into RuntimeError / ValueError like the reference's exceptions);
 *   - images are row-major float32, batch first: height maps (B,H,W) in millimetres, RGB (B,H,W,3).
 */
#ifndef TACEX_HIP_H
#define TACEX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TACEX_MAX_LEVELS 8
#define TACEX_ABI_VERSION 20

typedef struct tacex_taxim_ctx tacex_taxim_ctx;
typedef struct tacex_fots_ctx tacex_fots_ctx;
typedef struct tacex_fem_ctx tacex_fem_ctx;

const char* tacex_last_error(void);
int tacex_abi_version(void);
/* Number of HIP devices visible / name of the gcn arch of `device_id` (for loud failure messages). */
int tacex_device_count(int* count);
int tacex_device_arch(int device_id, char* buf, size_t buflen);

/* ---------------------------------------------------------------------------------------------
 * Taxim optical path.  Tables are HOST pointers, copied to the device once at creation
 * (replaces TaximTorch.__init__, TT:50-130, and the lru-cached tables TT:136-164).
 * ------------------------------------------------------------------------------------------- */
typedef struct tacex_taxim_params {
  int32_t height, width;        /* tactile image size H, W (TS:49-54 tactile_img_res = (W,H)) */
  int32_t calib_height, calib_width; /* calibration size (params.json sensor.h / sensor.w: 480, 640) */
  float pixmm;                  /* params.json sensor.pixmm (0.0295) */
  int32_t num_bins;             /* params.json sensor.num_bins (125) */
  float contact_scale;          /* params.json simulator.contact_scale (0.4), TT:459 */
  int32_t n_levels;             /* pyramid levels + 1 final blur (7), TT:464-471 */
  int32_t ksize_w[TACEX_MAX_LEVELS]; /* odd kernel widths  per level, TT:396-403 */
  int32_t ksize_h[TACEX_MAX_LEVELS]; /* odd kernel heights per level */
  const float* taps_w[TACEX_MAX_LEVELS]; /* normalised float32 taps, ksize_w[l] each, TT:362-366 */
  const float* taps_h[TACEX_MAX_LEVELS];
  const float* poly;            /* (3, num_bins, num_bins, 6) float32 = stack(grad_b,grad_g,grad_r)/255, TT:73-80 */
  const float* gel_map;         /* (H, W) float32, mm, max == 0, TT:82-90,159-164 */
  const float* background;      /* (3, H, W) float32 in [0,1], TT:92-94,136-137,414-430 */
  const float* feat_x;          /* (W,) float32: linspace(0, calib_width,  W+1)[:-1], TT:139-157 */
  const float* feat_y;          /* (H,) float32: linspace(0, calib_height, H+1)[:-1] */
} tacex_taxim_params;

int tacex_taxim_create(int device_id, const tacex_taxim_params* params, tacex_taxim_ctx** out);
void tacex_taxim_destroy(tacex_taxim_ctx* ctx);

/* Bytes of caller-provided device scratch tacex_taxim_render / tacex_taxim_deform need for B frames. */
size_t tacex_taxim_workspace_bytes(const tacex_taxim_ctx* ctx, int num_frames);

/* GS:581-593 (_get_height_map) + GS:557-579 (_get_camera_depth) + TS:115-131 (compute_indentation_depth)
 * in one pass over the camera depth image:
 *   hm_mm      = (isinf(depth_m) ? far_clip_m : depth_m) * 1000                       (B,Hc,Wc)
 *   frame_min  = min over the frame of hm_mm                                           (B,)
 *   indent_mm  = d <= gelpad_height ? (gelpad_height - d) * 1000 : 0,
 *                d = max(frame_min/1000 - gelpad_to_camera_min_distance, 0)            (B,)  [nullable]
 *   cam_u8     = uint8(((hm_mm - near_clip_m*1000) / (far_clip_m*1000)) * 255)  (sic)  (B,Hc,Wc) [nullable]
 * The clip range is passed as DOUBLES: the reference multiplies the Python doubles by 1000 and torch rounds the product once
 * to float32 (GS:573-574), so cam_u8 is bit-exact.  depth_m_dev may alias hm_mm_dev.
 *   frame_rows (B,4) int32 [nullable, needs indent_mm]: [0], [1] first / last frame ROW holding a pixel below the press plane,
 *                i.e. with S = (hm - frame_min) - indent < 0 (TT:441) - (height, -1) when there is none; [2], [3] first / last
 *                such COLUMN ((width, -1); (0, width - 1) for widths the pass cannot track).  By-product of the same pass (per-row
 *                and per-column minima); the render uses it to skip pyramid bands and 64-column blocks that cannot be non-zero
 *                (tacex_taxim_set_frame_rows + TACEX_FLAG_HAVE_FRAME_ROWS).  (ABI 10: two ints per frame before.) */
int tacex_height_map_from_depth(const float* depth_m_dev, double near_clip_m, double far_clip_m,
                                float gelpad_height_m, float gelpad_to_camera_min_distance_m,
                                float* hm_mm_dev, float* frame_min_dev, float* indent_mm_dev,
                                uint8_t* cam_u8_dev, int32_t* frame_rows_dev, int num_frames, int height, int width,
                                void* stream);

/* The same pass, handed to the NEXT tacex_taxim_render / _render_obs / _deform call of `ctx` instead of being launched now (ABI 11).
 * A render whose hm_mm / frame_min / press buffers are this pass's hm_mm_dev / frame_min_dev / indent_mm_dev (same frame count,
 * TACEX_FLAG_HAVE_FRAME_MIN, a frame-rows buffer that is this pass's) runs it INSIDE the pass: per chunk of the band levels, on the
 * chunk's own stream, so that one chunk's depth pass (HBM-bound) overlaps the previous chunk's band levels (matrix pipe) - the
 * reference's sequence _get_height_map -> compute_indentation_depth -> optical_simulation (GS:229-263, 581-593) as one launch
 * sequence.  Any other render on the context, or tacex_taxim_flush_deferred, runs the pending pass in full first: the outputs are
 * complete, in stream order, no later than the end of the next call on the context.  Frame size = the context's.  At most one
 * pending pass per context (a second call fails). */
int tacex_taxim_defer_height_map_from_depth(tacex_taxim_ctx* ctx, const float* depth_m_dev, double near_clip_m, double far_clip_m,
                                            float gelpad_height_m, float gelpad_to_camera_min_distance_m,
                                            float* hm_mm_dev, float* frame_min_dev, float* indent_mm_dev,
                                            uint8_t* cam_u8_dev, int32_t* frame_rows_dev, int num_frames);
/* Runs a pending deferred pass now (no-op without one). */
int tacex_taxim_flush_deferred(tacex_taxim_ctx* ctx, void* stream);

/* Height-map SOURCE: rasterise one analytic indenter per env into the height map (mm), with the per-frame
 * minimum and the indentation depth of TS:115-131 in the same pass.  Stands in for the TiledCamera depth render
 * (GS:229-263 -> _get_height_map GS:581-593) when the contact geometry is a primitive; 4 B/px written, nothing read.
 * indenters_dev (B, 8) f32: [kind, cx_px, cy_px, r_px, angle_rad, press_mm, cx2_px, cy2_px]
 *   kind 0 sphere, 1 lying cylinder (radius r/2), 2 wedge with 45 degree flanks, 3 two spheres, < 0 no contact.
 * depth = min(gel_top_mm - press_mm + profile(x, y), far_clip_mm), profile in mm above the indenter's lowest point. */
int tacex_height_map_from_indenters(const float* indenters_dev, float pixmm, float gel_top_mm, float far_clip_mm,
                                    float gelpad_height_m, float gelpad_to_camera_min_distance_m, float* hm_mm_dev,
                                    float* frame_min_dev, float* indent_mm_dev, int num_frames, int height, int width,
                                    void* stream);

/* Height-map SOURCE for arbitrary rigid indenters: the depth image the IsaacLab TiledCamera of the reference
 * hands _get_height_map (GS:229-263, 581-593 - "distance_to_image_plane" in metres, inf where nothing is seen inside the
 * clipping range), rendered here from one shared triangle mesh and one rigid pose per env.
 *   verts_dev (V,3) f32 object frame [m]; tris_dev (T,3) int32; pos_dev (B,3) f32 translation and quat_dev (B,4) f32 rotation
 *   (wxyz, normalised by the kernel) taking object coordinates into the CAMERA frame (x right, y down, z along the optical axis);
 *   pinhole intrinsics fx, fy, cx, cy in pixels, pixel (i, j) sampled at its centre (j + 0.5, i + 0.5);
 *   bounding_sphere: HOST pointer to {cx, cy, cz, r} of a sphere around the mesh in the object frame, nullable (image tiles
 *   the sphere cannot project onto skip the triangle loop);
 *   depth_m_dev (B,H,W) f32 out.  Feed it to tacex_height_map_from_depth. */
int tacex_depth_from_mesh(const float* verts_dev, const int32_t* tris_dev, int num_verts, int num_tris,
                          const float* pos_dev, const float* quat_dev, float fx, float fy, float cx, float cy,
                          float near_clip_m, float far_clip_m, const float* bounding_sphere, float* depth_m_dev, int num_envs, int height,
                          int width, void* stream);

/* Height-map SOURCE for the FEM gel pad itself (ABI 16): the same depth image, rendered from the DEFORMED surface of the pad - per env
 * vertices straight out of the FEM state, one camera pose per env (the route the reference leaves as a TODO in _get_height_map and
 * otherwise covers by re-rendering the UIPC meshes after every step, uipc_sim.py:268-284).
 *   x_dev (B, num_verts, 3) f64 world positions (UipcSim.x, read in place); surf_ids_dev (Vs,) int32 the rendered vertices, each
 *   < num_verts; tris_dev (T,3) int32 indices into surf_ids_dev, each < Vs (neither is checked on the device);
 *   cam_pos_dev (B,3) f64 and cam_rot_inv_dev (B,3,3) f64 row-major: camera-frame point p_c[i] = (Rinv[i][0] d0 + Rinv[i][1] d1)
 *   + Rinv[i][2] d2 with d = x - cam_pos (VisionTactileSensorUIPC.transform_world_to_camera_frame), in f64, rounded once to f32;
 *   intrinsics, clipping range and depth_m_dev (B,H,W) f32 out as in tacex_depth_from_mesh, whose rasterisation rules and float32
 *   operations this follows exactly from the f32 camera-frame point on.  Surfaces of up to 2048 vertices are projected once per
 *   workgroup into LDS; larger ones per triangle (same image).
 * Returns 2 (no GPU call) on a null buffer, a count <= 0, Vs > num_verts or a clipping range that is not 0 <= near < far. */
int tacex_depth_from_deformed_mesh(const double* x_dev, int num_verts, const int32_t* surf_ids_dev, int num_surf_verts,
                                   const int32_t* tris_dev, int num_tris, const double* cam_pos_dev, const double* cam_rot_inv_dev,
                                   float fx, float fy, float cx, float cy, float near_clip_m, float far_clip_m, float* depth_m_dev,
                                   int num_envs, int height, int width, void* stream);

/* Contact TRACTION of the FEM gel pad as an image in the camera frame: the per-vertex contact force of tacex_fem_contact_forces /
 * tacex_fem_ball_contact_forces (vertex_force_out_dev), divided by the barrier's vertex area and carried through the rasteriser of
 * tacex_depth_from_deformed_mesh - pixel for pixel the image that function renders, so aligned with the height map and the tactile RGB
 * frame it feeds.  Forces act ON the pad: [..., 2] is the normal pressure along the optical axis (negative where an indenter pushes the
 * face towards the camera), [..., 0:2] the shear.
 *   x_dev, num_verts, surf_ids_dev, num_surf_verts, tris_dev, num_tris, cam_pos_dev, cam_rot_inv_dev, intrinsics, clipping range: as in
 *   tacex_depth_from_deformed_mesh (the index tables are not checked on the device);
 *   vertex_force_dev (B, num_verts, 3) f64 world frame [N]; vertex_area_dev (num_verts,) f64 [m^2], one table for all envs
 *   (UipcObject.surface_vertex_areas): vertex traction tw = f / area per component in f64, camera frame
 *   tc[i] = (Rinv[i][0] tw[0] + Rinv[i][1] tw[1]) + Rinv[i][2] tw[2] in f64, rounded once to f32; zero where area <= 0;
 *   fragments are that function's; a pixel takes the fragment with the smallest (bits of z, triangle index) - the index decides between
 *   the equal depths two triangles give at a pixel centre on their shared edge, so the image does not depend on the order the workgroup
 *   happens to list its triangles in - and interpolates perspective-correctly with f32 operations, separately rounded:
 *   w_k = (l_k * iz_k) * z, t[i] = (w_0 t_0[i] + w_1 t_1[i]) + w_2 t_2[i];
 *   traction_dev (B,H,W,3) f32 out [Pa], 0 where no fragment lies inside the clipping range; depth_m_dev (B,H,W) f32 out or NULL:
 *   bit-equal to tacex_depth_from_deformed_mesh on the same arguments.
 *   Vertex tractions of up to 1536 surface vertices are formed once per workgroup in LDS; larger surfaces form them per pixel (same image).
 * Returns 2 (no GPU call) on a null buffer other than depth_m_dev, a count <= 0, Vs > num_verts or a clipping range that is not
 * 0 <= near < far. */
int tacex_traction_image_from_deformed_mesh(const double* x_dev, int num_verts, const int32_t* surf_ids_dev, int num_surf_verts,
                                            const int32_t* tris_dev, int num_tris, const double* vertex_force_dev,
                                            const double* vertex_area_dev, const double* cam_pos_dev, const double* cam_rot_inv_dev,
                                            float fx, float fy, float cx, float cy, float near_clip_m, float far_clip_m,
                                            float* traction_dev, float* depth_m_dev, int num_envs, int height, int width, void* stream);

/* Height-map SOURCE for the affine body that presses into the pad (ball_rolling_uipc.py:71-139): the same depth image, rendered from the
 * body's 12-unknown state - what the sensor camera sees of the object with the gel hidden, the input Taxim is built for
 * (ManiSkill-ViTac gen_rgb_image, tactile_sensor_sapienipc.py:424-457).
 *   rest_verts_dev (num_verts,3) f64 rest vertices X in the body frame, one table for all envs; tris_dev (T,3) int32 indices into it,
 *   each < num_verts (not checked on the device); q_dev (B,4,3) f64 = (p, c1, c2, c3), c_k the columns of A (UipcSim.q, read in place):
 *   world point per component w = ((p + X0 c1) + X1 c2) + X2 c3 in f64, separate multiplies and adds;
 *   cam_pos_dev / cam_rot_inv_dev / intrinsics / clipping range / depth_m_dev (B,H,W) f32 out as in tacex_depth_from_deformed_mesh: from
 *   the world point on it is that function's kernel (one shared body, a second vertex source), so the image is bit-equal to
 *   tacex_depth_from_deformed_mesh on those world points.  Bodies of up to 2048 vertices are projected once per workgroup into LDS.
 *   Image tiles that the part of the body's bounding sphere (radius |A|_2 max|X| about p) inside the clipping range cannot project onto
 *   skip the vertices altogether (no fragment can lie there: same image).
 * Returns 2 (no GPU call) on a null buffer, a count <= 0 or a clipping range that is not 0 <= near < far. */
int tacex_depth_from_affine_body(const double* rest_verts_dev, int num_verts, const int32_t* tris_dev, int num_tris, const double* q_dev,
                                 const double* cam_pos_dev, const double* cam_rot_inv_dev, float fx, float fy, float cx, float cy,
                                 float near_clip_m, float far_clip_m, float* depth_m_dev, int num_envs, int height, int width,
                                 void* stream);

/* Height-map SOURCE from a mesh LIBRARY (ABI 17): the image of tacex_depth_from_mesh, with every env rendering its OWN mesh.
 *   verts_dev (V,3) f32 every mesh's object-frame vertices back to back; tris_dev (T,3) int32 every mesh's triangles back to back,
 *   indexing verts_dev (the concatenated table); mesh_tris_dev (num_meshes,2) int32: first triangle and triangle count of every mesh;
 *   mesh_spheres_dev (num_meshes,4) f32 device, nullable: bounding sphere {cx, cy, cz, r} of every mesh (r < 0: unknown) for the tile
 *   skip; max_mesh_tris (host) >= every mesh's triangle count (sizes the launch); mesh_ids_dev (B,) int32 the mesh of every env,
 *   nullable = mesh 0, read on the device - an id outside [0, num_meshes) renders nothing (+inf); pos / quat / intrinsics / clipping /
 *   depth_m_dev (B,H,W) as in tacex_depth_from_mesh.  Tables are not checked on the device.  Each env's image is bit-equal to
 *   tacex_depth_from_mesh on its mesh alone (same float32 operations).  Meshes of more than 1024 triangles are rendered by several
 *   workgroups per image tile (a second launch on the stream, merged with an atomic minimum).
 * Returns 2 (no GPU call) on a null buffer, num_meshes or max_mesh_tris <= 0, an empty image or a bad clipping range. */
int tacex_depth_from_mesh_library(const float* verts_dev, const int32_t* tris_dev, const int32_t* mesh_tris_dev,
                                  const float* mesh_spheres_dev, int num_meshes, int max_mesh_tris, const int32_t* mesh_ids_dev,
                                  const float* pos_dev, const float* quat_dev, float fx, float fy, float cx, float cy,
                                  float near_clip_m, float far_clip_m, float* depth_m_dev, int num_envs, int height, int width,
                                  void* stream);

/* TS:115-131 on an existing mm height map. frame_min_dev (B,) is also written (re-used by the render);
 * frame_rows_dev (B,4) int32 nullable: contact row / column ranges as in tacex_height_map_from_depth. */
int tacex_indentation_depth(const float* hm_mm_dev, float gelpad_height_m,
                            float gelpad_to_camera_min_distance_m, float* frame_min_dev,
                            float* indent_mm_dev, int32_t* frame_rows_dev, int num_frames, int height, int width,
                            void* stream);

/* Shadow branch tables (TaximTorch.__init__ shadow calibration TT:96-126 + the per-shape parameters of TT:260-346).
 * Optional: only needed before a render with TACEX_FLAG_WITH_SHADOW. Host pointers, copied once. */
typedef struct tacex_shadow_params {
  int32_t num_directions;      /* 63  (shadowDirections) */
  int32_t num_fan_rays;        /* 4   = int(2 * fan_angle / fan_precision), TT:102 */
  int32_t num_heights;         /* 24 */
  int32_t num_steps;           /* 51  (longest table entry; shorter ones padded with +inf, TT:118-126) */
  const float* fan_angles;     /* (num_directions, num_fan_rays): direction + linspace(-fan_angle, fan_angle), TT:103-105 */
  const float* fan_cos;        /* (num_directions, num_fan_rays) float32 cos / sin of fan_angles as the HOST library computes them */
  const float* fan_sin;        /*   (torch.cos / torch.sin of the float32 table, TT:299,303): the device multiplies by these bits */
  const float* table;          /* (3, num_directions, num_heights, num_steps), RGB order, already / 255, +inf padded */
  int32_t win_left, win_right, win_top, win_bottom; /* composite window of the two box-dilation rounds, TT:261-272 */
  float shadow_depth_0;        /* 0.4, TT:97 */
  float height_precision;      /* params.json simulator.height_precision (0.1) */
  float discretize_precision;  /* params.json simulator.discretize_precision (0.1) */
  float step_x, step_y;        /* shadow_step(shape)[1], [0] (sic: x uses the height-scaled value), TT:298-305 */
  int32_t blur_kw, blur_kh;    /* shadow_blur_sigma kernel, TT:339-342: odd, (k - 1) / 2 smaller than the image (reflect padding) */
  const float* blur_taps_w;
  const float* blur_taps_h;
} tacex_shadow_params;

int tacex_taxim_set_shadow(tacex_taxim_ctx* ctx, const tacex_shadow_params* params);
/* extra scratch (beyond tacex_taxim_workspace_bytes) a render with TACEX_FLAG_WITH_SHADOW needs, placed right after it */
size_t tacex_taxim_shadow_workspace_bytes(const tacex_taxim_ctx* ctx, int num_frames);
/* The ray march of the shadow branch alone (TT:261-337): deformed gel z_dev (B,H,W) mm, shrunken contact mask mask_dev
 * (B,H,W) uint8, gradient direction grad_dir_dev (B,H,W) -> shadow_min_dev (B,H,W,3): per pixel and channel the minimum
 * table value over all ray samples that hit it, +inf where none does (what torch_scatter.scatter_min leaves in
 * `shadow_img`, TT:324-336).  Ring pixels, table bins and sample coordinates are integer work in the reference's op order
 * (float32 multiply, add, truncate - no fused multiply-add): parity tests compare this map EXACTLY. */
int tacex_taxim_shadow_rays(tacex_taxim_ctx* ctx, const float* z_dev, const uint8_t* mask_dev, const float* grad_dir_dev,
                            float* shadow_min_dev, int num_frames, void* stream);

/* Flags for tacex_taxim_render / tacex_taxim_deform */
#define TACEX_FLAG_NO_SHIFT      1u  /* press_depth=None: use the height map as is (TT:188-189 skipped) */
#define TACEX_FLAG_HAVE_FRAME_MIN 2u /* frame_min_dev already holds min(hm) per frame (skip that pass) */
#define TACEX_FLAG_OBS_U8         8u /* render_obs only: obs_out_dev is uint8 (B,obs_h,obs_w,3) = floor(255 x + 0.5) */
#define TACEX_FLAG_WITH_SHADOW    4u /* render only: shadow branch TT:260-346 (needs tacex_taxim_set_shadow + extra scratch) */
#define TACEX_FLAG_HAVE_FRAME_ROWS 16u /* with HAVE_FRAME_MIN: the buffer of tacex_taxim_set_frame_rows describes THESE height maps */

/* Contact row / column ranges of the height maps handed to the render (written by tacex_height_map_from_depth /
 * tacex_indentation_depth into a caller-owned (capacity_frames, 4) int32 buffer).  The deformed gel of TT:443-473 is exactly
 * zero on every pyramid band - and every 64-column block of a band - whose input window lies outside the ranges (zero gel map
 * only): those are stored as zeros without reading or multiplying anything.  Used only by calls that pass TACEX_FLAG_HAVE_FRAME_MIN | TACEX_FLAG_HAVE_FRAME_ROWS
 * with num_frames <= capacity_frames; without HAVE_FRAME_MIN the library computes the ranges in its own minimum pass.
 * nullptr disables. */
int tacex_taxim_set_frame_rows(tacex_taxim_ctx* ctx, const int32_t* frame_rows_dev, int capacity_frames);

/* TaximSimulator.optical_simulation (TS:80-113) -> Taxim.render_direct (TI:153-163) ->
 * TaximTorch._render_impl / __render no-shadow branch (TT:174-258), output already NHWC (TS:109-111).
 *   hm_mm_dev   (B,H,W) height map in mm (H,W = ctx size)
 *   press_dev   (B,)    press depth in mm (= indentation depth); ignored with TACEX_FLAG_NO_SHIFT
 *   frame_min_dev (B,)  scratch/in: per-frame min of hm (see TACEX_FLAG_HAVE_FRAME_MIN)
 *   rgb_dev     (B,H,W,3) float32 in [0,1]
 *   z_out_dev   (B,H,W) deformed gel (mm) after the final blur, nullable      (TT:443-473 result #1)
 *   mask_out_dev(B,H,W) uint8 shrunken contact mask, nullable                 (TT:473 result #2)
 *   workspace_dev: tacex_taxim_workspace_bytes(ctx, B) bytes of device scratch */
int tacex_taxim_render(tacex_taxim_ctx* ctx, const float* hm_mm_dev, const float* press_dev,
                       float* frame_min_dev, float* rgb_dev, float* z_out_dev, uint8_t* mask_out_dev,
                       void* workspace_dev, int num_frames, unsigned flags, void* stream);

/* FOTS contact statistics as a by-product of the render: when a buffer is set, the fused tail kernel (where one exists:
 * tacex_taxim_fots_partials_per_env > 0) stores one 16-byte partial {max Z, mask count, row sum, column sum} per wave and
 * tile while the frame is in LDS; tacex_fots_markers_partials consumes them.  Only calls with num_frames <= capacity_frames
 * write (the buffer holds capacity_frames * partials_per_env records); nullptr disables. */
int tacex_taxim_fots_partials_per_env(const tacex_taxim_ctx* ctx);
/* ... and the deformed gel / contact mask AT THE MARKER PIXELS only (FOTS looks nothing else up, MM:152-166): with the taps
 * set, the fused tail also fills z_pix_dev / mask_pix_dev (capacity_frames, n_markers) and the caller may pass
 * z_out_dev = mask_out_dev = NULL to the render - 5 B/px of stores less.  marker_x / marker_y: HOST int32 pixel positions
 * (the FOTS marker grid); markers outside the image are skipped.  NULL buffers disable. */
int tacex_taxim_set_fots_taps(tacex_taxim_ctx* ctx, const int32_t* marker_x, const int32_t* marker_y, int n_markers,
                              float* z_pix_dev, uint8_t* mask_pix_dev, int capacity_frames);
int tacex_taxim_set_fots_partials(tacex_taxim_ctx* ctx, void* partials_dev, int capacity_frames);

/* tacex_taxim_render + the low-resolution POLICY OBSERVATION in the same pass: obs_out_dev (B,obs_h,obs_w,3) is the
 * antialiased bilinear down-sample of the RGB frame (torchvision resize semantics, as tasks feed 32x32x3 to the policy:
 * tacex_tasks/.../ball_rolling_tactile_rgb.py:303,318).  Where the fused tail kernel exists the horizontal half of the
 * filter is accumulated while the frame is still in LDS (the full-resolution frame is never re-read), otherwise it falls
 * back to the two-pass resize.  obs_scratch_dev: obs_scratch_floats (csrc/taxim_layout.h) = B * (max(H * obs_w, obs_h * W) + obs_h * obs_w) * 3.
 * obs_out_dev is float32, or uint8 with TACEX_FLAG_OBS_U8 (the image a CNN policy consumes; a quarter of the bytes in the
 * per-step observation all-gather). */
int tacex_taxim_render_obs(tacex_taxim_ctx* ctx, const float* hm_mm_dev, const float* press_dev, float* frame_min_dev,
                           float* rgb_dev, float* z_out_dev, uint8_t* mask_out_dev, void* workspace_dev,
                           float* obs_scratch_dev, void* obs_out_dev, int obs_h, int obs_w, int num_frames,
                           unsigned flags, void* stream);

/* __get_shifted_height_map + __compute_gel_pad_deformation only (TT:432-473), as the FOTS wrapper calls
 * them (FS:128-129). Same arguments as above without the shading. */
int tacex_taxim_deform(tacex_taxim_ctx* ctx, const float* hm_mm_dev, const float* press_dev,
                       float* frame_min_dev, float* z_out_dev, uint8_t* mask_out_dev,
                       void* workspace_dev, int num_frames, unsigned flags, void* stream);

/* Shading only: deformed gel (B,H,W) mm -> RGB (TT:237-258): normals, bins, polynomial, + background, clip.
 * idx_out_dev (B,H,W,2) uint8 [idx_mag, idx_dir] is optional (parity tests). */
int tacex_taxim_shade(tacex_taxim_ctx* ctx, const float* z_dev, float* rgb_dev, uint8_t* idx_out_dev,
                      int num_frames, void* stream);

/* torchvision resize(bilinear, antialias=True) of a batch of single-channel images, used when the camera
 * resolution differs from the tactile resolution (TS:88-89, FS:121-122). */
int tacex_resize_bilinear_aa(const float* src_dev, int src_h, int src_w, float* dst_dev, int dst_h,
                             int dst_w, int num_frames, void* stream);
/* Same filter on channels-last images (B,H,W,C): produces the low-resolution policy observation from the
 * tactile RGB frame (tasks feed 32x32x3 to the policy, tacex_tasks/.../ball_rolling_tactile_rgb.py:303,318),
 * which is what the multi-GPU observation all-gather carries. */
int tacex_resize_bilinear_aa_nhwc(const float* src_dev, int src_h, int src_w, float* dst_dev, int dst_h,
                                  int dst_w, int channels, int num_frames,
                                  float* tmp_dev /* num_frames*dst_h*src_w*channels floats: separable two-pass
                                                    (recommended for down-sampling); NULL = single pass */,
                                  void* stream);

/* Ablation / test hook: 1 (default) = trailing small-kernel levels + shading run as ONE fused kernel where a tuned
 * instantiation exists (320x240, 640x480): the wave-autonomous streaming kernel (taxim_stream.hip) for plain renders, the
 * LDS-tiled kernel (taxim_tail.hip) when the full deformed-gel / mask frames are requested; 2 = always the LDS-tiled kernel;
 * 0 = every level as its own kernel + separate shade kernel. */
int tacex_taxim_set_fused_tail(tacex_taxim_ctx* ctx, int enabled);

/* Route read-back (tests, diagnostics): which kernel family the context's next render runs pyramid level `level` on - the
 * library answers from the same decision its launch code takes.  -1: null context / level out of range. */
#define TACEX_ROUTE_GENERIC 0        /* two-pass generic blur */
#define TACEX_ROUTE_BAND 1           /* fully unrolled band kernel */
#define TACEX_ROUTE_BAND_LOOP_384 2  /* looped band kernel, 384-thread form (W <= 384) */
#define TACEX_ROUTE_BAND_LOOP_640 3  /* looped band kernel, 640-thread form */
#define TACEX_ROUTE_MFMA 4           /* matrix-core band kernel */
#define TACEX_ROUTE_TAIL 5           /* fused into the tail (tacex_taxim_set_fused_tail) */
int tacex_taxim_level_route(const tacex_taxim_ctx* ctx, int level);
/* ... and how a render without the shadow branch ends: with_frames = 0 a plain render, != 0 one that also stores the full
 * deformed-gel / mask frames (z_out / mask_out).  -1: null context. */
#define TACEX_TAIL_NONE 0    /* every level as its own kernel, then the shade kernel */
#define TACEX_TAIL_TILED 1   /* LDS-tiled fused tail (taxim_tail.hip) */
#define TACEX_TAIL_STREAM 2  /* streaming fused tail (taxim_stream.hip) */
int tacex_taxim_tail_route(const tacex_taxim_ctx* ctx, int with_frames);

/* Frames one pass of the kernel sequence covers for a call with num_frames frames: large shards are walked in chunks whose
 * level buffers stay resident in the 256 MB Infinity Cache (== num_frames when the shard is rendered in one pass).
 * bench.py needs it to turn per-launch durations into bytes per launch. */
int tacex_taxim_chunk_frames(const tacex_taxim_ctx* ctx, int num_frames);

/* Optional per-stage timing with hipEvents on the launch stream (bench.py's roofline leg).
 * Stages: 0 = frame-min, 1..n_levels = blur levels, n_levels+1 = shade, n_levels+2 = fused tail. */
int tacex_taxim_set_profiling(tacex_taxim_ctx* ctx, int enabled);
/* Synchronises the recorded events; returns accumulated milliseconds and launch count, then resets. */
int tacex_taxim_read_profile(tacex_taxim_ctx* ctx, int stage, double* total_ms, int* launches);
int tacex_taxim_num_stages(const tacex_taxim_ctx* ctx);
const char* tacex_taxim_stage_name(const tacex_taxim_ctx* ctx, int stage);

/* ---------------------------------------------------------------------------------------------
 * FOTS marker-displacement field (MM:22-219 driven per env by FS:114-184).
 * ------------------------------------------------------------------------------------------- */
typedef struct tacex_fots_params {
  int32_t height, width;          /* tactile image size */
  int32_t num_markers_row, num_markers_col; /* 9, 11 (FSC:46-53) */
  const int32_t* marker_x;        /* HOST (rows*cols,) initial pixel x, row-major (row, col), MM:59-76 */
  const int32_t* marker_y;        /* HOST (rows*cols,) initial pixel y */
  double lamb[3];                 /* [dilate, shear, twist] = [0.00125, 0.00021, 0.00038], FS:77 */
  float mm2pix;                   /* 19.58, FSC:36 */
  float shear_max;                /* 10 px, MM:78 */
  float theta_max_deg;            /* 60 deg, MM:90 */
} tacex_fots_params;

int tacex_fots_create(int device_id, const tacex_fots_params* params, tacex_fots_ctx** out);
void tacex_fots_destroy(tacex_fots_ctx* ctx);

/* Per-env trajectory state (FS:101-103,168,176-177): only traj[0], traj[-1] and len(traj) are ever read
 * (MM:177-205).  Layout of traj_state_dev: (B, 8) float32 = [len, x0, y0, th0, xl, yl, thl, n_contacts of the last step].
 * Bytes needed: */
size_t tacex_fots_state_bytes(int num_envs);
size_t tacex_fots_workspace_bytes(int num_envs);

/* FS:130-182 for all envs in one go:
 *   z_dev (B,H,W) deformed gel, mask_dev (B,H,W) uint8 (both from tacex_taxim_deform / _render),
 *   indent_dev (B,) mm, theta_dev (B,) yaw of the indenter in the sensor frame (replaces the
 *   FrameTransformer read-out FS:147-159), traj_state_dev in/out,
 *   markers_dev (B,2,M,2) float32: [initial | current] x (x, y), FS:90-99. */
int tacex_fots_markers(tacex_fots_ctx* ctx, const float* z_dev, const uint8_t* mask_dev,
                       const float* indent_dev, const float* theta_dev, float* traj_state_dev,
                       float* markers_dev, void* workspace_dev, int num_envs, void* stream);

/* With pixels_compact != 0, z_dev / mask_dev are the (num_envs, num_markers) arrays tacex_taxim_set_fots_taps fills
 * instead of full (num_envs, H, W) frames. */
int tacex_fots_markers_compact(tacex_fots_ctx* ctx, const float* z_pix_dev, const uint8_t* mask_pix_dev,
                               const float* indent_dev, const float* theta_dev, float* traj_state_dev,
                               float* markers_dev, void* workspace_dev, const void* partials_dev,
                               int partials_per_env, int num_envs, void* stream);
/* Same, with the per-env contact statistics (max of the deformed gel, mask centroid sums; FS:130-141) taken from the
 * partials a tacex_taxim_render* / _deform call wrote (tacex_taxim_set_fots_partials) instead of re-reading z / mask. */
int tacex_fots_markers_partials(tacex_fots_ctx* ctx, const float* z_dev, const uint8_t* mask_dev,
                                const float* indent_dev, const float* theta_dev, float* traj_state_dev,
                                float* markers_dev, void* workspace_dev, const void* partials_dev,
                                int partials_per_env, int num_envs, void* stream);

/* Marker IMAGE and RGB x marker overlay (FS:346-384 `draw_markers`, FS:265-272) for all envs:
 *   canvas (H+24, W+24) uint8 = 255; for every marker in index order (later ones overwrite):
 *     u = x + 0.5 + 12, v = y + 0.5 + 12 (float64); patch = table[floor(frac(u) SR)][floor(frac(v) SR)][patch_w] (12 x 12);
 *     stamped at (floor(u) - 6, floor(v) - 6) when it lies fully inside the canvas;  image = canvas[12:-12, 12:-12].
 *   markers_dev (B,2,M,2) f32 as written by tacex_fots_markers (the CURRENT positions, index 1, are drawn);
 *   patch_table_dev (SR, SR, size_slots, 12, 12) uint8 - the reference draws it with cv2 (`generate_patch_array`, FS:387-446);
 *   patch_w = floor((marker_size - base_circle_radius) * SR) (FS:370-373: 15 for marker_size 3);
 *   img_dev (B,H,W) uint8 [nullable]; overlay_dev (B,H,W,3) uint8 = uint8(float64(rgb * 255) * marker / 255) [nullable,
 *   needs rgb_dev (B,H,W,3) f32]. */
int tacex_fots_marker_image(const float* markers_dev, const uint8_t* patch_table_dev, int super_resolution_ratio,
                            int size_slots, int patch_w, const float* rgb_dev, uint8_t* img_dev, uint8_t* overlay_dev,
                            int num_envs, int num_markers, int height, int width, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gelpad FEM inner step (what libuipc's world.advance() runs for the StableNeoHookean gelpad,
 * US:250-252, UO:442-470, UA:364-428).  Batched: `num_envs` independent copies of one tet mesh.
 * All floating point is float64.  Parity: UNPINNED (libuipc is an un-vendored submodule); the
 * restatement follows Smith, de Goes, Kim 2018 "Stable Neo-Hookean Flesh Simulation".
 * ------------------------------------------------------------------------------------------- */
typedef struct tacex_fem_params {
  int32_t num_verts, num_tets;
  const double* rest_positions;  /* HOST (V,3) */
  const int32_t* tets;           /* HOST (T,4) */
  double youngs, poisson;        /* Pa, - (UO:59,76-88: E = 0.01 MPa, nu = 0.49) */
  double density;                /* kg/m^3 (1e3) */
  double dt;                     /* s (US:57: 0.01) */
  double gravity[3];             /* (0,0,-9.8) US:60 */
  double constraint_strength_ratio; /* SoftPositionConstraint strength (UA:38: 100) */
} tacex_fem_params;

int tacex_fem_create(int device_id, const tacex_fem_params* params, tacex_fem_ctx** out);
void tacex_fem_destroy(tacex_fem_ctx* ctx);
size_t tacex_fem_workspace_bytes(const tacex_fem_ctx* ctx, int num_envs);

/* Per-element Stable-Neo-Hookean energy, gradient (12) and Hessian (12x12, optionally PSD-projected),
 * one tet per lane.  x_dev (B,V,3); outputs nullable: energy_dev (B,T), grad_dev (B,T,12), hess_dev (B,T,144). */
int tacex_fem_element_terms(tacex_fem_ctx* ctx, const double* x_dev, double* energy_dev, double* grad_dev,
                            double* hess_dev, int project_psd, int num_envs, void* stream);

/* Total incremental potential per env (inertia + dt^2 * elastic + soft position constraints),
 * wavefront-reduced: E_dev (B,).  x_tilde_dev (B,V,3) is the inertial target; constrained_dev (B,V) uint8
 * and aim_dev (B,V,3) describe UA:364-385's animation targets (nullable = no constraints). */
int tacex_fem_energy(tacex_fem_ctx* ctx, const double* x_dev, const double* x_tilde_dev,
                     const uint8_t* constrained_dev, const double* aim_dev, double* E_dev,
                     void* workspace_dev, int num_envs, void* stream);

/* Assembled nodal gradient (B,V,3) of the same potential - atomics-free vertex gather over incident tets. */
int tacex_fem_gradient(tacex_fem_ctx* ctx, const double* x_dev, const double* x_tilde_dev,
                       const uint8_t* constrained_dev, const double* aim_dev, double* g_dev,
                       void* workspace_dev, int num_envs, void* stream);

/* IPC contact of the gelpad SURFACE against one analytic indenter per env (first slice; reference cfg
 * US:103-124 `Contact`: constitution "ipc", d_hat 1e-3, resistance 10 GPa - libuipc's Compute Contact / Detect Candidates).
 * Every surface vertex v gets the barrier term  dt^2 * stiffness * area_v * b(d_v / d_hat),  b(s) = -(s-1)^2 ln s on (0,1)
 * (Li et al. 2020 eq. 6), d_v = signed distance to the indenter (sphere |x - c| - R, half-space n.(x - c), capsule: distance to the axis segment - R); the energy,
 * gradient, PSD-projected Hessian (b'' n n^T) enter tacex_fem_energy / _gradient / _newton_step, and the Newton step length is
 * first cut to 0.9 x the conservative bound min_v d_v / |dx_v| (the CCD filter of the line search: no vertex can cross the
 * indenter surface), then backtracked on the energy as before.  Friction and mesh-mesh contact are not part of this slice.
 *   vertex_area_host (V) HOST f64: a third of the area of the surface triangles around a vertex, 0 for interior vertices
 *                    (copied once; NULL keeps the previous table);
 *   indenters_dev (num_envs, 8) f64 [kind, cx, cy, cz, radius, nx, ny, nz]: kind 0 none, 1 sphere, 2 half-space (unit
 *                    normal n through c), 3 capsule (radius around the segment c -+ (nx, ny, nz): the vector is HALF the
 *                    axis); read by every later compute call until replaced; NULL disables contact.
 * Replaced tables are freed by the setter (it drains the device first: a set-up call, not a step-path call). */
int tacex_fem_set_contact(tacex_fem_ctx* ctx, const double* vertex_area_host, double d_hat, double stiffness,
                          const double* indenters_dev);

/* Coulomb friction of the gelpad surface against its env's indenter (US:103-124: enable_friction, default_friction_ratio,
 * eps_velocity), the IPC way (Li et al. 2020, eq. 18-20) with normal force and contact normal lagged per time step - taken at the
 * state the step starts from, the normal force capped by the contact reaction there (= the previous step's normal force); the
 * tangential sliding is measured from the positions the time step starts at and relative to the indenter's own displacement
 * since the previous tacex_fem_step (its positions are kept in the workspace), potential mu lam f0(|u|) smoothed below
 * eps_velocity * dt.  The displacement is the TRANSLATION of the indenter row (cx, cy, cz) between two steps: the caller may move
 * an indenter by mutating the rows in place or by handing a new indenters_dev to tacex_fem_set_contact every step (the previous
 * positions survive that call; they are reset when contact is disabled, enabled for the first time, or when tacex_fem_step runs
 * with another workspace / num_envs).  A ROTATION of a capsule or mesh indenter (kinds 3 / 4: the last three row entries) between
 * two steps is not part of the displacement - a spinning indenter drags the pad as if it only translated.
 * Acts inside tacex_fem_step only (tacex_fem_newton_step has no notion of the step's start).  friction_ratio 0 = off. */
int tacex_fem_set_friction(tacex_fem_ctx* ctx, double friction_ratio, double eps_velocity);

/* WHERE the friction lag (normal force lam and normal n per contact vertex, frozen for the time step) is taken:
 *   1 - IPC's rule to the letter (Li et al. 2020, section 5.4, "lagged from the previous time step"): barrier force and normal of the
 *       PREVIOUS configuration, i.e. the positions the step starts from against the indenter where it stood at the previous step;
 *   0 - (round 4) at the step's start positions against the indenter's NEW position, the force capped by the contact reaction there.
 * Both are the previous step's normal force where that step converged tightly and the indenter approaches; they differ when it
 * retreats (0 takes the smaller, already relaxed barrier force) and at loose Newton tolerances.  Only mode 1 makes the step's end
 * state a stationary point of the plain incremental potential of IPC (tests/test_fem_physics_gpu.py); mode 0 (the default) is the
 * one that stays bounded at the reference's default Newton tolerance, where the previous configuration is not in balance. */
int tacex_fem_set_friction_lag(tacex_fem_ctx* ctx, int mode);

/* Which Newton kernel the last tacex_fem_step / tacex_fem_newton_step of the context launched: 1 = CU-resident (the env's state on one CU),
 * 0 = the streaming fallback (larger meshes, the deterministic switch on more than 512 vertices), -1 = none yet.  (ABI 11) */
int tacex_fem_newton_resident(const tacex_fem_ctx* ctx);

/* The route of the last Newton launch of the context (tacex_fem_step, tacex_fem_newton_step, tacex_fem_ball_step) (ABI 18):
 *   threads  = threads per env: 256, 512 or 768 for the CU-resident kernel, the block size of the streaming and ball kernels; 0 = none yet
 *   lds_mode = -1 for the CU-resident and ball kernels; for the streaming kernel 2 = every PCG vector in LDS (21 V doubles),
 *              1 = x, p and the H.p accumulators (9 V doubles), 0 = global memory (the deterministic switch, or neither fits).
 * Every kernel's dynamic LDS must fit next to its static __shared__ in a CU's 160 KB; a pad that does not fit one route takes the next. */
int tacex_fem_newton_route(const tacex_fem_ctx* ctx, int* threads, int* lds_mode);

/* Contact-following start of tacex_fem_step's Newton loop (default on): a surface vertex inside the barrier zone of the indenter's
 * previous position starts the iteration displaced by the indenter's translation since the previous step (its gap is what it was).
 * An initial guess only - the step's minimiser is unchanged - but the one that lets a RETREATING indenter cost 2-3 Newton iterations
 * like a pressing one instead of 4-30 (libuipc starts from the current positions: world.advance(), US:250-252; 0 restores that). */
int tacex_fem_set_contact_following(tacex_fem_ctx* ctx, int enable);

/* Summation order of the CU-resident Newton kernel's tet -> vertex sums.  0 (default): per-tet rows are added into per-vertex LDS
 * accumulators with ds_add_f64 - the order of a vertex's ~24 contributions depends on wave timing, so two runs agree to round-off
 * (1e-16 relative per add), not bit for bit.  1: rows travel through an exchange window and are gathered in a fixed order (bit-identical
 * runs, ~25 % more time per PCG iteration).  No counterpart in the reference (libuipc's CUDA backend uses atomics throughout). */
int tacex_fem_set_deterministic(tacex_fem_ctx* ctx, int enable);

/* Two-level preconditioner of the Newton system (CU-resident kernel): z = D^-1 r (3x3 block Jacobi, always) + P A_c^-1 P^T r.
 * P: every vertex has 8 (coarse node, weight) pairs - the trilinear hat functions of a small grid laid over the mesh
 * (vertex_nodes_host (V,8) int32 in [0, num_coarse), vertex_weights_host (V,8) f64 >= 0, rows summing to 1; unused slots weight 0);
 * coarse_inverse_host (3 num_coarse, 3 num_coarse) f64 = inverse of P^T A_0 P with A_0 = M (1 + s C) + dt^2 K(rest state), built
 * by the caller (UipcSim does it from tacex_fem_element_terms at the rest state and the constraint flags; constant per mesh
 * and constraint set).  num_coarse <= 64; 0 switches the coarse correction off.  Tables are copied. */
int tacex_fem_set_coarse_space(tacex_fem_ctx* ctx, int num_coarse, const int32_t* vertex_nodes_host,
                               const double* vertex_weights_host, const double* coarse_inverse_host);

/* gaps_dev (num_envs, V) f64 <- signed distance of every vertex of x_dev (num_envs, V, 3) to its env's indenter, by the solver's own
 * distance function (+inf without an indenter): what the caller of tacex_fem_step needs to keep the "an indenter approaches by less
 * than the current gap" contract (UipcSim.contact_gaps). */
int tacex_fem_contact_gaps(tacex_fem_ctx* ctx, const double* x_dev, double* gaps_dev, int num_envs, void* stream);

/* Contact forces of the gelpad at the state x_dev (num_envs, V, 3) and their net wrench per env, from the solver's own barrier and
 * friction terms.  Forces act ON THE PAD, in newtons; the force on the indenter is the negative.  Per surface vertex:
 *   normal force   f_n = lam n, lam = -dB/dd >= 0 of the barrier at x, n the contact normal (away from the indenter);
 *   friction force f_f = -grad of IPC's lagged friction potential at x (with_friction != 0): lag and sliding reference are those of the
 *                  context's LAST tacex_fem_step - its start positions, indenter displacement and the indenter position it ended with,
 *                  read from step_workspace_dev (the indenter rows give kind, radius and axis only: moving an indenter after the step
 *                  changes the normal part, not the friction part) - with the env's own friction ratio (material library).  Reported for IPC's lag only (tacex_fem_set_friction_lag mode 1): a
 *                  function of stored data alone.  With mode 0, a null workspace, or a workspace / num_envs other than the last
 *                  step's, a call with with_friction set is refused (2) with a message; nothing is approximated.
 * A vertex at or beyond the indenter surface contributes nothing (it shows in slot 15).  An env without an indenter (kind 0, a mesh id
 * outside the library) reports zeros; an env whose friction reference was cleared (tacex_fem_reset_envs) and has not stepped since
 * reports zero friction (the reset clears that reference only: the normal part is the barrier's at the reset state).  Friction ratio 0 or contact disabled: valid zeros.
 * wrench_dev (num_envs, 16) f64:
 *   0..2 sum f_n | 3..5 sum f_f | 6..8 torque sum (x_v - ref) x (f_n + f_f) | 9 sum lam_v | 10 contact area (sum of the vertex areas of
 *   the active vertices) | 11 number of active vertices | 12..14 centre of pressure sum lam_v x_v / sum lam_v (the reference point when
 *   sum lam = 0) | 15 smallest gap over the surface vertices (+inf without an indenter)
 * ref_points_dev (num_envs, 3): the torque's reference point per env (NULL: the origin).  vertex_force_dev (num_envs, V, 3), nullable:
 * f_n + f_f of every vertex, zeros at interior and inactive vertices.  One launch, fixed summation order: bit-reproducible, and an
 * env's results do not depend on the batch it shares.  The rotation of an indenter between two steps does not enter the friction
 * displacement (tacex_fem_set_friction).  Not implemented for a scene with an affine body (2): tacex_fem_ball_contact_forces reports
 * that scene's pair contacts.  Enqueued on `stream`. */
int tacex_fem_contact_forces(tacex_fem_ctx* ctx, const double* x_dev, const void* step_workspace_dev /* nullable: no friction */,
                             const double* ref_points_dev /* (B,3), nullable: origin */, int with_friction,
                             double* wrench_dev /* (B,16) */, double* vertex_force_dev /* (B,V,3), nullable */,
                             int num_envs, void* stream);

/* Rigid TRIANGLE-MESH indenter shared by all envs (indenter kind 4 of tacex_fem_set_contact's rows): vertices (num_verts,3) f64 in
 * the mesh's own frame, triangles (num_tris,3) int32.  An env's indenter row [4, px, py, pz, offset, rx, ry, rz] places it: p =
 * position of the mesh origin, r = rotation vector (axis * angle), offset >= 0 inflates the surface.  The barrier acts between
 * every weighted gelpad vertex and its nearest triangle (point-triangle distance, closest feature = face / edge / vertex);
 * the distance is unsigned.  num_tris = 0 removes the mesh.  Tables are copied. */
int tacex_fem_set_indenter_mesh(tacex_fem_ctx* ctx, int num_verts, const double* verts_host, int num_tris, const int32_t* tris_host);

/* Indenter mesh LIBRARY (ABI 17): one rigid mesh PER ENV for indenter kind 4, chosen by a device id array
 * (tacex_fem_set_indenter_mesh_ids).  Mesh k has vert_counts[k] vertices and tri_counts[k] triangles; verts_host holds every mesh's
 * (vert_counts[k],3) f64 vertices back to back, tris_host every mesh's (tri_counts[k],3) int32 triangles back to back, each indexing
 * its own mesh's vertices.  Each mesh is ordered and clustered exactly as tacex_fem_set_indenter_mesh does it, so an env sees the same
 * distances as with that mesh alone; tacex_fem_set_indenter_mesh is a library of one with no id array.  num_meshes = 0 removes the
 * library.  Tables are copied; the id array set before stays in place. */
int tacex_fem_set_indenter_mesh_library(tacex_fem_ctx* ctx, int num_meshes, const int32_t* vert_counts, const double* verts_host,
                                        const int32_t* tri_counts, const int32_t* tris_host);

/* ids_dev (B,) int32 device: the library mesh of every env, read by every later call with B envs (the caller may rewrite it between
 * steps, e.g. to draw new shapes at a reset; it must stay allocated while set).  NULL: every env uses mesh 0.  An id outside
 * [0, num_meshes) is never dereferenced: that env's kind-4 row acts as no indenter and tacex_fem_step sets flag 32 in its
 * step_info[., 2]. */
int tacex_fem_set_indenter_mesh_ids(tacex_fem_ctx* ctx, const int32_t* ids_dev);

/* Gel MATERIAL LIBRARY (ABI 19): one gel material PER ENV, chosen by a device id array (tacex_fem_set_material_ids) - the reference's
 * per-object StableNeoHookeanCfg(youngs_modulus, poisson_rate) / mass_density (tacex_uipc/objects/uipc_object.py:54-92) and the
 * per-element friction ratio of its contact tabular, for envs that share one context.  Host arrays of num_materials entries: youngs
 * [Pa] > 0, -1 < poisson < 0.5, density [kg/m^3] > 0, friction_ratio >= 0 (as tacex_fem_create / tacex_fem_set_friction).  Per material
 * the library holds what tacex_fem_create builds for the scene's one material - the Stable Neo-Hookean constants and the (V) mass
 * table, by the same expressions in the same order - so an env of material k computes bit for bit (tacex_fem_set_deterministic) what a
 * context created with material k and tacex_fem_set_friction(ratio k) computes.  Honoured by tacex_fem_step, tacex_fem_newton_step,
 * tacex_fem_element_terms, tacex_fem_energy and tacex_fem_gradient (every Newton kernel route).  While a library is set the ratio of
 * tacex_fem_set_friction is not used (its eps_velocity is); friction is on for the scene when any material's ratio is > 0, an env
 * whose material has ratio 0 runs without.  d_hat, contact stiffness, eps_velocity, dt and the constraint strength stay scene-wide.
 * num_materials = 0 removes the library (and its coarse inverses): the scene is again what tacex_fem_create / tacex_fem_set_friction
 * made.  Not implemented together with tacex_fem_set_affine_body: either call fails when the other is in force.  Tables are copied;
 * the id array set before stays in place. */
int tacex_fem_set_material_library(tacex_fem_ctx* ctx, int num_materials, const double* youngs, const double* poisson,
                                   const double* density, const double* friction_ratio);

/* ids_dev (B,) int32 device: the library material of every env, read by every later call with B envs (the caller may rewrite it
 * between steps, e.g. to draw new gels at a reset; it must stay allocated while set).  NULL: every env uses material 0.  An id outside
 * [0, num_materials) is never dereferenced: that env computes with material 0 and tacex_fem_step sets flag 64 in its step_info[., 2]. */
int tacex_fem_set_material_ids(tacex_fem_ctx* ctx, const int32_t* ids_dev);

/* The coarse inverse of tacex_fem_set_coarse_space depends on the material: coarse_inverses_host (num_materials, 3 num_coarse,
 * 3 num_coarse) f64, one per material of the library, each built as the coarse_inverse_host of a scene of that material alone.  Call
 * after tacex_fem_set_material_library and tacex_fem_set_coarse_space (either of them drops these tables); without it every env uses
 * the scene's one inverse (a valid, weaker preconditioner for the other materials).  num_materials = 0 removes them.  Copied. */
int tacex_fem_set_material_coarse_inverses(tacex_fem_ctx* ctx, int num_materials, const double* coarse_inverses_host);

/* Block part of the preconditioner: block-tridiagonal LDL^T along VERTEX CHAINS instead of one 3x3 block per vertex.  A chain is a
 * sequence of mesh vertices, consecutive ones sharing a tet (the columns of vertices through a gelpad's thickness: the nearly
 * incompressible material couples the layers of a thin pad most strongly; UipcSim builds them with
 * coarse_space.build_vertex_chains).  chain_offsets_host (num_chains + 1) indexes chain_vertices_host; every vertex may appear in at
 * most one chain, the rest are chains of one vertex (= block Jacobi).  num_chains = 0 switches chains off.  Per Newton iteration the
 * kernel factors S_0 = D_0, G_i = S_i^-1 A(i, i+1), S_{i+1} = D_{i+1} - A(i, i+1)^T G_i and keeps S^-1 / G as floats in LDS.
 * Tables are copied.  (CU-resident Newton kernel only.) */
int tacex_fem_set_chains(tacex_fem_ctx* ctx, int num_chains, const int32_t* chain_offsets_host, const int32_t* chain_vertices_host);

/* Device-side convergence for repeated Newton launches: dx_dev (num_envs,) f64 holds, per env, max |d| of the UNSCALED Newton
 * direction of its last iteration - not of the update the CCD bound and the line search made of it (the caller fills it with
 * +inf at the start of a time step); an env whose value is <= dx_tol
 * (= velocity_tol * dt, US:62-66) returns at once from the next tacex_fem_newton_step, so extra iterations cost nothing and
 * no host round trip is needed to stop them.  nullptr disables. */
int tacex_fem_set_newton_early_exit(tacex_fem_ctx* ctx, double* dx_dev, double dx_tol);

/* One projected-Newton iteration per env: assemble (block-Jacobi + coarse-grid preconditioned, tacex_fem_set_coarse_space) system, matrix-free PCG
 * (US:70-72 tol_rate: the PCG stops when r^T M^-1 r <= tol_rate x b^T M^-1 b - libuipc's own test, LinearPCG::pcg `abs(rz_new) <=
 * global_tol_rate * rz0`: relative on r.z itself, i.e. sqrt(tol_rate) on the M^-1 norm), backtracking line search on the energy (US:76: max_iter 8; when the capped search finds no decrease
 * the step is halved further, down to 2^-32, instead of leaving the env stuck).  x_dev is updated in place.
 * stats_dev (B,4) float64 = [energy_before, energy_after, step_length, pcg_iterations]. */
int tacex_fem_newton_step(tacex_fem_ctx* ctx, double* x_dev, const double* x_tilde_dev,
                          const uint8_t* constrained_dev, const double* aim_dev, double* stats_dev,
                          void* workspace_dev, int num_envs, int pcg_max_iter, double pcg_tol_rate,
                          int ls_max_iter, void* stream);

/* One backward-Euler time step of every env - what `world.advance()` does for the gelpad (US:250-252) - with NO host round trip:
 *   x_prev = x;  x_tilde = x + dt v + dt^2 gravity;  up to max_newton Newton iterations (as tacex_fem_newton_step), each env leaving
 *   the loop on the device once the UNSCALED Newton direction of an iteration has max |d| <= velocity_tol * dt (US:62-66; IPC's
 *   test on the search direction, whatever the CCD bound and the line search made of the step);
 *   v = (x - x_prev) / dt.
 * x_dev, v_dev (B,V,3) f64 are updated in place, x_tilde_dev (B,V,3) is written.  With the CU-resident Newton kernel (one thread per
 * vertex: 512 threads per env for meshes of <= 512 vertices, 768 threads for larger ones as long as the env's state fits the CU's
 * 160 KB of LDS - about 600 vertices with friction, 745 without; simple_axle.msh, 593 vertices / 2 003 tets, does with friction; the
 * wide variant takes analytic indenters only and is not available with tacex_fem_set_deterministic) the whole loop is ONE launch; the streaming fallback
 * (any vertex count; analytic indenters - and since ABI 17 mesh indenters - with barrier, step bound and - ABI 11 - friction lagged at the
 * step's start; block-Jacobi PCG) launches
 * max_newton kernels on a fixed schedule in which converged envs return at once.  stats_dev (B,4) = [energy_before, energy_after, step_length, pcg_iterations] of the LAST iteration
 * run; step_info_dev (B,4) f64 = [newton_iterations, max |d| of the last iteration, flags, pcg_iterations_total] (both kernels: the fallback
 * sums / ORs over its launches), flags: 1 = a contact vertex was at or beyond its indenter's surface when an iteration started
 * (the caller moved the indenter by more than the gap: that vertex gets no restoring force), 2 = a line search found no decrease;
 * informational: 4 = the env dropped the coarse correction for the rest of the step (its stopping test passed with the residual's
 * 2-norm above |b|: no reduction at all), 8 = its PCG met negative curvature and iterations of the step were solved with the PSD-safe Hessian
 * (|c_J| of the Stable Neo-Hookean d2J/dF2 term clamped per element; the gradient is exact, the minimiser the same); 32 (ABI 17) = the
 * env's kind-4 row named a mesh id outside the indenter mesh library (tacex_fem_set_indenter_mesh_ids): it had no indenter; 64 (ABI 19)
 * = the env's material id lay outside the material library (tacex_fem_set_material_ids): it stepped with material 0.
 * workspace_dev: tacex_fem_workspace_bytes(ctx, num_envs). */
int tacex_fem_step(tacex_fem_ctx* ctx, double* x_dev, double* v_dev, double* x_tilde_dev, const uint8_t* constrained_dev,
                   const double* aim_dev, double* stats_dev, double* step_info_dev, void* workspace_dev, int num_envs,
                   const double gravity[3], int max_newton, double velocity_tol, int pcg_max_iter, double pcg_tol_rate,
                   int ls_max_iter, void* stream);

/* ---- The reference's own UIPC scene: a FREE affine-body ball on a ground plane under the gelpad (second slice) --------
 * Replaces, for `UipcObjectCfg(constitution_cfg=AffineBodyConstitutionCfg())` next to the gelpad
 * (scripts/benchmarking/tactile_sim_performance/envs/ball_rolling_uipc.py:71-92; source/tacex_uipc/tacex_uipc/objects/uipc_object.py:62-74,
 * 456-466: `AffineBodyConstitution().apply_to(mesh, m_kappa * MPa, mass_density)`, kinematic = False) and `ground(ground_height,
 * ground_normal)` + the default contact model (source/tacex_uipc/tacex_uipc/sim/uipc_sim.py:192-201), what libuipc's
 * `world.advance()` does with them.  libuipc is not in the reference tree: the model is oracle/abd_oracle.py's (PARITY UNPINNED) -
 * Lan et al. 2022 (affine body: q = (p, A), mass matrix S (x) I_3 from the surface mesh's moments, orthogonality energy
 * kappa vol |A^T A - I|^2), Li et al. 2020 (barrier on every point-triangle pair closer than d_hat, pad vertex / ball triangle AND
 * ball vertex / pad triangle, ground against the surface vertices of both bodies), additive CCD on the pairs, and lagged Coulomb
 * friction of EVERY contact (pairs of both kinds and ground contacts of both bodies; ratio and stick tolerance from tacex_fem_set_friction,
 * US:103-124: the contacts of the state the step starts from are frozen - normal force, normal, barycentric weights - and slide
 * relative to it, Li et al. 2020 section 5.4).  EDGE-EDGE pairs (every pad surface edge against every ball edge closer than d_hat:
 * segment-segment distance, weight = the mean of the two edges' areas, IPC's mollifier m(|e_a x e_b|^2) with threshold
 * 1e-3 |e_a|^2 |e_b|^2 at rest, Li et al. 2020 eq. 24) complete IPC's contact set; tacex_fem_set_edge_edge(ctx, 0) switches that pair kind
 * off (on after tacex_fem_set_affine_body).
 *
 * tacex_fem_set_affine_body: ONE body per env, the same mesh for all envs.  verts_host (num_verts,3) f64 in the body frame, tris_host
 * (num_tris,3) outward oriented; density [kg/m^3]; kappa [Pa] (m_kappa * 1e6); pad_vertex_area_host (V) contact weights of the gelpad's
 * vertices (0: interior) and pad_tris_host (num_pad_tris,3) its surface triangles; d_hat [m], stiffness [J/m^2] as tacex_fem_set_contact;
 * the ground is the half-space z >= ground_height (enable_ground = 0: none); kinematic = 1 (`AffineBodyConstitutionCfg.kinematic`,
 * uipc_object.py:70-73, 463-466 `is_fixed`): the body's twelve unknowns are FIXED within a step - the caller moves q_dev between steps
 * and the pad feels the body through the pairs and their friction.  num_verts = 0 removes the body.  Tables are copied.
 * State: q_dev / qv_dev (num_envs,4,3) f64 = (p, c_1, c_2, c_3) with c_k = COLUMN k of A (a surface point is p + sum_k X_k c_k) and its
 * velocity.  tacex_fem_ball_step = one backward-Euler step of pad + ball: predictor (gravity on the pad vertices and on p), the whole
 * Newton loop in one launch (PCG preconditioned by 3x3 blocks on the pad and the exact 12x12 ball block; an env leaves the loop once
 * the unscaled direction has max |d| <= velocity_tol * dt on the position rows AND <= transrate_tol * dt on the affine rows,
 * uipc_sim.py:62-66), velocities.  step_info (num_envs,4) = [Newton iterations, max |d|, flags (1 a surface vertex at / below the
 * ground, 2 line search failed, 16 a candidate list overflowed), PCG iterations].  workspace: tacex_fem_ball_workspace_bytes.
 * tacex_fem_ball_terms: energy (num_envs) and gradient (num_envs, V + 4, 3) of the step's incremental potential at (x, q) against the
 * predictors (x_tilde, q_tilde) - the entry point the parity tests compare with the oracle term by term.  x_prev_dev / q_prev_dev
 * (both or neither): the state friction slides relative to; the friction lag (forces, normals, weights) is then taken at (x, q) itself.
 * tacex_fem_ball_moments: the 4x4 moment matrix S (row-major) and kappa * vol the library derived from the mesh. */
int tacex_fem_set_affine_body(tacex_fem_ctx* ctx, int num_verts, const double* verts_host, int num_tris, const int32_t* tris_host, double density,
                              double kappa, const double* pad_vertex_area_host, int num_pad_tris, const int32_t* pad_tris_host, double d_hat,
                              double stiffness, double ground_height, int enable_ground, int kinematic);
int tacex_fem_set_edge_edge(tacex_fem_ctx* ctx, int enable);
/* Line search of tacex_fem_ball_step: after a backtracking (halving) search that had to cut the step, `bisections` more energy evaluations
 * between the accepted and the last rejected step keep the LARGEST step that still does not increase the incremental potential.  A cut step
 * was cut by a pair entering the barrier zone (contact resistance 10 GPa against a 0.1 MPa gel: micrometres inside cost more than the step
 * gains); the accepted half usually leaves that pair just outside d_hat, where it has no curvature for the next iteration either, which is cut
 * again - the larger step takes it inside, into the next Hessian.  Same acceptance rule (E <= E0 on a CCD-feasible step), same minimiser;
 * default 4 (bench scene: worst env of a step 4.4 -> 3.1 Newton iterations, 135 K -> 178 K frames/s per 512-env shard), 0 = plain halving. */
int tacex_fem_set_line_search_refine(tacex_fem_ctx* ctx, int bisections);
size_t tacex_fem_ball_workspace_bytes(const tacex_fem_ctx* ctx, int num_envs);
int tacex_fem_ball_moments(const tacex_fem_ctx* ctx, double moments_out[16], double* kappa_vol_out);
int tacex_fem_ball_terms(tacex_fem_ctx* ctx, const double* x_dev, const double* x_tilde_dev, const double* q_dev, const double* q_tilde_dev,
                         const uint8_t* constrained_dev, const double* aim_dev, const double* x_prev_dev, const double* q_prev_dev,
                         double* energy_dev, double* grad_dev, double* step_info_dev, void* workspace_dev, int num_envs, void* stream);
int tacex_fem_ball_step(tacex_fem_ctx* ctx, double* x_dev, double* v_dev, double* q_dev, double* qv_dev, const uint8_t* constrained_dev,
                        const double* aim_dev, double* step_info_dev, void* workspace_dev, int num_envs, const double gravity[3], int max_newton,
                        double velocity_tol, double transrate_tol, int pcg_max_iter, double pcg_tol_rate, int ls_max_iter, void* stream);

/* Per-env reset of the FEM state - what `UipcObject.reset(env_ids)` / `write_vertex_positions_to_sim(vertex_positions, env_ids)`
 * (source/tacex_uipc/tacex_uipc/objects/uipc_object.py:280-370; `reset` is a TODO stub there, the write ignores env_ids) are for: an
 * RL task puts ONE env's gelpad back while the others go on.  For every env of env_ids_dev (num_reset,) int32 (NULL: all num_envs):
 *   x <- positions_dev (num_reset, V, 3) f64 when given, else the rest positions of tacex_fem_create;   v <- 0;
 *   step_info row <- 0 (nullable);   the indenter position the friction displacement of the NEXT tacex_fem_step is measured from
 *   <- none (the env's next step sees no sliding, like the first step of a fresh scene, wherever its indenter is put meanwhile).
 * Nothing else of the solver survives a time step (friction lag, warm start, lagged preconditioner blocks and x_prev are rebuilt
 * by every tacex_fem_step), so the next step of a reset env is bit-identical to the first step of a fresh context in deterministic
 * mode.  workspace_dev: the workspace tacex_fem_step runs with (nullable before the first step).  Enqueued on `stream`. */
int tacex_fem_reset_envs(tacex_fem_ctx* ctx, const int32_t* env_ids_dev, int num_reset, const double* positions_dev, double* x_dev,
                         double* v_dev, double* step_info_dev, void* workspace_dev, int num_envs, void* stream);

/* The affine body's part of a per-env reset (ABI 18): q[env] <- q0_dev (4,3) f64, qv[env] <- 0 for the listed envs (env_ids_dev NULL:
 * all).  For a KINEMATIC body, the pose its next step measures the body's motion from (the end of the previous step, kept in
 * ball_workspace_dev) becomes q0 as well, so friction sees no motion in that step, like the first step of a fresh scene; the other
 * envs keep theirs.  Enqueued on `stream`. */
int tacex_fem_ball_reset_envs(tacex_fem_ctx* ctx, const int32_t* env_ids_dev, int num_reset, const double* q0_dev, double* q_dev,
                              double* qv_dev, void* ball_workspace_dev, int num_envs, void* stream);

/* Contact forces of the ball scene (tacex_fem_set_affine_body) at the state x_dev (num_envs, V, 3), q_dev (num_envs, 4, 3): the pairs
 * between pad and body (pad vertex x body triangle, body vertex x pad triangle, pad edge x body edge unless tacex_fem_set_edge_edge
 * switched them off), the ground under both, and IPC's lagged friction of all of them - tacex_fem_ball_step's own terms evaluated once,
 * in one launch.  A force on a state row is -(1 / dt^2) d/d row of the term's share of the incremental potential, in newtons, world
 * frame.  A pair is active when it is closer than d_hat and its weight is positive; lam = -kappa w m b'(d / d_hat) / d_hat >= 0.
 * Friction (with_friction != 0): the lagged contacts are the active pairs and ground contacts of the state the last step STARTED from -
 * x_prev / q_prev of ball_workspace_dev, or x_prev_dev (num_envs, V, 3) / q_prev_dev (num_envs, 4, 3) when given (both or neither; they
 * override the workspace's rows: the entry the parity tests use, like tacex_fem_ball_terms) - with lam, normal and coefficients frozen
 * there; the force is -mu lam f1(|u|) / |u| u on every row, u the tangential relative displacement since that state, mu and
 * eps_velocity * dt the context's (tacex_fem_set_friction).  A kinematic body's rows slide from the pose the last step measured the body's
 * motion from (where it stood when the step before ended; that step's first with its workspace: no motion), which tacex_fem_ball_step
 * leaves in the workspace: the friction reported is what the step balanced.  An env put back by tacex_fem_ball_reset_envs reports zero friction
 * until it steps.  Friction ratio 0: valid zeros.  Refused (2, with a message): a context without a body, null x / q / record, one of
 * x_prev_dev / q_prev_dev alone, with_friction with neither explicit previous states nor the workspace and num_envs of the context's last
 * tacex_fem_ball_step.
 * record_dev (num_envs, 44) f64 - forces act ON THE BODY NAMED FIRST:
 *   0..2   pad <- body: sum of the barrier forces on the pad rows (the mollifier's term of nearly parallel edge pairs included)
 *   3..5   pad <- body: sum of the friction forces of the pair contacts on the pad rows
 *   6..8   torque of 0..5 on the pad, sum (x_row - ref) x f_row
 *   9      sum lam over the active pairs         10  number of active pairs        11  flags (0, or 16: a candidate list overflowed)
 *   12..14 centre of pressure sum lam_k c_k / sum lam_k, c_k the pad-side closest point (the reference point when sum lam = 0)
 *   15     smallest distance over the active pairs (+inf: none)      16..18 active pairs of kind 0 / 1 / 2      19  0
 *   20..31 body: generalised contact force on its 12 rows (p, c_1, c_2, c_3): pairs + their friction + ground + ground friction
 *   32..34 body <- ground: friction (x, y) and normal (z) force
 *   35 / 36 / 37 sum lam, count and smallest gap of the body's ground contacts (+inf: none)
 *   38..40 pad <- ground force     41 / 42 count and smallest gap of the pad's ground contacts (+inf: none)     43  0
 * Slots 0..9 and 12..15 mean what they mean in tacex_fem_contact_forces' record.  ref_points_dev (num_envs, 3): the torque's reference
 * point per env (NULL: the origin).  vertex_force_dev (num_envs, V, 3), nullable: the total contact force of every pad vertex (pairs,
 * their friction, ground, ground friction).  Candidates are culled as in the step (lists of 512 per env in LDS); an overflow sets flag
 * 16 and the sums then miss contacts - nothing is written out of bounds.  List slots are handed out with atomics: results agree to
 * round-off from run to run and batch to batch, not bit for bit.  Enqueued on `stream`.  The call was added without a change of
 * TACEX_ABI_VERSION (no existing signature or struct moved): a caller detects it by looking the symbol up, not by the version. */
int tacex_fem_ball_contact_forces(tacex_fem_ctx* ctx, const double* x_dev, const double* q_dev,
                                  const void* ball_workspace_dev /* nullable */, const double* x_prev_dev /* nullable */,
                                  const double* q_prev_dev /* nullable */, const double* ref_points_dev /* (B,3), nullable: origin */,
                                  int with_friction, double* record_dev /* (B,44) */, double* vertex_force_dev /* (B,V,3), nullable */,
                                  int num_envs, void* stream);

/* Attachment animation (UA:364-428: `_compute_aim_positions` + the animator callback `animate_tet` UA:365-385) for all envs:
 *   aim_position[b, idx[a]] = R(body_quat[b]) * offsets[a] + body_pos[b];  is_constrained[b, idx[a]] = 1
 * body_pos_dev (B,3) / body_quat_dev (B,4 wxyz) float32 pose of the rigid body the gelpad is attached to (IsaacLab root / link
 * state), offsets_dev (A,3) float32 attachment offsets in the body frame (UA:293-297), idx_dev (A,) int32 vertex ids.
 * The rotation is evaluated in float32 like IsaacLab's transform_points (UA:411-413) and widened to float64 on store.
 * aim_compact_dev (B,A,3) float64 optionally receives the same positions densely (the reference's `self.aim_positions`). */
int tacex_fem_set_attachment_targets(const float* body_pos_dev, const float* body_quat_dev, const float* offsets_dev,
                                     const int32_t* idx_dev, double* aim_position_dev, uint8_t* is_constrained_dev,
                                     double* aim_compact_dev, int num_envs, int num_attachment_points, int num_verts,
                                     void* stream);

/* FEM-driven markers (VT:347-366): barycentric surface points -> pinhole projection.
 *   surf_pos_dev (B,Vs,3) surface vertex positions in the CAMERA frame, tri_dev (M,3) int32 vertex ids,
 *   weight_dev (M,3) float64, intrinsics fx,fy,cx,cy (VT:57-63: 340,325,160,125) -> uv_dev (B,M,2) float64 */
int tacex_fem_marker_uv(const double* surf_pos_dev, const int32_t* tri_dev, const double* weight_dev,
                        double fx, double fy, double cx, double cy, double* uv_dev, int num_envs,
                        int num_surf_verts, int num_markers, void* stream);

/* gen_marker_flow's per-step part for a static marker grid (VT:354-413: no random rotation / translation / shift / noise / lost
 * tracking - the shipped cfgs) in ONE launch: the FEM state's surface vertices -> camera frame (VT:142-187) -> barycentric point ->
 * pinhole projection of all markers, then the step's subset next to its initial projection.
 *   x_dev (B,V,3) f64 world positions (the FEM state itself); surf_ids_dev (Vs) int64: global vertex id of every surface vertex;
 *   cam_pos_dev (B,3), cam_rot_inv_dev (B,3,3) row-major: camera-frame point = cam_rot_inv (x - cam_pos); tri_dev (M,3) int32 SURFACE-local
 *   vertex ids and weight_dev (M,3) f64 per marker; init_uv_dev (B,M,2) the projections of the reference surface; select_dev (K) int64: the
 *   markers of this step's subset (VT:394-399, drawn by the caller); normalize_div > 0: values / normalize_div - 1 (VT:407-409), 0: pixels.
 *   Outputs: curr_uv_dev (B,M,2) f64 (nullable) all current projections; flow_dev (B,2,K,2) f64 and / or flow_f32_dev (B,2,K,2) f32:
 *   [initial | current] (u, v) of the subset. */
int tacex_fem_marker_flow(const double* x_dev, const int64_t* surf_ids_dev, const double* cam_pos_dev, const double* cam_rot_inv_dev,
                          const int32_t* tri_dev, const double* weight_dev, double fx, double fy, double cx, double cy,
                          const double* init_uv_dev, const int64_t* select_dev, double normalize_div, double* curr_uv_dev, double* flow_dev,
                          float* flow_f32_dev, int num_envs, int num_verts, int num_markers, int num_selected, void* stream);

/* gen_marker_flow with the whole randomisation interface of VT:354-413 (random grid, lost tracking, noise, random subset) for a batch in
 * ONE launch, every env on a marker pattern and a random stream of its own: a MARKER PATTERN LIBRARY.
 *   Library (built once by the caller): num_patterns = P >= 1 patterns, pattern k = the k-th draw of the marker grid with its triangles and
 *   barycentric weights: lib_tri_dev (P,Mmax,3) int32 SURFACE-local vertex ids, lib_weight_dev (P,Mmax,3) f64, lib_count_dev (P) int32;
 *   rows >= count[k] are padding and never read.  max_markers = Mmax <= 1024 (one env's markers are staged in LDS).
 *   pattern_ids_dev (B) int32, read at every launch (a task re-draws an env's pattern by writing it in place); an id outside [0, P) reads
 *   pattern 0.  draws_dev (B) uint32: the env's draw number t; the kernel uses it and stores t + 1.  Writing it back reproduces a draw.
 *   Per env e with k = pattern_ids[e], t = draws[e]:
 *   1. every marker m < count[k]: initial (u, v) from ref_surf_cam_dev (B,Vs,3; the reference surface in the camera frame) with the
 *      arithmetic of tacex_fem_marker_uv, current (u, v) from x_dev with the arithmetic of tacex_fem_marker_flow - bit-equal to both;
 *   2. in-image mask on the env's own initial projection: 5 < u < image_height and 5 < v < image_width (sic: the reference's axis swap);
 *   3. lost tracking: m survives iff U > lose_probability;
 *   4. noise: sigma * N added to init u, init v, current u, current v of every survivor (four independent normals), before normalisation;
 *   5. selection among the n survivors, K = num_selected: n >= K: the survivor whose (key, m) pair has rank r < K in ascending order goes
 *      to slot r (a uniform K-subset in random order); 0 < n < K: the survivors in marker order, padded by repeating the last; n = 0: zeros;
 *      then values / normalize_div - 1 if normalize_div > 0, the zero case included;
 *   6. outputs: flow_dev (B,2,K,2) f64 and / or flow_f32_dev (B,2,K,2) f32 (at least one); curr_uv_dev (B,Mmax,2) f64 [nullable]: all
 *      current projections, noise-free, rows >= count zero; num_tracked_dev (B) int32 [nullable] = n;
 *   7. draws[e] = t + 1.
 *   Random numbers: Philox4x32-10 (tacex_philox4x32), key (seed & 0xffffffff, seed >> 32), counter (m, stream, e, t).
 *     stream 0: word 0 -> U, word 1 -> subset key;  stream 1: words (0,1) -> Box-Muller pair for (init u, init v), (2,3) -> (current u, v).
 *     uniform of a word w = (w + 0.5) * 2^-32 in f64; Box-Muller of (a, b) = sqrt(-2 ln a) cos(2 pi b), sqrt(-2 ln a) sin(2 pi b) in f64.
 *   The draws of an env depend on (seed, e, t, m) alone - not on B, the other envs or the launch shape; a sharded job gives every rank
 *   its own seed.
 * Returns 2 before any HIP call for NULL arguments, P < 1, Mmax outside [1, 1024], lose_probability outside [0, 1], negative sigma. */
int tacex_fem_marker_flow_library(const double* x_dev, const int64_t* surf_ids_dev, const double* cam_pos_dev, const double* cam_rot_inv_dev,
                                  const double* ref_surf_cam_dev, const int32_t* lib_tri_dev, const double* lib_weight_dev,
                                  const int32_t* lib_count_dev, int num_patterns, int max_markers, const int32_t* pattern_ids_dev,
                                  uint32_t* draws_dev, uint64_t seed, double fx, double fy, double cx, double cy, double lose_probability,
                                  double sigma, int image_height, int image_width, double normalize_div, double* curr_uv_dev,
                                  double* flow_dev, float* flow_f32_dev, int32_t* num_tracked_dev, int num_envs, int num_verts,
                                  int num_surf_verts, int num_selected, void* stream);

/* Philox4x32-10 (Random123 constants and round function) on the HOST: the function the marker kernel calls, so that a CPU test pins the
 * generator.  ctr (4), key (2) -> out (4) uint32. */
int tacex_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* Sensor camera model: what a GelSight's camera does to the rendered frame - a per-unit colour response, pixel-to-pixel gain
 * differences (fixed pattern), read and shot noise, 8-bit quantisation - applied to rgb_dev (B,H,W,3) f32 in ONE launch on `stream`
 * (tacex_amd/csrc/camera_model.hip).  B = num_frames, any H, W >= 1; inputs are finite.
 *   out_dtype 0: out_dev is (B,H,W,3) f32 in [0,1]; out_dev == rgb_dev (in place) is allowed and gives the same image.
 *   out_dtype 1: out_dev is (B,H,W,3) uint8 = floor(255 v + 0.5).
 * All arithmetic is float32, every operation rounded on its own (no fused multiply-add), in the order written below.
 * Profiles: profiles_dev (P,16) f32, P = num_profiles.  Row: [0..8] colour matrix M row-major, [9..11] offset o, [12] read-noise sigma
 *   `read` (in units of full scale), [13] shot coefficient s (variance = s * signal), [14] fixed-pattern sigma_f, [15] reserved, written 0.
 *   Frame b uses row profile_ids_dev[b] ((B,) int32; NULL: row 0 for every frame).  An id outside [0, P) is the identity profile
 *   (M = I, everything else 0): the output is the clamped input.
 * Draws: the pixels of a frame are taken in row-major order in groups of four; group g holds pixels 4g .. 4g+3 (the last group of a
 *   frame may be partial).  Sample j = 3 p + c of a group (pixel p of the group, channel c) takes word j % 4 of Philox4x32-10
 *   (tacex_philox4x32) with key (seed & 0xffffffff, seed >> 32) and counter (g, j / 4, frame_offset + b, call).  The draw is the
 *   integer d = (sum of the word's four bytes) - 510: mean exactly 0, variance exactly 4 (256^2 - 1) / 12 = 21845, bounded at +-3.45
 *   standard deviations, no transcendental function.  S = float32(1 / sqrt(21845.0)).  The fixed-pattern draw d_f is the same with
 *   counter (g, 4 + j / 4, frame_offset + b, 0): it does not depend on `call`.
 * Per pixel (r, g, b) and output channel c:
 *     a = ((M[c][0]*r + M[c][1]*g) + M[c][2]*b) + o[c]
 *     if sigma_f != 0:  a = a * (1 + (sigma_f*S) * float(d_f))
 *     a = min(max(a, 0), 1)
 *     sig = sqrtf(read*read + s*a)
 *     v = a + (sig*S) * float(d)
 *     v = min(max(v, 0), 1)
 *     out = v (out_dtype 0)   or   (uint8) floorf(255*v + 0.5f) (out_dtype 1)
 * An image depends on (seed, frame_offset + b, call, profile) alone - not on B, the other frames or the launch shape: a shard of
 * envs passes its first global env index as frame_offset and renders the frames the whole batch would.
 * Returns 2 before any HIP call for a NULL rgb_dev, profiles_dev or out_dev, num_profiles <= 0, num_frames, height or width <= 0,
 * an out_dtype other than 0 or 1, out_dtype 1 with out_dev == rgb_dev, and a batch beyond one launch (2^31 - 1 workgroups). */
int tacex_camera_model(const float* rgb_dev, const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev,
                       uint64_t seed, uint32_t frame_offset, uint32_t call, void* out_dev, int out_dtype, int num_frames, int height,
                       int width, void* stream);

/* HOST: the 12 integer draws d (fixed_pattern 0) or d_f (fixed_pattern != 0; `call` is ignored) of group `group` of frame
 * `frame` (= frame_offset + b) - the function the kernel calls, compiled for the host, so that a CPU test pins the draws. */
int tacex_camera_noise_draw(uint64_t seed, uint32_t frame, uint32_t call, uint32_t group, int fixed_pattern, int32_t out[12]);

/* Sensor lens model: what the short wide-angle lens of a GelSight and the mounting of one unit do to the rendered frame - radial
 * and tangential (Brown-Conrady) distortion, a mounting shift, rotation, scale and shear against the pad, vignetting, and a
 * softness that grows towards the corners - applied to rgb_dev (B,H,W,3) f32 as ONE gather on `stream`
 * (tacex_amd/csrc/lens_model.hip) into out_dev (B,H,W,3) f32.  B = num_frames, any H, W >= 1; inputs are finite.  Any (B,H,W,3)
 * f32 image goes through it (tactile_rgb, a marker overlay).  The stage sits between tactile_rgb and tacex_camera_model.
 * All arithmetic is float32, every operation rounded on its own (no fused multiply-add), in the order written below; the kernel
 * has no division and no transcendental function.  min / max are C's fminf / fmaxf (a NaN operand gives the other operand).
 * Profiles: profiles_dev (P,16) f32, P = num_profiles.  Row:
 *     [0] k1  [1] k2  [2] p1  [3] p2  [4] e00  [5] e01  [6] e10  [7] e11  [8] tx  [9] ty  [10] cx  [11] cy  [12] v1  [13] v2  [14] b0  [15] b2
 *   k1, k2: radial and p1, p2: tangential distortion coefficients in normalised units (1 = half the frame's width); with the
 *   formulas below a negative k1 pulls the source position of a corner pixel towards the centre, a positive one pushes it outwards;
 *   E = A - I: the mounting rotation, scale and shear A minus identity; (tx, ty): the mounting shift [px];
 *   (cx, cy): the optical centre's offset from the frame centre [px]; v1, v2: vignetting; b0, b2: softness [source px].
 *   Frame b uses row profile_ids_dev[b] ((B,) int32; NULL: row 0 for every frame).  An id outside [0, P) is the identity profile:
 *   the all-zero row.
 * Constants, float32: s = 2.0f / float(W) (the one division, on the host), hw = float(W) * 0.5f, hh = float(H) * 0.5f.
 * Output pixel (row i, column j), with jf = float(j), if = float(i):
 *     px = ((jf + 0.5) - hw) - cx              py = ((if + 0.5) - hh) - cy
 *     xn = px*s   yn = py*s   xx = xn*xn   yy = yn*yn   xy = xn*yn   r2 = xx + yy
 *     rad = (k1 + k2*r2) * r2
 *     dx = (xn*rad + (p1 + p1)*xy) + p2*(r2 + (xx + xx))
 *     dy = (yn*rad + p1*(r2 + (yy + yy))) + (p2 + p2)*xy
 *     ou = ((e00*px + e01*py) + hw*dx) + tx    ov = ((e10*px + e11*py) + hw*dy) + ty
 *     u = jf + ou   v = if + ov                 the source position [source px; pixel (i, j) is at (u, v) = (j, i)]
 *   Softness: if b0 == 0 and b2 == 0:  colour = tap(u, v)
 *     otherwise  hs = 0.5 * min(max(b0 + b2*r2, 0), 4),  um = u - hs, up = u + hs, vm = v - hs, vp = v + hs,
 *                colour = (((tap(um, vm) + tap(up, vm)) + tap(um, vp)) + tap(up, vp)) * 0.25    per channel
 *   tap(u, v), bilinear with edge replicate:
 *     a u or v that is not finite is replaced by 0
 *     x0f = floorf(u)  fx = u - x0f  gx = 1 - fx        y0f = floorf(v)  fy = v - y0f  gy = 1 - fy
 *     x0 = int(min(max(x0f, -1), float(W)))  x1 = x0 + 1, both then clamped to [0, W-1]; y0, y1 likewise with H
 *     with a = rgb[y0][x0], b = rgb[y0][x1], c = rgb[y1][x0], d = rgb[y1][x1]:   (a*gx + b*fx)*gy + (c*gx + d*fx)*fy    per channel
 *   Vignetting: g = min(max(1 + (v1 + v2*r2)*r2, 0), 1),   out = g * colour    per channel
 * The identity profile returns the input bit for bit (u = jf exactly, a tap with zero fractions is (a*1 + b*0)*1 + (..)*0, g = 1;
 * only a -0 comes out as +0).  A frame depends on its own input and profile alone - not on B or the other frames.
 * Returns 2 before any HIP call for a NULL rgb_dev, profiles_dev or out_dev, num_profiles < 1, num_frames, height or width <= 0,
 * out_dev == rgb_dev (a gather cannot run in place - unlike tacex_camera_model), and height x width >= 2^31 or a batch beyond
 * one launch (2^31 - 1 workgroups). */
int tacex_lens_model(const float* rgb_dev, const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev, float* out_dev,
                     int num_frames, int height, int width, void* stream);

/* tacex_lens_model followed by tacex_camera_model on the gathered colour, in ONE launch: out_dev equals
 * tacex_camera_model(tacex_lens_model(rgb)) bit for bit, for out_dtype 0 (f32) and 1 (uint8).  The lens arguments are those of
 * tacex_lens_model (lens_profiles_dev (PL,16), lens_profile_ids_dev), the others those of tacex_camera_model; the Philox
 * counter is addressed by the group of four consecutive OUTPUT pixels.  Returns 2 for what either of the two refuses
 * (out_dev == rgb_dev for both dtypes). */
int tacex_lens_camera_model(const float* rgb_dev, const float* lens_profiles_dev, int num_lens_profiles, const int32_t* lens_profile_ids_dev,
                            const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev, uint64_t seed,
                            uint32_t frame_offset, uint32_t call, void* out_dev, int out_dtype, int num_frames, int height, int width,
                            void* stream);

/* Points (markers) moved the way tacex_lens_model moves the image.  xy_dev (B,N,2) f64, N = num_points, in ideal image pixels
 * (x = column, y = row - the convention of marker_motion; a point at (x, y) lies on the centre of pixel (i, j) = (y, x)):
 * out_dev (B,N,2) f64 is where the lens of frame b's profile shows the point; out_dev may be xy_dev.
 * The image kernel maps output -> source, a point needs the inverse: with the real-valued displacement (ou, ov)(qx, qy) of the
 * formulas above (jf = qx, if = qy) evaluated in FLOAT64 (the f32 profile row widened, s = 2.0 / double(W), the same order of
 * operations), q solves q + displacement(q) = (x, y) by fixed-point iteration from q = (x, y):
 *     q <- (x, y) - displacement(q),   TACEX_LENS_POINT_ITERATIONS = 24 times, no convergence test.
 * (The iteration contracts by the displacement's Jacobian norm, about 3 |k1| r2 + 5 |k2| r2^2 + |E|: a third per round in the
 * corner of a 4:3 frame at k1 = -0.15, where the first guess is 30 px off on 320 columns - below 1e-9 px after 24 rounds.)
 * Returns 2 before any HIP call for NULL xy_dev, profiles_dev or out_dev, num_profiles < 1, num_frames, num_points, height or
 * width <= 0. */
#define TACEX_LENS_POINT_ITERATIONS 24
int tacex_lens_points(const double* xy_dev, const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev, double* out_dev,
                      int num_frames, int num_points, int height, int width, void* stream);

/* Contact force field of the optical path: an elastic-foundation (Winkler) contact model with regularised Coulomb shear, evaluated
 * per pixel of the height map and reduced per env and per cell of a coarse tactile grid, in ONE launch on `stream`
 * (tacex_amd/csrc/contact_field.hip).  B = num_frames, any H, W >= 1.  All per-pixel operations are float32, each rounded on its own
 * (no fused multiply-add), in the order written; sums are float64, in an order fixed by (H, W) alone and without atomics: the same
 * input gives the same bits, and an env's outputs do not depend on the batch it is evaluated in.
 * Inputs: hm_mm_dev (B,H,W) f32 height map [mm]; frame_min_dev (B,) f32 its per-frame minimum and indent_mm_dev (B,) f32 the
 *   indentation depth [mm], as tacex_height_map_from_depth / tacex_indentation_depth leave them;
 *   gels_dev (P,4) f32, P = num_gels, row [k_n, k_t, mu, 0] with k_n, k_t in Pa/mm, all >= 0; frame b uses row gel_ids_dev[b]
 *   ((B,) int32; NULL: row 0).  An id outside [0, P): every output of the env is zero (the whole record too);
 *   slip_dev (B,5) f32 [dx_mm, dy_mm, dtheta_rad, cx_px, cy_px]: the object's motion over the pad since first contact, about the
 *   pixel (cx, cy); NULL: all zero (no shear anywhere);
 *   pixmm: pixel pitch [mm]; a = float32(double(pixmm)^2 * 1e-6) is a pixel's area [m^2].
 * Per pixel (row i, column j):
 *     S = (hm - frame_min) - indent                      (TT:441)
 *     d = S < 0 ? -S : 0                                 [mm]; a NaN gives 0
 *     p = k_n * d                                        [Pa]
 *   and, where d > 0 (everything below is 0 / false where d == 0):
 *     rx = (float(j) - cx) * pixmm,  ry = (float(i) - cy) * pixmm
 *     ux = dx - dtheta * ry,  uy = dy + dtheta * rx,  n = sqrtf(ux*ux + uy*uy)
 *     slips = k_t*n >= mu*p
 *     s = min(k_t*n, mu*p) / n,  tx = ux * s,  ty = uy * s       (tx = ty = 0 where n == 0)
 *   traction on the pad in the camera frame (x = columns, y = rows, z = optical axis): (tx, ty, -p) [Pa] - the layout and sign of
 *   tacex_traction_image_from_deformed_mesh; force of the pixel: fx = tx*a, fy = ty*a, fn = p*a, (fx, fy, -fn) [N].
 * record_dev (B,16) f64.  With the float64 sums over the frame's pixels (float32 terms widened to float64; products with i, j formed in float64)
 *   and (cx0, cy0) = ((W-1)/2, (H-1)/2), m = double(pixmm) * 1e-3:
 *   [0..2] (sum fx, sum fy, -sum fn) [N];
 *   [3..5] torque about the image centre on the pad face, sum r x f with r = ((j-cx0) m, (i-cy0) m, 0) [N m]:
 *          [3] = -(sum fn*i - cy0 sum fn) m,  [4] = (sum fn*j - cx0 sum fn) m,
 *          [5] = ((sum fy*j - cx0 sum fy) - (sum fx*i - cy0 sum fx)) m;
 *   [6] Fn = sum fn;  [7] contact area = count * double(a) [m^2];  [8] count of pixels with d > 0;
 *   [9], [10] centre of pressure (x, y) = (sum p*j, sum p*i) / sum p [px]; (cx0, cy0) when sum p == 0;
 *   [11] largest d [mm];  [12] penetrated volume = (sum d) * double(pixmm)^2 [mm^3];  [13] count of slipping pixels;
 *   [14] principal-axis angle 0.5 atan2(2 m11, m20 - m02) of the pressure distribution, with x = [9], y = [10] and
 *        m20 = sum p*j*j / sum p - x*x, m02 = sum p*i*i / sum p - y*y, m11 = sum p*j*i / sum p - x*y [px^2]; 0 when sum p == 0;
 *   [15] sqrt(max(l_min, 0) / l_max), l = (m20+m02)/2 -+ sqrt(((m20-m02)/2)^2 + m11^2); 0 when sum p == 0 or l_max <= 0.
 * cells_dev (B,grid_rows,grid_cols,3) f32, nullable: the force (sum fx, sum fy, -sum fn) [N] on every cell of a grid laid over the
 *   image, summed in float64 and rounded once; pixel (i, j) belongs to cell ((i*grid_rows)/H, (j*grid_cols)/W) (integer division).
 *   The cells of an env sum to [0..2].
 * image_dev (B,H,W,3) f32 [Pa], nullable: (tx, ty, -p) of every pixel; when given, every pixel is written.
 * frame_rows_dev (B,4) int32, nullable: the contact rectangles [row lo, row hi, column lo, column hi] that
 *   tacex_height_map_from_depth / tacex_indentation_depth produce for THESE height maps (nothing outside one has S < 0).  Only the
 *   rectangle is read; every output is bit-equal to the call without it, and a frame with an empty rectangle reads no pixel.
 *   (The rectangle is clamped to the image: it can skip pixels, never address outside the frame.)
 * 16-byte loads along rows are used when hm_mm_dev (and image_dev) are 16-byte aligned and W % 4 == 0; the result is the same bits
 * otherwise.  One workgroup handles one frame and keeps 8 rows of pixel forces and of per-cell runs in LDS: about
 * 8 (12 W + 24 grid_cols c) bytes with c = ceil(ceil(W / grid_cols) / 32) (none when cells_dev is NULL).
 * Returns 2 before any HIP call for a NULL hm_mm_dev, frame_min_dev, indent_mm_dev, gels_dev or record_dev, num_gels <= 0,
 * num_frames, height or width <= 0, pixmm <= 0 (or NaN), grid_rows outside [1, height] or grid_cols outside [1, width] (checked
 * with or without cells_dev), and a width / grid_cols pair that needs more than 128 KiB of LDS. */
int tacex_contact_field(const float* hm_mm_dev, const float* frame_min_dev, const float* indent_mm_dev, const float* gels_dev,
                        int num_gels, const int32_t* gel_ids_dev, const float* slip_dev, float pixmm, const int32_t* frame_rows_dev,
                        int grid_rows, int grid_cols, double* record_dev, float* cells_dev, float* image_dev, int num_frames,
                        int height, int width, void* stream);

/* Gel memory of the optical path: the viscoelastic residual imprint of the elastomer.  The height map of this step is rewritten in
 * place from per-pixel state that remembers past contact, per env, in ONE launch on `stream` (tacex_amd/csrc/gel_memory.hip).
 * B = num_frames, K = terms (1 or 2 Prony branches, fixed for the life of a state buffer), any H, W >= 1.  All operations are
 * float32, each rounded on its own (no fused multiply-add), in the order written.
 *   hm_mm_dev (B,H,W) f32 height map [mm], rewritten in place;  state_dev (B,K,H,W) f32, the branch states m_k, zero after a reset;
 *   live_dev (B,) int32; coef_dev (P,8) f32, P = num_profiles, row [a1, c1, a2, c2, floor_mm, 0, 0, 0]; frame b uses row
 *   profile_ids_dev[b] ((B,) int32; NULL: row 0).  An id outside [0, P) is the all-zero row: the map stays as it is and the frame's
 *   state becomes zero.  The host computes, in float64 and then rounded to float32, a_k = exp(-dt / tau_k) (0 when tau_k == 0) and
 *   c_k = (1 - a_k) w_k from a profile's time constants tau_k [s], weights w_k >= 0 with w_1 + w_2 <= 1 and the step dt > 0.
 *   z0_mm = float32((gelpad_to_camera_min_distance + gelpad_height) * 1000), sum and product in double: the pad's rest plane [mm].
 * Per pixel:
 *     t = z0 - hm,  d = t > 0 ? t : 0                     penetration [mm]; a NaN gives 0
 *     m_k' = (a_k * m_k) + (c_k * d)                      k = 1..K: two products and a sum, three roundings
 *     if d == 0 and m_k' < floor_mm:  m_k' = 0            (the state returns to exactly zero after a release)
 *     M = m_1' (K = 1),  m_1' + m_2' (K = 2);  r = z0 - M
 *     hm' = r  if M > 0 and r < hm,  else hm              the imprint never lifts a pixel
 *   live'[b] = 1 if and only if a state element of frame b is non-zero after the call, else 0.
 * A frame that enters with live == 0 and has no pixel with d > 0 is left as it is by these statements (zero state, unchanged map):
 * the kernel moves no state byte for it and leaves live at 0.  live must therefore be 1 for a frame whose state is not all zero.
 * With sum w <= 1 the imprint is never deeper than the deepest past press; held at d0 for n steps and released for j, a pixel
 * shows M = sum_k w_k d0 (1 - a_k^n) a_k^j.
 * Outputs besides hm, state and live: frame_min_dev (B,) f32, indent_mm_dev (B,) f32 and frame_rows_dev (B,4) int32 (nullable) are
 * exactly what tacex_indentation_depth(hm', gelpad_height_m, gelpad_to_camera_min_distance_m, ...) writes for the rewritten map, for
 * every geometry (where W % 4 != 0 or H > 2048 the ranges are the whole frame, as there).
 * One workgroup per frame and no atomics between workgroups: the same inputs give the same bits on every call, alone or in a batch.
 * 16-byte loads and stores where W % 4 == 0 (hm_mm_dev and state_dev must then be 16-byte aligned), 4-byte ones otherwise.
 * Returns 2 before any HIP call for a NULL hm_mm_dev, state_dev, live_dev, coef_dev, frame_min_dev or indent_mm_dev, terms not 1 or
 * 2, num_profiles, num_frames, height or width <= 0, and misaligned buffers at W % 4 == 0. */
int tacex_gel_memory(float* hm_mm_dev, float* state_dev, int32_t* live_dev, const float* coef_dev, int num_profiles,
                     const int32_t* profile_ids_dev, float z0_mm, float gelpad_height_m, float gelpad_to_camera_min_distance_m,
                     float* frame_min_dev, float* indent_mm_dev, int32_t* frame_rows_dev, int num_frames, int height, int width,
                     int terms, void* stream);

/* Relief tile library as a height-map source: every env presses its own tile of a library - a height field sampled bilinearly, on a
 * flat, spherical or cylindrical carrier, under a pose the caller writes in place - into hm_mm_dev (B,H,W) f32 [mm] in ONE launch on
 * `stream` (tacex_amd/csrc/relief_source.hip); frame minimum, indentation depth and contact ranges of the map come out of the same
 * launch.  B = num_frames.  The projection is orthographic, as in tacex_height_map_from_indenters, and the relief is displaced along
 * the optical axis: a height field without undercuts.  All operations are float32, each rounded on its own (no fused multiply-add),
 * in the order of the parentheses.
 * Library: texels_dev f32, all tiles back to back, each row-major; a texel is the relief height [mm] standing proud of the carrier,
 *   -inf means "no material here" (NaN and +inf are refused by the host layer);
 *   tiles_i_dev (P,4) int32, P = num_tiles, row [first texel, rows Th, cols Tw, wrap 0/1];
 *   tiles_f_dev (P,4) f32, row [pitch_mm, top_mm, u0, v0]: the texel pitch, the largest finite texel of the tile, and the anchor in
 *   texel coordinates - the carrier's origin, by default the tile centre ((Tw-1)/2, (Th-1)/2);
 *   relief_ids_dev (B,) int32, read on the device (NULL: tile 0 for every frame); an id outside [0, P) gives far clip everywhere and
 *   the library is not read (like kind < 0 of tacex_height_map_from_indenters).
 * Pose: pose_dev (B,16) f32, written in place by the caller between steps:
 *     [0..5] m00 m01 m02 m10 m11 m12   [6] press_mm   [7..9] t0 tx ty   [10] carrier   [11] radius_mm R   [12] gain   [13] du  [14] dv
 *     [15] 0
 *   M maps a pixel to texel coordinates; press_mm is how far the relief's highest point sits below the gel top where the carrier is 0;
 *   (t0, tx, ty) tilt the whole object [mm, mm/px]; carrier 0 plane, 1 sphere, 2 cylinder with its axis along the tile's u (any other
 *   value: plane); gain scales the relief (>= 0); (du, dv) scroll the texture against the carrier [texels] (rolling).
 * Per sample at x = column, y = row as float32:
 *     u = ((m00*x) + (m01*y)) + m02            v = ((m10*x) + (m11*y)) + m12
 *     s = (u - u0)*pitch                        t = (v - v0)*pitch                 object frame [mm]
 *     plane:    c = 0
 *     sphere:   q = (s*s) + (t*t);   c = q <= R*R ? R - sqrtf(max(R*R - q, 0)) : +inf
 *     cylinder: q = t*t;             the same expression
 *     uu = u + du;  vv = v + dv
 *     if !(|uu| < 2^30 && |vv| < 2^30):  h = -inf
 *     else  fu = floorf(uu), fv = floorf(vv), a = uu - fu, b = vv - fv, i0 = (int)fu, j0 = (int)fv
 *       wrap:     i0, i0+1, j0, j0+1 taken modulo Tw / Th (non-negative modulo)
 *       no wrap:  outside 0 <= uu <= float(Tw-1) or 0 <= vv <= float(Th-1):  h = -inf;  otherwise i0 = min(i0, Tw-1),
 *                 i1 = min(i0+1, Tw-1), j0 and j1 likewise with Th
 *       with h00 = texel[j0][i0], h01 = texel[j0][i1], h10 = texel[j1][i0], h11 = texel[j1][i1]:
 *       h = (((h00*(1-a)) + (h01*a))*(1-b)) + (((h10*(1-a)) + (h11*a))*b)
 *     depth = (((gel_top - press) + c) + (gain*(top - h))) + ((t0 + (tx*x)) + (ty*y))
 *     d = depth < far_clip ? depth : far_clip                                       a NaN gives far clip
 *   A sample that touches a -inf texel is no material (0 * -inf = NaN: far clip); a sample whose carrier is +inf is far clip and
 *   reads no texel.
 * samples (a host argument) 1: hm = d at (x, y) = (column, row).  samples 4: hm = ((d0 + d1) + (d2 + d3)) * 0.25 of the clamped
 *   values d at (x-0.25, y-0.25), (x+0.25, y-0.25), (x-0.25, y+0.25), (x+0.25, y+0.25), in this order: the anti-aliasing for stamp
 *   edges and for tiles finer than the pixel.
 * Outputs besides hm: frame_min_dev (B,) f32, indent_mm_dev (B,) f32 (nullable) and frame_rows_dev (B,4) int32 (nullable) are
 *   exactly what tacex_indentation_depth(hm, gelpad_height_m, gelpad_to_camera_min_distance_m, ...) writes for that map (without
 *   indent_mm_dev the ranges are those of a press depth of 0).
 * One workgroup per frame and no atomics between workgroups: the same inputs give the same bits on every call, alone or in a batch.
 * Texel indices are 32-bit: the library holds fewer than 2^31 texels.
 * Returns 2 before any HIP call, writing nothing, for a NULL texels_dev, tiles_i_dev, tiles_f_dev, pose_dev, hm_mm_dev or
 * frame_min_dev, num_tiles, num_frames, height or width <= 0, width % 4 != 0, height or width above 2048, samples not 1 or 4, and an
 * hm_mm_dev that is not 16-byte aligned.  The call was added without a change of TACEX_ABI_VERSION (no existing signature or struct
 * moved): a caller detects it by looking the symbol up, not by the version. */
int tacex_height_map_from_relief(const float* texels_dev, const int32_t* tiles_i_dev, const float* tiles_f_dev, int num_tiles,
                                 const int32_t* relief_ids_dev, const float* pose_dev, float gel_top_mm, float far_clip_mm,
                                 float gelpad_height_m, float gelpad_to_camera_min_distance_m, float* hm_mm_dev, float* frame_min_dev,
                                 float* indent_mm_dev, int32_t* frame_rows_dev, int num_frames, int height, int width, int samples,
                                 void* stream);

/* Signed-distance volume library as a height-map source: every env presses its own volume of a library - a grid of signed distances
 * sampled trilinearly and sphere-traced along the optical axis, under a full rigid pose, uniform scale and iso level the caller
 * writes in place - into hm_mm_dev (B,H,W) f32 [mm] (tacex_amd/csrc/volume_source.hip).  B = num_frames.  Two launches on
 * `stream`: the marching kernel, then the kernel of tacex_indentation_depth on the map it wrote.  The projection is orthographic, as
 * in tacex_height_map_from_indenters: a pixel's camera-frame point is X = column*pixmm, Y = row*pixmm, Z = depth [mm].  All
 * operations are float32, each rounded on its own (no fused multiply-add), in the order of the parentheses; 1/v is the correctly
 * rounded quotient; "c ? a : b" with a NaN in c's comparison takes b.
 * Library: voxels_dev f32 (num_voxels), all grids back to back, each (D,Hv,Wv) with index order z, y, x; a voxel is the signed
 *   distance [object mm] at that grid point, negative inside (the host layer refuses non-finite values);
 *   volumes_i_dev (P,4) int32, P = num_volumes, row [first voxel, D, Hv, Wv];
 *   volumes_f_dev (P,8) f32, row [pitch_mm, i0, j0, k0, step_scale, 0, 0, 0]: the voxel pitch, the anchor - the voxel coordinates
 *   (x, y, z) of the object frame's origin, by default the grid centre ((Wv-1)/2, (Hv-1)/2, (D-1)/2) - and the factor in (0, 1]
 *   that shortens every step (for fields that are only a lower bound of the distance);
 *   volume_ids_dev (B,) int32, read on the device (NULL: volume 0 for every frame).
 * Pose: pose_dev (B,16) f32, written in place by the caller between steps:
 *     [0..8] R row-major, object -> camera   [9..11] tx ty tz [mm]   [12] scale   [13] level_mm   [14] [15] 0 (not read)
 *   A camera point P lies at o = R^T (P - t) / scale in the object frame, at q = o / pitch + anchor in voxel coordinates; the
 *   surface is {sdf = level}: a positive level inflates the object.
 * Per frame (from the pose row r[0..15] and the volume row), with N = (Wv, Hv, D), anchor = (i0, j0, k0) and a = 0, 1, 2 the
 * object axes x, y, z:
 *     g = scale*pitch          inv = 1/g          vox = g                                  one voxel pitch in camera mm
 *     ax[a] = (r[a]*pixmm)*inv     ay[a] = (r[3+a]*pixmm)*inv     az[a] = r[6+a]*inv
 *     q0[a] = anchor[a] - ((((r[a]*tx) + (r[3+a]*ty)) + (r[6+a]*tz))*inv)
 *     par[a] = !(|az[a]| >= 1e-12f)          ia[a] = par[a] ? 0 : 1/az[a]          hmax[a] = float(N[a] - 1)
 *   The frame is FAR CLIP EVERYWHERE, and the library is not read, when the id is outside [0, P); when the volume row has
 *   first < 0, an axis < 2 or first + D*Hv*Wv > num_voxels; or unless g > 0, step_scale > 0, |level| < 2^30 and all twelve of
 *   |ax[a]|, |ay[a]|, |az[a]|, |q0[a]| < 2^30 (a NaN or inf in the pose fails these).
 * Per pixel at x = column, y = row as float32:
 *     b[a] = (q0[a] + (x*ax[a])) + (y*ay[a])                                              q[a](z) = b[a] + (z*az[a])
 *   clipping, starting from lo = near_clip, hi = far_clip, for a = 0, 1, 2 in turn:
 *     par[a]:   the interval is empty unless b[a] >= 0 && b[a] <= hmax[a]
 *     else      t1 = (0 - b[a])*ia[a];  t2 = (hmax[a] - b[a])*ia[a];  tn = t1 < t2 ? t1 : t2;  tf = t1 < t2 ? t2 : t1
 *               lo = tn > lo ? tn : lo;   hi = tf < hi ? tf : hi
 *   The pixel is far clip, and reads no voxel, when the interval is empty, unless lo <= hi, or unless all |b[a]| < 2^30.
 *   marching:  z = lo;  for n = 0 .. max_steps-1:
 *     tap at z: for each a  c = q[a](z);  c = c > 0 ? c : 0;  c = c < hmax[a] ? c : hmax[a];  m[a] = min((int)floorf(c), N[a]-2);
 *               w[a] = c - float(m[a])          (the upper neighbour m[a]+1 stays in the grid)
 *       with v[dz][dy][dx] = voxel[first + ((m[2]+dz)*Hv + (m[1]+dy))*Wv + (m[0]+dx)] and lerp(p, q, t) = p + (t*(q - p)):
 *       x then y then z:  e[dz][dy] = lerp(v[dz][dy][0], v[dz][dy][1], w[0]);  f[dz] = lerp(e[dz][0], e[dz][1], w[1]);
 *       s = lerp(f[0], f[1], w[2])
 *     d = ((s - level)*scale)*step_scale
 *     if d < tol_mm:  depth = z, done            (also a ray that enters its interval inside the object: cut flat by box or near clip)
 *     z = z + d                                  (d >= tol_mm here: the step is max(d, tol_mm))
 *     if !(z <= hi):  depth = far_clip, done     (the ray left its interval; a NaN ends here)
 *     if n == max_steps-1:  depth = d < vox ? z : far_clip          the grazing-ray rule: the last tap was within one voxel
 *   hm = depth < far_clip ? depth : far_clip
 * Outputs besides hm: frame_min_dev (B,) f32, indent_mm_dev (B,) f32 (nullable) and frame_rows_dev (B,4) int32 (nullable) are
 *   exactly what tacex_indentation_depth(hm, gelpad_height_m, gelpad_to_camera_min_distance_m, ...) writes for that map - its
 *   kernel runs as the second launch (without indent_mm_dev the ranges are those of a press depth of 0).
 * A workgroup marches a 32 x 8 tile of one frame (four waves of 16 x 4 neighbouring pixels), no atomics and no dependence on the
 * batch: the same inputs give the same bits on every call, alone or in a batch.  Voxel indices are 32-bit (num_voxels < 2^31),
 * offsets into hm 64-bit.
 * Returns 2 before any HIP call, writing nothing, for a NULL voxels_dev, volumes_i_dev, volumes_f_dev, pose_dev, hm_mm_dev or
 * frame_min_dev, num_voxels, num_volumes, num_frames, height or width <= 0, width % 4 != 0, height or width above 2048, more
 * tiles than one launch takes, pixmm not > 0, max_steps outside 1..128, tol_mm not > 0, near_clip_mm >= far_clip_mm (or a NaN),
 * and an hm_mm_dev that is not 16-byte aligned.  The call was added without a change of TACEX_ABI_VERSION (no existing signature
 * or struct moved): a caller detects it by looking the symbol up, not by the version. */
int tacex_height_map_from_sdf(const float* voxels_dev, int num_voxels, const int32_t* volumes_i_dev, const float* volumes_f_dev,
                              int num_volumes, const int32_t* volume_ids_dev, const float* pose_dev, float pixmm, float near_clip_mm,
                              float far_clip_mm, int max_steps, float tol_mm, float gelpad_height_m,
                              float gelpad_to_camera_min_distance_m, float* hm_mm_dev, float* frame_min_dev, float* indent_mm_dev,
                              int32_t* frame_rows_dev, int num_frames, int height, int width, void* stream);

/* Scenes of signed-distance volumes as a height-map source: every env holds K = num_slots (1..8) SLOTS, each a volume of the library of
 * tacex_height_map_from_sdf under its own pose, folded into one field by union, subtraction and intersection during the march
 * (tacex_amd/csrc/sdf_scene.hip).  Library, projection, float32 arithmetic ("each operation rounded on its own, in the order of the
 * parentheses"), clip planes, max_steps, tol_mm, the outputs besides hm and the two launches are those of tacex_height_map_from_sdf;
 * sqrt is the correctly rounded root.  The caller writes three tensors in place between steps:
 *   part_ids_dev (B,K) int32: the slot's volume;   part_ops_dev (B,K) int32: 0 union, 1 subtract, 2 intersect;
 *   part_pose_dev (B,K,16) f32: the pose row of tacex_height_map_from_sdf, with [14] blend_mm (>= 0) and [15] 0 (not read).
 * Per slot: g, inv, vox, ax, ay, az, q0, par, ia, hmax as in tacex_height_map_from_sdf from the slot's pose row and volume row, and
 *   blend = r[14].  The slot is EMPTY - the library is not read for it - when its id is outside [0, P), its op outside 0..2, unless
 *   |blend| < 2^30, or when the volume row or the pose fail the checks of tacex_height_map_from_sdf.
 *   vox_env = the smallest vox over the env's non-empty union slots (2^30 when there is none).
 * Per 32 x 8 TILE of the frame (tile column tc, tile row tr) a non-empty slot is LIVE when its op is intersect, or when the image of
 * its grid's box meets the tile: over the eight corners c (bit 0, 1, 2 of c choose 0 or hmax[a] on axis a = 0, 1, 2)
 *     o[a] = (corner[a] - anchor[a])*vox     X = (((r[0]*o[0]) + (r[1]*o[1])) + (r[2]*o[2])) + tx     Y likewise with r[3..5], ty
 *     xmin, xmax, ymin, ymax: the smallest and largest X and Y;     margin = blend > 0 ? pixmm + blend : pixmm
 *     x0 = float(32*tc)*pixmm   x1 = float(32*tc + 31)*pixmm   y0 = float(8*tr)*pixmm   y1 = float(8*tr + 7)*pixmm
 *     live = xmax + margin >= x0 && xmin - margin <= x1 && ymax + margin >= y0 && ymin - margin <= y1
 *   (a union or subtraction whose box is further than its blend width from every ray of the tile cannot be hit there; an
 *   intersection with a part that is absent leaves nothing, so it is never dropped).  Slots that are not live do not exist for the
 *   tile's pixels.  A tile without a live union slot is far clip, and reads no voxel.
 * Per pixel and live slot s: b_s[a] as b[a] in tacex_height_map_from_sdf, and [lo_s, hi_s] by its clipping from lo = near_clip,
 *   hi = far_clip; meets_s = the interval is not empty, lo_s <= hi_s and all |b_s[a]| < 2^30.
 *   The pixel's interval is lo = the smallest lo_s, hi = the largest hi_s over the live UNION slots with meets_s; without one the
 *   pixel is far clip and reads no voxel.  Subtract and intersect slots never extend it.
 * The field f at depth z is a left fold over the live slots in slot order, from f = 2^30:
 *     q[a] = b_s[a] + (z*az[a]);  c[a], m[a], w[a] and the tap s(c) at the clamped point as in tacex_height_map_from_sdf;  x[a] = q[a] - c[a]
 *     inside = meets_s && z >= lo_s && z <= hi_s
 *     inside:   u = ((s(c) - level)*scale)*step_scale
 *     else      e2 = (((x[0]*x[0]) + (x[1]*x[1])) + (x[2]*x[2]))*(vox*vox)                    squared distance to the box [mm^2]
 *               p = ((s(c) - level)*scale)*step_scale;  p = p > 0 ? p : 0;  u = sqrt(e2 + (p*p))
 *       (for a surface inside its convex box a lower bound of the distance: |P-Q|^2 >= |P-C|^2 + |C-Q|^2 for the projection C of P;
 *       equal to the tap on the faces up to rounding, growing with the distance from the box)
 *     min(a, b) = b < a ? b : a;     smin_k(a, b) = min(a, b), and for k > 0:
 *               t = k - |a - b|;  t = t > 0 ? t : 0;  h = t/k;  smin_k(a, b) = min(a, b) - ((h*h)*(k*0.25f))
 *     union: f = smin_blend(f, u)     subtract: f = -smin_blend(-f, u)     intersect: f = -smin_blend(-f, -u)
 *   (A union slot with blend not > 0 that is not inside and has sqrt(e2) >= f cannot change f; the kernel skips its tap.)
 * marching:  z = lo;  for n = 0 .. max_steps-1:
 *     if f(z) < tol_mm:  depth = z, done
 *     z = z + f(z)
 *     if !(z <= hi):  depth = far_clip, done
 *     if n == max_steps-1:  depth = f(z before the step) < vox_env ? z : far_clip                          the grazing-ray rule
 *   hm = depth < far_clip ? depth : far_clip
 * A scene whose only non-empty slot is slot 0, a union with blend 0, gives the bits of tacex_height_map_from_sdf for that volume and
 * pose in hm, frame_min, indent and the ranges: the one slot is live wherever a ray meets its box, every marched point is inside
 * (z stays in [lo_s, hi_s]), and min(2^30, u) takes the steps u takes.
 * All three operations are 1-Lipschitz in 1-Lipschitz arguments, so the march never steps past the folded surface.  No atomics and
 * no dependence on the batch: the same inputs give the same bits on every call, alone or in a batch.
 * Returns 2 before any HIP call, writing nothing, for a NULL voxels_dev, volumes_i_dev, volumes_f_dev, part_ids_dev, part_pose_dev,
 * part_ops_dev, hm_mm_dev or frame_min_dev, num_voxels, num_volumes, num_frames, height or width <= 0, num_slots outside 1..8,
 * width % 4 != 0, height or width above 2048, more tiles than one launch takes, pixmm not > 0, max_steps outside 1..128, tol_mm not
 * > 0, near_clip_mm >= far_clip_mm (or a NaN), and an hm_mm_dev that is not 16-byte aligned.  The call was added without a change of
 * TACEX_ABI_VERSION (no existing signature or struct moved): a caller detects it by looking the symbol up, not by the version. */
int tacex_height_map_from_sdf_scene(const float* voxels_dev, int num_voxels, const int32_t* volumes_i_dev, const float* volumes_f_dev,
                                    int num_volumes, const int32_t* part_ids_dev, const float* part_pose_dev, const int32_t* part_ops_dev,
                                    int num_slots, float pixmm, float near_clip_mm, float far_clip_mm, int max_steps, float tol_mm,
                                    float gelpad_height_m, float gelpad_to_camera_min_distance_m, float* hm_mm_dev, float* frame_min_dev,
                                    float* indent_mm_dev, int32_t* frame_rows_dev, int num_frames, int height, int width, void* stream);

/* tacex_height_map_from_sdf_scene, and which slot every pixel shows: the same arguments, contract, launches and bits in hm_mm_dev,
 * frame_min_dev, indent_mm_dev and frame_rows_dev (the same kernel source, instantiated with the owner), plus
 *   part_map_dev (B,H,W) uint8, not NULL: the OWNER of every pixel, a slot index 0..K-1, or 255 where hm is far_clip.
 * The owner follows the comparison inside smin at every fold.  In every evaluation of f(z):
 *     own = 255
 *     for every live slot s in slot order that is evaluated (one that the rule "a union slot with blend not > 0 that is not inside
 *     and has sqrt(e2) >= f" skips is not), with f the value BEFORE the fold and u the slot's value:
 *         union:      if u < f:    own = s          (smin_blend(f, u) takes its second argument)
 *         subtract:   if u < -f:   own = s          (smin_blend(-f, u))
 *         intersect:  if -u < -f:  own = s          (smin_blend(-f, -u))
 *     the same rule with blend > 0 and without.  s is the slot's index in 0..K-1, not its position among the tile's live slots.
 *   part_map = own of the evaluation that assigned the pixel's depth - the one with f(z) < tol_mm, or the last one where the
 *   grazing-ray rule gave the depth -, and 255 wherever hm == far_clip: a tile without a live union slot, a pixel without an
 *   interval, a ray that hit nothing, a depth >= far_clip.
 * So the owner is the part one sees: of a union the nearer part, of a subtraction the wall of the cut, of an intersection the
 * clipping part.  One byte per pixel is stored by the lane that stores the depth; no atomics, no dependence on the batch.
 * Returns 2 before any HIP call, writing nothing, for what tacex_height_map_from_sdf_scene refuses and for a NULL part_map_dev.
 * Added without a change of TACEX_ABI_VERSION: a caller detects it by looking the symbol up. */
int tacex_height_map_from_sdf_scene_parts(const float* voxels_dev, int num_voxels, const int32_t* volumes_i_dev, const float* volumes_f_dev,
                                          int num_volumes, const int32_t* part_ids_dev, const float* part_pose_dev,
                                          const int32_t* part_ops_dev, int num_slots, float pixmm, float near_clip_mm, float far_clip_mm,
                                          int max_steps, float tol_mm, float gelpad_height_m, float gelpad_to_camera_min_distance_m,
                                          float* hm_mm_dev, float* frame_min_dev, float* indent_mm_dev, int32_t* frame_rows_dev,
                                          uint8_t* part_map_dev, int num_frames, int height, int width, void* stream);

/* Per-part contact records: tacex_contact_field with a LABEL per pixel, one slip row and one record per (frame, label), in ONE launch on
 * `stream` (tacex_amd/csrc/contact_parts.hip).  Inputs, per-pixel float32 operations, float64 sums, gel table, pixmm, frame_rows_dev and
 * the 16 record slots are those of tacex_contact_field; there are no cells.  L = num_labels (1..8).
 *   labels_dev (B,H,W) uint8: the pixel's label, e.g. the part map of tacex_height_map_from_sdf_scene_parts;
 *   slip_dev (B,L,5) f32: a slip row [dx_mm, dy_mm, dtheta_rad, cx_px, cy_px] per label; NULL: all zero.
 * Per pixel: S, d, p as in tacex_contact_field; where d > 0 and the label l is < L, the shear (tx, ty) and `slips` with the slip row
 *   (b, l).  A pixel whose label is >= L has no shear (tx = ty = 0, slips = false) and enters no record: e.g. where the gel memory
 *   leaves an imprint and no part was hit.
 * record_dev (B,L,16) f64: record (b, l) holds the slots of tacex_contact_field over the pixels of label l alone - the same sums,
 *   the same torque origin (the image centre), the same values for a label without pressure ([9], [10] the image centre, [14], [15]
 *   zero).  An id outside the gel table: all L records of the env and its image are zero.
 * image_dev (B,H,W,3) f32 [Pa], nullable: (tx, ty, -p) of every pixel, (0, 0, -p) where the label is >= L; every pixel is written.
 * Sums are float64 in an order fixed by (H, W) alone, without atomics; a record does not depend on the batch, on the other labels'
 * slip rows, on frame_rows_dev being given, or on the alignment of image_dev.  With L = 1, every label 0 and slip_dev (B,1,5) holding
 * the rows of a (B,5) table, record_dev[:,0] and image_dev are the bits of tacex_contact_field with that table.
 * 16-byte loads are used when W % 4 == 0, hm_mm_dev is 16-byte and labels_dev 4-byte aligned; the same bits otherwise.
 * Returns 2 before any HIP call for a NULL hm_mm_dev, frame_min_dev, indent_mm_dev, gels_dev, labels_dev or record_dev, num_gels,
 * num_frames, height or width <= 0, num_labels outside 1..8, pixmm <= 0 (or NaN).  Added without a change of TACEX_ABI_VERSION. */
int tacex_contact_field_parts(const float* hm_mm_dev, const float* frame_min_dev, const float* indent_mm_dev, const float* gels_dev,
                              int num_gels, const int32_t* gel_ids_dev, const uint8_t* labels_dev, int num_labels, const float* slip_dev,
                              float pixmm, const int32_t* frame_rows_dev, double* record_dev, float* image_dev, int num_frames, int height,
                              int width, void* stream);

/* Contact point cloud of the optical path: a fixed-size set of K = max_points surface points per env, sampled from the contact pixels
 * of the height map, in ONE launch on `stream` (tacex_amd/csrc/contact_points.hip): a stream compaction, no atomics, no global
 * scratch, no host synchronisation.  B = num_frames, any H, W >= 1 with H * W < 2^31.
 * Inputs: hm_mm_dev (B,H,W) f32, frame_min_dev (B,) f32 and indent_mm_dev (B,) f32 exactly as for tacex_contact_field;
 *   frame_rows_dev (B,4) int32, nullable: the contact rectangles [row lo, row hi, column lo, column hi] of THESE height maps, as in
 *   tacex_contact_field.  Pixels are looked for inside the rectangle only (clamped to the image: it can skip pixels, never address
 *   outside the frame); every output is bit-equal to the call without it, and a frame with an empty rectangle reads no pixel.  (The
 *   gradient of a selected pixel taps its four neighbours wherever they lie.)
 *   labels_dev (B,H,W) u8, nullable: a label per pixel, e.g. the part map of tacex_height_map_from_sdf_scene_parts;
 *   label: -1 selects every label (255 too), 0..254 only the pixels whose label equals it; label >= 0 with a NULL labels_dev is refused;
 *   pixmm > 0: pixel pitch [mm];  min_depth_mm >= 0;  max_points K in [1, 16384];  pad: 0 = zero fill, 1 = repeat;
 *   pose_dev (B,12) f32, nullable: a row-major [R | t] per env (row r is R[r][0], R[r][1], R[r][2], t[r]);  unit f32 > 0: the length
 *   unit of the points in mm^-1 (1e-3: metres);  jitter 0 / not 0, seed u64, frame_offset i64, call u32: below.
 * Per pixel (row i, column j):
 *     S = (hm - frame_min) - indent
 *     d = S < 0 ? -S : 0                                 [mm]; a NaN gives 0
 *   The pixel is a CONTACT PIXEL iff d > min_depth_mm and it passes the label filter.  With min_depth_mm == 0 and no labels this is
 *   the pixel set of tacex_contact_field (its record slot [8] is N).
 * Rank: the N contact pixels of a frame are ranked r = 0..N-1 in row-major order of the whole frame.
 * Slots: with the offset o (0, or the jitter below), slot k of K takes
 *     N > K:                     rank floor((k*N + o) / K) in 64-bit integer arithmetic - strictly increasing in k and below N; a pixel
 *                                of rank r is therefore the source of slot k iff ceil((r*K - o)/N) <= k < ceil(((r+1)*K - o)/N), and
 *                                that range holds at most one slot;
 *     N <= K, pad == 0:          rank k for k < N; the slots beyond are invalid;
 *     N <= K, pad == 1, N > 0:   rank k mod N;
 *     N == 0:                    every slot is invalid.
 * Jitter: w = philox4x32_10(ctr = {lo32(g), hi32(g), call, 0x70747363}, key = {lo32(seed), hi32(seed)})[0] (tacex_philox4x32) with
 *   g = frame_offset + b as a 64-bit two's complement number, and o = (uint64(w) * N) >> 32, which is in [0, N).  Without jitter, or
 *   when N <= K, o = 0.  A subsample then starts at another rank on every call, env and seed; the ranks stay evenly spaced.
 * Point of a slot whose pixel is (i, j).  All arithmetic is float32, every operation rounded on its own (no fused multiply-add):
 *     x = (float(j) - cx0) * pixmm,  y = (float(i) - cy0) * pixmm,  z = S,   with cx0 = float(W-1) / 2, cy0 = float(H-1) / 2 [mm]
 *   - the camera frame of tacex_contact_field: origin on the pad face at the image centre, x = columns, y = rows, z along the
 *   optical axis, so z is negative under an indenter.
 *   Gradient: jl = max(j-1, 0), jr = min(j+1, W-1), gx = (hm[i,jr] - hm[i,jl]) / (float(jr - jl) * pixmm), gx = 0 when W == 1;
 *     gy likewise along i (gy = 0 when H == 1).  Neighbours need not be in contact.
 *   Normal: s = sqrtf((gx*gx + gy*gy) + 1),  n = (gx / s, gy / s, -1 / s): the indenter surface's normal pointing into the gel.
 *   With pose_dev:    q = (unit*x, unit*y, unit*z),  p'[r] = ((R[r][0]*q[0] + R[r][1]*q[1]) + R[r][2]*q[2]) + t[r],
 *                     n'[r] = (R[r][0]*n[0] + R[r][1]*n[1]) + R[r][2]*n[2]   (not renormalised);
 *   without:          p' = (unit*x, unit*y, unit*z),  n' = n.
 *   The penetration is reported as d [mm], untransformed.
 * Outputs: points_dev (B,K,3) f32, required; each of the following nullable: normals_dev (B,K,3) f32, depth_dev (B,K) f32,
 *   pixels_dev (B,K,2) int32 [row, col], labels_out_dev (B,K) u8 (the pixel's label; 0 when labels_dev is NULL),
 *   count_dev (B,2) int32 [N, V], V the number of valid slots: 0 for N = 0, K for N >= K or pad == 1, N otherwise.
 *   Invalid slots: points, normals and depth 0, pixels -1, labels 255.  Every slot of every given output is written.
 * An env's outputs depend on its own inputs and g alone, not on the batch it is launched in; the same input gives the same bits.
 * One workgroup handles one frame and keeps K pixel indices in LDS (4 K bytes).  16-byte row loads are used when W % 4 == 0,
 * hm_mm_dev is 16-byte aligned (and labels_dev, where the filter reads it, 4-byte aligned); the same bits otherwise.
 * Returns 2 before any HIP call for a NULL hm_mm_dev, frame_min_dev, indent_mm_dev or points_dev, num_frames, height or width <= 0,
 * height * width >= 2^31, pixmm or unit <= 0 (or NaN), min_depth_mm < 0 (or NaN), max_points outside [1, 16384], pad other than 0 or
 * 1, label outside [-1, 254], and label >= 0 with a NULL labels_dev; 2 as well when 4 K bytes exceed the LDS a workgroup can get on
 * the device.  Added without a change of TACEX_ABI_VERSION: a caller detects it by looking the symbol up. */
#define TACEX_CONTACT_POINTS_MAX 16384
int tacex_contact_points(const float* hm_mm_dev, const float* frame_min_dev, const float* indent_mm_dev, const int32_t* frame_rows_dev,
                         const uint8_t* labels_dev, int label, float pixmm, float min_depth_mm, int max_points, int pad,
                         const float* pose_dev, float unit, int jitter, uint64_t seed, int64_t frame_offset, uint32_t call,
                         float* points_dev, float* normals_dev, float* depth_dev, int32_t* pixels_dev, uint8_t* labels_out_dev,
                         int32_t* count_dev, int num_frames, int height, int width, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TACEX_HIP_H */
