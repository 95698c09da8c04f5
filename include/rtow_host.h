/*
 * rtow_host.h — C handle API over the host-side C++ mirror of the reference's construction
 * surface (ray_tracing_in_one_weekend_amd/host/rtow.hpp).  It exists so that non-C++ hosts
 * (the Python/ctypes test and bench harness here; a Rust `extern "C"` block in the reference)
 * can build scenes with the reference's constructors and obtain the RtFlatScene/RtCamera that
 * rt_scene_upload()/rt_render() take (include/rtow_mi355x.h).  No GPU code in this library.
 *
 * Reference interfaces mirrored (paths relative to /root/reference/src):
 *   rth_scene_build     demo_scene.rs:37,229  scene fns `fn(aspect_ratio) -> (HitableList, Camera)`
 *   rth_tex_*           texture.rs:15-17,32-37,156-161,175-181  ConstantTex / CheckerTex::new /
 *                       PerlinTex::new / ImageTex::new
 *   rth_material        material.rs + pbr.rs public-field structs (tag = RtMatType)
 *   rth_sphere          hitable.rs:57-62  Sphere { c, r, mat, name }
 *   rth_set_sky         lib.rs:11 SKY_COLOR.set(..), demo_scene.rs:19 ENV_TEX
 *   rth_set_camera      camera.rs:14-20  Camera::new(lookfrom, lookat, vup, vfov, aspect_ratio)
 *   rth_rng_reseed      lib.rs:8  thread-local SmallRng::seed_from_u64(1995)
 * All functions return 0 / a valid handle on success; on failure they return a negative code /
 * RTH_INVALID and rth_last_error() holds the text (no exception crosses the boundary).
 */
#ifndef RTOW_HOST_H
#define RTOW_HOST_H
#include "rtow_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTH_INVALID 0xFFFFFFFFu

typedef struct RthScene RthScene;

const char* rth_last_error(void);

/* Registers decoded pixels (Rgb<f32> = u8/255, row 0 = top) under the path the scene code
 * passes to ImageTex::new, e.g. "res/earthmap.jpg" (texture.rs:175-181). */
int rth_register_image(const char* path, uint32_t w, uint32_t h, const float* rgb);

/* Re-seeds the thread-local RNG (lib.rs:8; default 1995) that PerlinTex::new draws from. */
void rth_rng_reseed(uint64_t seed);

/* Runs a named scene function: "sphere_scene", "moving_sphere_scene", "quads_scene", "mesh_scene", "test_sphere", "simple_light_scene",
 * "cornell_box", "final_scene", "earth_env_scene", "pbr_sweep_scene"; flattens world + sky + camera.  The thread RNG is reset to its
 * fresh-process state (seed 1995) first, so repeated builds give identical Perlin tables. */
int rth_scene_build(const char* name, float aspect_ratio, RthScene** out);

/* Piecewise construction with the reference's constructors. */
int rth_scene_new(RthScene** out);
uint32_t rth_tex_constant(RthScene* s, const float col[3]);
uint32_t rth_tex_checker(RthScene* s, const float odd[3], const float even[3]);
uint32_t rth_tex_perlin(RthScene* s, float scale);
uint32_t rth_tex_image(RthScene* s, const char* path);
/* type = RtMatType; tex0/tex1 = handles from rth_tex_* or RTH_INVALID; color = Metal albedo;
 * p = the scalar fields in the order documented at RtMatType. */
uint32_t rth_material(RthScene* s, uint32_t type, uint32_t tex0, uint32_t tex1, const float color[3], const float p[4]);
uint32_t rth_sphere(RthScene* s, const float c[3], float r, uint32_t material, const char* name);
/* "The Next Week" chapter 1, MovingSphere::new(center0, center1, radius, material): the centre moves linearly from c0 (time 0) to c1
 * (time 1).  Flattens to the sphere at c0 plus an entry of rth_scene_motion; only at the top level of the world (not below
 * rth_translate / rth_rotate_y, not as a medium boundary: rth_scene_finish fails). */
uint32_t rth_moving_sphere(RthScene* s, const float c0[3], const float c1[3], float r, uint32_t material, const char* name);
/* "The Next Week" chapter 6: the quad Q + a u + b v (0 <= a, b <= 1) and the triangle with the corners a, b, c, stored as Q = a,
 * u = b - a, v = c - a (each rounded to f32 once).  They flatten to entries of rth_scene_quads, in the order the world lists them; only
 * at the top level of the world (not below rth_translate / rth_rotate_y, not as a medium boundary: rth_scene_finish fails). */
uint32_t rth_quad(RthScene* s, const float Q[3], const float u[3], const float v[3], uint32_t material);
uint32_t rth_triangle(RthScene* s, const float a[3], const float b[3], const float c[3], uint32_t material);
/* hitable.rs:244-362 XYRect/XZRect/YZRect { min, max, mat } (axis = RtRectAxis) and hitable.rs:364-383 GBox::new */
uint32_t rth_rect(RthScene* s, uint32_t axis, const float mn[3], const float mx[3], uint32_t material);
uint32_t rth_gbox(RthScene* s, const float mn[3], const float mx[3], uint32_t material);
/* hitable.rs:404-520: wrap the world entry `hitable` in Translate { offset, ptr } / RotateY::new(ptr, angle);
 * the handle stays valid and now denotes the wrapper (wrappers nest, outermost applied last) */
uint32_t rth_translate(RthScene* s, uint32_t hitable, const float offset[3]);
uint32_t rth_rotate_y(RthScene* s, uint32_t hitable, float angle_degrees);
/* hitable.rs:529-533: turn the world entry `hitable` into ConstantMedium::new(hitable, density, phase_tex) */
uint32_t rth_constant_medium(RthScene* s, uint32_t hitable, float density, uint32_t phase_tex);
/* Hitable::bbox (hitable.rs:52) of a world entry, wrappers included: out = {min.xyz, max.xyz}; returns the trait
 * method's bool (1/0), < 0 on a bad handle.  BvhNode::new sorts by it (hitable.rs:163-174). */
int rth_hitable_bbox(RthScene* s, uint32_t hitable, float out[6]);
/* sky = RtSkyType; env_path only for RT_SKY_ENV */
int rth_set_sky(RthScene* s, uint32_t sky, const char* env_path);
int rth_set_camera(RthScene* s, const float lookfrom[3], const float lookat[3], const float vup[3], float vfov,
                   float aspect_ratio);
/* The book's thin-lens camera, Camera::new(lookfrom, lookat, vup, vfov, aspect_ratio, aperture, focus_dist) (chapter 13): the
 * RtCamera is rth_set_camera's bit for bit; rth_scene_lens gives {aperture / 2, focus_dist} for rt_set_lens.  aperture >= 0,
 * focus_dist > 0, both finite. */
int rth_set_camera_lens(RthScene* s, const float lookfrom[3], const float lookat[3], const float vup[3], float vfov,
                        float aspect_ratio, float aperture, float focus_dist);
/* The camera's shutter, after rth_set_camera / rth_set_camera_lens: 0 <= shutter_open <= shutter_close <= 1 (default 0, 1). */
int rth_set_camera_shutter(RthScene* s, float shutter_open, float shutter_close);
/* Wraps everything added so far in a BvhNode like build_bvh (demo_scene.rs:223-227) and flattens. */
int rth_scene_finish(RthScene* s, int use_bvh);

const RtFlatScene* rth_scene_flat(const RthScene* s);
int rth_scene_camera(const RthScene* s, RtCamera* out);
/* The lens of the finished scene's camera: {0, 1} for a pinhole one. */
int rth_scene_lens(const RthScene* s, RtLens* out);
/* The motion of the finished scene for rt_set_motion: its moving spheres (pointers into the scene, valid until rth_scene_free) and the
 * camera's shutter; n_moving 0 for a static scene. */
int rth_scene_motion(const RthScene* s, RtMotion* out);
/* The planar primitives of the finished scene for rt_set_quads (pointers into the scene, valid until rth_scene_free); n 0 for a scene
 * without any. */
int rth_scene_quads(const RthScene* s, RtQuads* out);
/* The light set of the finished scene for rt_set_lights (pointers into the scene, valid until rth_scene_free): the parallelogram of
 * every BARE Emission axis-aligned rectangle and every bare Emission quad, in the order the world lists them; n 0 for a scene without
 * any.  More than RT_MAX_LIGHTS: the first RT_MAX_LIGHTS are kept; *n_found (may be NULL) is how many there were.  Emitters below
 * rth_translate / rth_rotate_y or inside a medium boundary, emissive spheres and emissive triangles are left out (rt_set_lights takes
 * world-space parallelograms only: pass those yourself). */
int rth_scene_lights(const RthScene* s, RtLights* out, uint32_t* n_found);
const char* rth_scene_sphere_name(const RthScene* s, uint32_t index);
void rth_scene_free(RthScene* s);

/* ---- driver conveniences (main.rs:109-128) -------------------------------------------------------------- */

/* Saves rows*nx RGB8 pixels (row 0 = top, i.e. the layout rt_render's out_rgb8 already has after the flip of
 * main.rs:127) as an 8-bit RGB PNG, what `img.save(file_name)` writes at main.rs:121,128.  The file appears
 * atomically (written to <path>.part, then renamed), so it can be polled as a preview. */
int rth_png_write(const char* path, const uint8_t* rgb8, uint32_t nx, uint32_t ny);

/* The reference's output name (main.rs:110-112): local time as RFC 3339 with ':' replaced by '-', cut before the
 * fractional seconds, + ".png", e.g. "2024-05-17T21-03-44.png".  unix_seconds < 0 = now.  buf_len >= 24. */
int rth_output_file_name(int64_t unix_seconds, char* buf, uint32_t buf_len);

#ifdef __cplusplus
}
#endif
#endif
