/*
 * rtow_mi355x.h — C-ABI of the MI355X (gfx950) wavefront path tracer.
 *
 * This is the drop-in boundary for the per-pixel integration loop of
 * zhouhang95/ray_tracing_in_one_weekend.  The reference has no FFI of its own: the seam is
 * the pair (scene builder -> renderer) described in SURVEY.md §8(b).  Every entry point
 * below names the reference interface it replaces (paths relative to /root/reference).
 *
 *   scene side : demo_scene.rs:37,229  fn(aspect_ratio) -> (Vec<Arc<dyn Hitable>>, Camera)
 *                lib.rs:11             SKY_COLOR (global sky fn pointer)
 *   render side: main.rs:77-108        the per-column pixel loop
 *                main.rs:38-60         ray_color (closest hit -> emitted/scatter -> recurse)
 *   output     : main.rs:98-105,127    /spp, gamma 2, *255.99 as u8, vertical flip
 *
 * Conventions
 *   - plain C structs, pointers and sizes; no C++/torch types; no exceptions cross it.
 *   - every function returns 0 on success, a negative RT_ERR_* otherwise; text via
 *     rt_last_error().
 *   - the caller owns all buffers; rt_scene_upload() copies and retains nothing host-side.
 *   - a context (RtCtx) is bound to ONE GPU and is driven by one host thread; multi-GPU sharding is
 *     expressed through RtParams.shard_* (one process per GPU, the host gathers — bench.py does it with
 *     torch.distributed) or handled inside the library by an RtMulti (one process, n GPUs, RCCL gather).
 *   - fp32 throughout; image row 0 is the BOTTOM row in the f32 output (reference `j`
 *     order, main.rs:84) and the TOP row in the RGB8 output (after the flip, main.rs:127).
 */
#ifndef RTOW_MI355X_H
#define RTOW_MI355X_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 11u /* 11: RtFlatScene::med_xform (wrappers around a medium); wrapper chains of any depth, up to RT_MAX_MEDIA = 65 535 media.
                             * 10: rt_prepare; the test hooks moved to rtow_mi355x_debug.h */

/* error codes */
#define RT_OK 0
#define RT_ERR_INVALID (-1)   /* bad argument / inconsistent scene            */
#define RT_ERR_DEVICE (-2)    /* HIP runtime error (text in rt_last_error)   */
#define RT_ERR_NOMEM (-3)     /* host or device allocation failed            */
#define RT_ERR_UNSUPPORTED (-4)
#define RT_ERR_STATE (-5)     /* e.g. render before scene upload             */

/* Material tags.  Order follows SURVEY.md §3.4; one tag per `impl Material`. */
enum RtMatType {
    RT_MAT_EMISSION = 0,         /* material.rs:17-29   tex0 = emit                          */
    RT_MAT_DIFFUSE = 1,          /* material.rs:31-46   tex0 = albedo                        */
    RT_MAT_LAMBERT = 2,          /* material.rs:48-59   tex0 = albedo                        */
    RT_MAT_METAL = 3,            /* material.rs:61-73   color = albedo, p0 = fuzz            */
    RT_MAT_DIELECTRIC = 4,       /* material.rs:75-97   p0 = ior                             */
    RT_MAT_ISOTROPIC = 5,        /* material.rs:99-113  tex0 = albedo                        */
    RT_MAT_OREN_NAYAR = 6,       /* pbr.rs:12-42        tex0 = albedo, p0 = roughness        */
    RT_MAT_BURLEY_DIFFUSE = 7,   /* pbr.rs:45-69        tex0 = albedo, p0 = roughness        */
    RT_MAT_ROUGH_PLASTIC = 8,    /* pbr.rs:153-189      tex0 = spec, tex1 = diff, p0 = roughness, p1 = eta */
    RT_MAT_DISNEY_DIFFUSE = 9,   /* pbr.rs:192-222      tex0 = albedo, p0 = roughness, p1 = subsurface */
    RT_MAT_DISNEY_METAL = 10,    /* pbr.rs:224-278      tex0 = albedo, p0 = roughness, p1 = anisotropic, p2 = rot */
    RT_MAT_DISNEY_SHEEN = 11,    /* pbr.rs:281-308      tex0 = albedo, p0 = tint             */
    RT_MAT_DISNEY_CLEARCOAT = 12,/* pbr.rs:310-335      p0 = clearcoat_gloss                 */
    RT_MAT__COUNT = 13
};

/* Texture tags, one per `impl Texture` (texture.rs). */
enum RtTexType {
    RT_TEX_CONSTANT = 0, /* texture.rs:15-23    color0 = col                                  */
    RT_TEX_CHECKER = 1,  /* texture.rs:25-49    color0 = odd, color1 = even                    */
    RT_TEX_PERLIN = 2,   /* texture.rs:153-168  scale, aux = index of the Perlin table set     */
    RT_TEX_IMAGE = 3,    /* texture.rs:170-193  aux = image index                              */
    RT_TEX__COUNT = 4
};

/* Sky models (demo_scene.rs:22-35; selected through lib.rs:11 SKY_COLOR). */
enum RtSkyType {
    RT_SKY_GRADIENT = 0, /* sky_color      demo_scene.rs:28-31 */
    RT_SKY_BLACK = 1,    /* black_sky      demo_scene.rs:33-35 */
    RT_SKY_ENV = 2       /* tex_sky_color  demo_scene.rs:22-26, image = sky_image */
};

/* Axis-aligned rectangle kinds (hitable.rs:244-362): the axis that is constant on the rectangle.
 * The plane coordinate is min[axis] (the reference reads `self.min.z` etc. and ignores max[axis]). */
enum RtRectAxis {
    RT_RECT_YZ = 0, /* YZRect hitable.rs:324-362  x = min.x, normal +X, uv = (y, z) */
    RT_RECT_XZ = 1, /* XZRect hitable.rs:284-322  y = min.y, normal +Y, uv = (x, z) */
    RT_RECT_XY = 2  /* XYRect hitable.rs:244-282  z = min.z, normal +Z, uv = (x, y) */
};

/* Instance transforms (hitable.rs:404-520).  A primitive below `Translate { offset, ptr }` /
 * `RotateY::new(ptr, angle)` wrappers carries the index of its INNERMOST wrapper; xf_parent links
 * each wrapper to the next one outwards (RT_NO_XFORM at the top).  hit() applies the chain to the
 * ray from the outside in and fixes the HitRecord from the inside out, exactly like the nested
 * trait objects do (including RotateY's face-normal quirk, hitable.rs:505). */
enum RtXformType {
    RT_XF_TRANSLATE = 0, /* param = offset.x, offset.y, offset.z, 0   hitable.rs:404-418 */
    RT_XF_ROTATE_Y = 1   /* param = sin_theta, cos_theta, angle_degrees, 0   hitable.rs:438-510 */
};
#define RT_NO_XFORM 0xFFFFFFFFu
/* (wrappers nest to any depth, as the trait objects do: chains of up to 4 are walked in registers, longer ones through a list
 * that rt_scene_upload builds) */

#define RT_NO_MEDIUM 0xFFFFFFFFu
#define RT_MAX_MEDIA 65535u /* a depth's block of free-path counters holds this many; the 32nd and later media of a scene are
                             * tested together by a ray that reaches any of them, so scenes with many media are slower */

#define RT_NO_TEX 0xFFFFFFFFu
#define RT_PERLIN_POINTS 256u /* texture.rs:51 */

/*
 * Flattened structure-of-arrays scene.  Replaces `Vec<Arc<dyn Hitable>>` + the trait
 * objects behind it (hitable.rs:57-62, material.rs, pbr.rs, texture.rs).  Spheres (SURVEY.md
 * §8(a) a4), axis-aligned rectangles / boxes, the Translate / RotateY instance wrappers (§8(f)
 * rank 1) and ConstantMedium (§8(f) rank 2) are on the accelerated path.
 */
typedef struct RtFlatScene {
    /* spheres: hitable.rs:57-62 `Sphere { c, r, mat, name }` in world-list order */
    uint32_t n_spheres;
    const float* sph_cx;   /* [n_spheres] */
    const float* sph_cy;
    const float* sph_cz;
    const float* sph_r;
    const uint32_t* sph_mat; /* [n_spheres] index into the material table */

    /* axis-aligned rectangles: hitable.rs:244-362 `XYRect/XZRect/YZRect { min, max, mat }`; a GBox
     * (hitable.rs:364-383) flattens to its 6 sides in the order of GBox::new.  Rect i has primitive
     * index n_spheres + i: rects come after the spheres in the closest-hit tie order (= world-list
     * order when the scene lists its spheres first, as simple_light_scene does). */
    uint32_t n_rects;
    const uint8_t* rect_axis;  /* [n_rects] RtRectAxis: the constant coordinate */
    const float* rect_min;     /* [3*n_rects] `min` as written in the scene */
    const float* rect_max;     /* [3*n_rects] `max` */
    const uint32_t* rect_mat;  /* [n_rects] */

    /* instance transforms */
    uint32_t n_xforms;
    const uint8_t* xf_type;     /* [n_xforms] RtXformType */
    const float* xf_param;      /* [4*n_xforms] */
    const uint32_t* xf_parent;  /* [n_xforms] next wrapper outwards or RT_NO_XFORM */
    const uint32_t* sph_xform;  /* [n_spheres] innermost wrapper or RT_NO_XFORM; NULL = none */
    const uint32_t* rect_xform; /* [n_rects]   likewise */

    /* homogeneous media: hitable.rs:523-588 `ConstantMedium::new(boundary, density, phase_tex)`.
     * The boundary's primitives are flattened like any others but tagged with the medium that owns
     * them (sph_medium / rect_medium); tagged primitives are NOT hit directly — medium i is primitive
     * n_spheres + n_rects + i and its hit() does the two boundary queries and the one random draw of
     * hitable.rs:540-568.  Its material is the Isotropic phase function (material.rs:99-113). */
    uint32_t n_media;
    const float* med_neg_inv_density; /* [n_media] -1/(k*density), k = how many times the scene's own tree calls the
                                       * medium per visit: 2 for each enclosing BvhNode that holds it as its only
                                       * object (left == right, hitable.rs:188, 236-237), else 1 */
    const uint32_t* med_mat;          /* [n_media] material index (RT_MAT_ISOTROPIC) */
    const uint32_t* sph_medium;       /* [n_spheres] owning medium or RT_NO_MEDIUM; NULL = none */
    const uint32_t* rect_medium;      /* [n_rects] likewise */
    const uint32_t* med_xform;        /* [n_media] the innermost wrapper AROUND medium i — `Translate { ptr: ConstantMedium }`,
                                       * hitable.rs:409-416: the medium's hit() then sees the moved ray (its length, its
                                       * rec.p = r.at(t)) and the wrapper fixes the record — or RT_NO_XFORM; NULL = none.
                                       * The chains of the boundary's primitives continue through this wrapper (they end
                                       * at the world like any other); wrappers INSIDE the boundary need no entry here. */

    /* materials */
    uint32_t n_materials;
    const uint8_t* mat_type;   /* [n_materials] RtMatType */
    const float* mat_color;    /* [3*n_materials] Metal albedo; unused otherwise */
    const float* mat_p0;       /* [n_materials] see RtMatType comments */
    const float* mat_p1;
    const float* mat_p2;
    const float* mat_p3;
    const uint32_t* mat_tex0;  /* [n_materials] texture index or RT_NO_TEX */
    const uint32_t* mat_tex1;

    /* textures */
    uint32_t n_textures;
    const uint8_t* tex_type;   /* [n_textures] RtTexType */
    const float* tex_color0;   /* [3*n_textures] */
    const float* tex_color1;   /* [3*n_textures] */
    const float* tex_scale;    /* [n_textures] PerlinTex.scale */
    const uint32_t* tex_aux;   /* [n_textures] perlin set index / image index */

    /* Perlin table sets (texture.rs:53-91): rand_vec then perm_x, perm_y, perm_z */
    uint32_t n_perlin;
    const float* perlin_vec;    /* [n_perlin*256*3] xyz interleaved */
    const uint16_t* perlin_perm;/* [n_perlin*3*256] values 0..255 */

    /* images (texture.rs:170-181): Rgb<f32> = u8/255, row 0 = top of the file */
    uint32_t n_images;
    const uint32_t* img_w;      /* [n_images] */
    const uint32_t* img_h;
    const uint64_t* img_offset; /* [n_images] offset in floats into `texels` */
    const float* texels;        /* RGB interleaved */
    uint64_t n_texel_floats;

    /* sky (lib.rs:11) */
    uint32_t sky_type;  /* RtSkyType */
    uint32_t sky_image; /* image index for RT_SKY_ENV (demo_scene.rs:19 ENV_TEX) */
} RtFlatScene;

/* camera.rs:7-10 — the four derived vectors of `Camera` (private fields there). */
typedef struct RtCamera {
    float origin[3];
    float horizontal[3];
    float vertical[3];
    float lower_left_corner[3];
} RtCamera;

/*
 * Render parameters.  Replaces the constants captured by the closure at main.rs:80:
 * nx, ny (main.rs:66-67), samples_per_pixel (main.rs:64), MAX_DEPTH (main.rs:36) and
 * the seed base 95 (main.rs:82).
 */
typedef struct RtParams {
    uint32_t nx, ny;
    uint32_t spp;
    int32_t max_depth;   /* reference MAX_DEPTH = 50: segments with depth 0..=max_depth are traced */
    uint64_t seed;       /* reference: 95 */
    /* Row-interleaved sharding: image row j belongs to shard
     * (j / shard_band) % shard_count.  shard_count <= 1 renders every row. */
    uint32_t shard_band;
    uint32_t shard_count;
    uint32_t shard_id;
    uint32_t spp_slice;  /* samples per pixel traced per wavefront slice; 0 = library default */
    uint32_t flags;      /* RT_FLAG_* */
    uint32_t reserved;
} RtParams;

#define RT_FLAG_NONE 0u
/* Closest hit by the plain list walk (HitableList::hit order, hitable.rs:117-132) instead of the
 * LDS-resident BVH.  Results are identical either way; the flag exists for cross-checking. */
#define RT_FLAG_BRUTE_FORCE 1u
/* Russian roulette, the estimator the reference keeps commented out at main.rs:49-53: after a
 * successful scatter draw one more f32; the path continues with probability
 * threshold = attenuation.max_element() and its attenuation is divided by the threshold.
 * Unbiased, NOT the reference's default estimator (opt-in; paths get ~2x shorter at depth 50). */
#define RT_FLAG_RUSSIAN_ROULETTE 2u
/* Flag bits 4u and 8u are diagnostic hooks, declared in rtow_mi355x_debug.h (RT_FLAG_TIME_DEPTHS, RT_FLAG_PRODUCTION_KERNELS). */

typedef struct RtStats {
    uint64_t n_paths;          /* nx_rows_local * nx * spp                                   */
    uint64_t n_rays;           /* closest-hit queries = ray_color calls passing main.rs:40   */
    uint64_t n_rays_secondary; /* n_rays - n_paths                                           */
    uint64_t n_texture_fetches;/* ImageTex texel fetches (0 when not counted)                */
    uint64_t n_bad_dir;        /* paths dropped where the reference would assert (main.rs:39) */
    double seconds_total;      /* wall time of the render call, host clock                   */
    double seconds_trace;      /* sum of trace+shade kernel time (HIP events, device clock)   */
    double seconds_device;     /* all kernels of the call (HIP events)                       */
    uint64_t bytes_algorithmic;/* 96*n_rays + 24*n_paths (+12*n_texture_fetches), SURVEY §8(d) */
    uint64_t bytes_trace_algorithmic; /* trace kernel share: 48*n_rays + 48*n_secondary + 12*n_paths + 12*n_texture_fetches */
    uint32_t n_trace_launches;
    uint32_t n_slices;
    uint64_t rays_per_depth[64]; /* rays traced at depth d (d < 64) */
} RtStats;

typedef struct RtCtx RtCtx;

/* -- lifecycle ------------------------------------------------------------------------ */
uint32_t rt_abi_version(void);
/* 16 hex digits over the device sources and compiler flags the library was built from ("unknown" for a hand-made build).
 * Measurement records (profiles/) carry it so that a number is never quoted for kernels other than the ones it was taken on. */
const char* rt_build_id(void);
/* Creates a context on HIP device `device_id`.  Replaces main.rs:72-73 (thread pool setup). */
int rt_ctx_create(int device_id, RtCtx** out_ctx);
void rt_ctx_destroy(RtCtx* ctx);
/* Last error text of `ctx` (or of the calling thread's last failed rt_ctx_create if NULL). */
const char* rt_last_error(const RtCtx* ctx);

/* -- scene ---------------------------------------------------------------------------- */
/* Validates and copies the flat scene to HBM (packed device records, Perlin tables,
 * texel pool).  Replaces `let (world, cam) = scene(aspect)` hand-over at main.rs:74 and
 * `SKY_COLOR.set` (demo_scene.rs:38).  May be called again to replace the scene. */
int rt_scene_upload(RtCtx* ctx, const RtFlatScene* scene);

/* Number of image rows owned by a shard, and the mapping local row -> image row. */
uint32_t rt_shard_rows(uint32_t ny, uint32_t shard_band, uint32_t shard_count, uint32_t shard_id);
uint32_t rt_shard_row_to_image_row(uint32_t local_row, uint32_t shard_band, uint32_t shard_count,
                                   uint32_t shard_id);

/* -- render --------------------------------------------------------------------------- */
/*
 * Renders the shard described by `params` and copies the result to host memory.
 * Replaces the pixel loop main.rs:77-108 and the quantisation main.rs:98-105,127.
 *   out_rgb_f32 : [rows_local*nx*3] linear radiance mean (c / spp, BEFORE gamma), local
 *                 row 0 = lowest image row of the shard (reference j order).  May be NULL.
 *   out_rgb8    : [rows_local*nx*3] gamma-2, *255.99 saturating u8, rows in DESCENDING j
 *                 (i.e. flipped like main.rs:127).  May be NULL.
 */
int rt_render(RtCtx* ctx, const RtCamera* cam, const RtParams* params, float* out_rgb_f32,
              uint8_t* out_rgb8, RtStats* stats);

/*
 * Optional: tells the context which frame it will be asked for — nx, ny, spp, spp_slice and the shard fields of `params` are
 * read, no scene is needed — so that the device memory for its work buffers (100 B per ray of a slice: 53 GB for 1920 x 1080 x
 * 256 spp in one slice) is requested NOW, by a helper thread, while the host builds its scene.  The reference knows its frame
 * before it builds the world (main.rs:64-67 against main.rs:74), and renders one frame per process: without the hint the first
 * rt_render starts the same request itself and renders its first slices in what has arrived so far.  Returns at once.
 */
int rt_prepare(RtCtx* ctx, const RtParams* params);

/* Pinned (page-locked) host memory for the two output images.  rt_render() writes a destination allocated here — or any
 * memory the caller has registered with the HIP runtime — by asynchronous copies at PCIe rate behind the last kernel; a
 * pageable destination (a plain Vec / malloc) works too and costs a staged copy (~3 ms instead of ~0.6 ms for a
 * 1920 x 1080 frame).  This is what a host that replaces main.rs:109-128 (the receive loop that fills the ImageBuffer)
 * would allocate its frame in.  NULL on failure. */
void* rt_host_alloc(size_t bytes);
void rt_host_free(void* p);

/*
 * Same, but the f32 framebuffer stays in HBM: `d_out_rgb_f32` is a DEVICE pointer to
 * rows_local*nx*3 floats (e.g. the storage of a tensor that RCCL will gather).  `stream`
 * is a hipStream_t (NULL = the context's own stream); the call returns after the work has
 * been enqueued and `stats` (if not NULL) forces a synchronisation to read the counters.
 * A sphere-only scene synchronises `stream` once more, 0.1 ms into the frame: the number of
 * pixels whose primary-ray candidate list overflowed decides on the host whether depth 0 needs
 * a closest-hit launch (none does in any headline configuration).  The first frame on a stream
 * is preceded by ~0.3 ms of spin kernels that check that the library's second stream runs
 * beside it (two streams on one hardware queue would run the two halves of a slice in turn).
 */
int rt_render_device(RtCtx* ctx, const RtCamera* cam, const RtParams* params,
                     void* d_out_rgb_f32, void* stream, RtStats* stats);

/*
 * Progressive preview.  Replaces the partial saves of the receive loop, main.rs:114-123 (there: every 10
 * columns of pixels; here: after every slice of samples, the unit in which a wavefront renderer finishes
 * work).  After each slice of a following rt_render() the callback gets the running mean of the samples
 * done so far, quantised and flipped exactly like the final image (main.rs:98-105,127): rows_local*nx*3
 * bytes, valid during the call.  The final image is unchanged by the callback; choose the preview cadence
 * with RtParams.spp_slice.  NULL removes the callback.  rt_render_device() never calls it.
 */
typedef void (*RtProgressFn)(void* user, uint32_t spp_done, uint32_t spp_total, const uint8_t* rgb8, uint32_t nx,
                             uint32_t rows);
int rt_set_progress(RtCtx* ctx, RtProgressFn fn, void* user);

/*
 * Thin lens: defocus blur.  The book's Camera::new(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist) (Ray Tracing in One
 * Weekend, chapter 13; the reference's camera.rs has no lens) with lens_radius = aperture / 2.  The RtCamera stays camera.rs's
 * unit-focal-length camera; the lens is applied on top of it.  A primary ray leaves origin + rx LU + ry LV, (rx, ry) drawn in the unit
 * disc, towards origin + focus_dist * (llc + u H + v V - origin), with LU = lens_radius H / |H| and LV = lens_radius V / |V|: the plane
 * of focus lies at focus_dist along -w, as the book's does.  DESIGN.md "Thin lens".
 */
typedef struct RtLens {
    float lens_radius, focus_dist;
} RtLens;
/* The lens of every following rt_render / rt_render_device of `ctx` (per context, like rt_set_progress; rt_scene_upload leaves it).
 * NULL or lens_radius 0: the pinhole camera, bit for bit.  RT_ERR_INVALID, and the previous lens stays, unless both values are finite,
 * lens_radius >= 0 and, where lens_radius > 0, focus_dist > 0. */
int rt_set_lens(RtCtx* ctx, const RtLens* lens);

/* Motion blur ("The Next Week", chapter 1): spheres whose centre moves linearly while the shutter is open, every path carrying a time.
 * Sphere `sphere[k]` of the uploaded scene has its RtFlatScene centre c0 at time 0 and center1[3 k ..] at time 1; radius, material and
 * name stay.  A path's time is tm = shutter_open + u * (shutter_close - shutter_open), u the f32 draw of counter 254 of the path's key
 * (one time for all its segments); the sphere is then hit at c(tm) = c0 + tm * (c1 - c0), every operation rounded to f32 (c1 - c0
 * once, at this call), exactly as a static sphere at c(tm) would be.  DESIGN.md "Moving spheres".
 * Only bare spheres move: one below a Translate / RotateY wrapper or bounding a medium is RT_ERR_UNSUPPORTED. */
typedef struct RtMotion {
    uint32_t n_moving;
    const uint32_t* sphere;   /* [n_moving] sphere indices of the uploaded scene, strictly increasing */
    const float* center1;     /* [3*n_moving] centre at time 1 */
    float shutter_open, shutter_close; /* 0 <= shutter_open <= shutter_close <= 1 */
} RtMotion;
/* The motion of every following render of `ctx`, after rt_scene_upload (RT_ERR_STATE before); rt_scene_upload clears it (the indices
 * belong to a scene).  NULL or n_moving 0: the static renderer, bit for bit.  n_moving > 0 selects the motion kernels even when no
 * sphere is displaced, and rebuilds what bounds the listed spheres (tree leaves, grid cells, candidate-list spheres) over the region
 * they sweep.  RT_ERR_INVALID (indices unsorted, repeated or out of range, non-finite center1, a shutter outside
 * 0 <= open <= close <= 1) or RT_ERR_UNSUPPORTED: the previous motion stays.  The arrays are copied. */
int rt_set_motion(RtCtx* ctx, const RtMotion* motion);

/* Planar primitives ("The Next Week", chapter 6): quadrilaterals (parallelograms) Q + a u + b v, 0 <= a, b <= 1, in any orientation, and
 * triangles with the corners Q, Q + u, Q + v (a, b >= 0, a + b <= 1), attached to the uploaded scene.  Planar primitive i is primitive
 * n_spheres + n_rects + n_media + i: it comes after everything of the world list, no existing index moves, and it takes part in the
 * winner rule t < best || (t == best && idx > best_idx).  The primitives are bare (no wrapper, no medium boundary); transform the
 * vertices yourself.  The hit test is the book's quad::hit, every operation one IEEE f32 operation:
 *   at rt_set_quads, once, in this order:  n = cross(u, v);  normal = n / sqrt(dot(n, n)) (three divisions);  D = dot(normal, Q);
 *     w = n / dot(n, n) (three divisions);  dot(a, b) = (ax bx + ay by) + az bz,  cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx)
 *   per ray:  denom = dot(normal, d), a miss where |denom| < 1e-8;  t = (D - dot(normal, o)) / denom, rejected when NaN, t < t_min or
 *     t > t_max;  P = o + d t;  p = P - Q;  alpha = dot(w, cross(p, v));  beta = dot(w, cross(u, p));  quad: 0 <= alpha <= 1 &&
 *     0 <= beta <= 1;  triangle: alpha >= 0 && beta >= 0 && alpha + beta <= 1.
 * The record is p = P, t, uv = (alpha, beta) (what an image texture reads) and set_face_normal(r, normal).  A planar primitive carries
 * no tangent, as a rectangle carries none: DisneyMetal on one is RT_ERR_UNSUPPORTED.  As the book's, the test is NOT watertight across
 * an edge two primitives share: in f32 a ray through the edge may be accepted by both, or by neither.
 * Conditioning: RT_ERR_INVALID unless |n|^2 >= RT_PLANAR_MIN_SIN2 |u|^2 |v|^2 (evaluated in double; sin of the angle between u and v
 * at least 2^-10, 0.056 degrees) — the limit the culling bound is derived for.  A tree leaf is the box of the 3 or 4 corners grown by
 *   slack = 2^-24 (64 L / sin(u, v) + 16 (M + RT_PLANAR_REACH W)),  L = max(|u|, |v|), M = the largest corner coordinate magnitude,
 *   W = the largest coordinate magnitude of the scene's bounds and of all corners of the set,
 * which covers what the f32 test can accept outside the exact figure for every ray whose origin coordinates stay within
 * RT_PLANAR_REACH W (DESIGN.md "Planar primitives").  Scattered rays start on the scene; the camera is checked: rt_render of a context
 * that holds a set returns RT_ERR_UNSUPPORTED when |origin_k| + lens_radius exceeds RT_PLANAR_REACH W on any axis.
 * Moving spheres and planar primitives do not combine yet: rt_set_motion on a context that holds planar primitives, and rt_set_quads
 * on one that holds a motion, are RT_ERR_UNSUPPORTED and the previous state stays.  rt_set_lens combines freely. */
enum RtPlanarKind { RT_PLANAR_QUAD = 0, RT_PLANAR_TRIANGLE = 1 };
#define RT_PLANAR_MIN_SIN2 9.5367431640625e-07 /* 2^-20 */
#define RT_PLANAR_REACH 16.0
typedef struct RtQuads {
    uint32_t n;
    const float* q;        /* [3n] corner Q */
    const float* u;        /* [3n] edge vectors: the quad is Q + a u + b v, 0 <= a,b <= 1; */
    const float* v;        /* [3n] the triangle has the corners Q, Q+u, Q+v (a,b >= 0, a+b <= 1) */
    const uint8_t* kind;   /* [n] RtPlanarKind */
    const uint32_t* mat;   /* [n] index into the material table of the uploaded scene */
} RtQuads;
/* The planar primitives of every following render of `ctx`, after rt_scene_upload (RT_ERR_STATE before); rt_scene_upload clears them.
 * NULL or n 0: the renderer without planar primitives, bit for bit, with the upload's search structures back.  A set selects the
 * general kernels in their planar instantiations (no sphere grid, no candidate lists) and builds the tree over the scene's entries
 * and the set.  RT_ERR_INVALID (a non-finite component, a kind outside the enum, a material index out of range, a degenerate or
 * ill-conditioned u, v, more entries than the tree indexes) or RT_ERR_UNSUPPORTED: the previous set stays.  A device-side failure
 * (RT_ERR_NOMEM, RT_ERR_DEVICE) while a set replaces another leaves the context WITHOUT planar primitives, not with the previous set.
 * The arrays are copied. */
int rt_set_quads(RtCtx* ctx, const RtQuads* quads);

/* Light importance sampling ("The Rest of Your Life": the mixture density).  The lights are SAMPLING TARGETS ONLY: world-space
 * parallelograms Q + a u + b v, 0 <= a, b <= 1, towards which scattering surfaces aim half of their rays.  They are not geometry and
 * carry no material; the closest hit never sees them, no shadow ray is traced and emission is still picked up when a path hits an
 * emitter.  One half of the mixture covers the whole hemisphere, so the estimator is unbiased for ANY set of parallelograms: a set
 * that lies where the emitters are (an XZRect light, an emissive quad, an emitter below wrappers given by its world-space corners) is
 * merely the one that lowers the variance, and a wrong or stale set costs noise, never a wrong mean.
 * Set-up, once per light k in rt_set_lights: (normal_k, D_k, w_k) exactly as rt_set_quads computes them for a quad, and
 *   area_k = sqrt(dot(n, n)), n = cross(u, v).
 * Materials affected: RT_MAT_DIFFUSE (its density p_s = dot(n, dir) RT_FRAC_1_PI) and the materials that draw random_on_hemisphere —
 * Lambert and the seven pbr.rs materials, tags 2 and 6..12 (p_s = 0.5 RT_FRAC_1_PI).  Emission, Metal, Dielectric, Isotropic, media,
 * misses and the sky draw nothing new and are unchanged in every bit.  Per hit of an affected material, every operation one IEEE f32
 * operation in this order, the rng standing where the material's first draw stands without a set:
 *   1. s = next().
 *   2. s < 0.5: the material's own direction with its own draws (Diffuse: normalize(n + normalize(random_in_unit_sphere)) with the
 *      near-zero fix; the others: random_on_hemisphere(n)).
 *   3. else: k = min((uint32)(next() * n_lights), n_lights - 1);  a = next();  b = next();  target = (Q_k + u_k a) + v_k b;
 *      dir = normalize(target - po), po = offset_hit_point(p, n) = the scattered ray's origin.
 *   4. c = dot(n, dir); !(c > 0) (a NaN dir too): the path ends with zero radiance, as a Metal scatter that returns false.
 *   5. p_L = (sum_k pdf_k) / n_lights, summed in index order from 0; pdf_k = 0 unless the quad test of rt_set_quads accepts the ray
 *      (po, dir) on light k with t_min = 1e-3, t_max = FLT_MAX, and then pdf_k = (t t) / (fabsf(dot(normal_k, dir)) area_k).
 *   6. wgt = p_s / ((p_s + p_L) 0.5f).
 *   7. attenuation = the material's formula evaluated with dir, each component then multiplied by wgt.
 * RT_FLAG_RUSSIAN_ROULETTE acts on the weighted attenuation afterwards.  (A light-chosen target on the very edge of its quad may fail
 * its own f32 hit test: pdf_k = 0 and the weight is 2, probability of the order 2^-20 per draw, not corrected.)
 * rt_set_lens and rt_set_quads combine freely with a light set.  Moving spheres and a light set do not combine yet: rt_set_motion on a
 * context that holds a light set, and rt_set_lights on one that holds a motion, are RT_ERR_UNSUPPORTED and the previous state stays. */
#define RT_MAX_LIGHTS 16u
typedef struct RtLights {
    uint32_t n;        /* 1..RT_MAX_LIGHTS */
    const float* q;    /* [3n] world-space parallelograms Q + a u + b v, 0 <= a,b <= 1 */
    const float* u;    /* [3n] */
    const float* v;    /* [3n] */
} RtLights;
/* The light set of every following render of `ctx`, after rt_scene_upload (RT_ERR_STATE before); rt_scene_upload clears it.  NULL or
 * n 0: the renderer without light sampling, bit for bit.  RT_ERR_INVALID (n > RT_MAX_LIGHTS, a NULL array, a non-finite component, u, v
 * that fail the RT_PLANAR_MIN_SIN2 conditioning of rt_set_quads — the same test, in double) or RT_ERR_UNSUPPORTED: the previous set
 * stays.  The arrays are copied. */
int rt_set_lights(RtCtx* ctx, const RtLights* lights);

/* -- progressive accumulation, a per-pixel error estimate and a noise target ----------------------------------------
 * rt_render traces a fixed spp and drops its running sums.  An ACCUMULATION keeps them: samples are added in any portions, the frame so
 * far can be read at any time, and with it a measure of its noise.  Path keys are a function of (seed, pixel, sample) and a pixel's
 * samples are summed in sample order, so after rt_accum_begin(first_sample 0) and adds of n1 + n2 + ... = n samples the images are, bit
 * for bit, those of rt_render with spp = n, however the adds and their slices are cut.
 * Moments, per pixel and per sample (r, g, b) — the f32 values the sum reads — every operation one IEEE f64 operation, no FMA:
 *   Y = ((0.2126 (double)r + 0.7152 (double)g) + 0.0722 (double)b);   S1 += Y;   S2 += Y * Y   in sample order, across slices and adds.
 * With n = samples done:  Ybar = S1 / n;  V = max(0, (S2 - S1 * S1 / n) / (n - 1)) / n, the variance of the mean (V = 0 where n < 2);
 * out_sem = (float)sqrt(V), the standard error of the pixel's mean luminance.  A non-finite sample propagates as IEEE arithmetic has it
 * (its pixel's sem, and with it the frame figures, become NaN); max(0, x) keeps a NaN.
 * Frame figures, in f64, over the npix pixels of the shard:  mean_luminance = (sum_p Ybar_p) / npix;  rms_sem = sqrt((sum_p V_p) / npix);
 * noise = rms_sem / mean_luminance — where mean_luminance == 0: 0 when rms_sem == 0, +inf otherwise — and +inf where n < 2.  The sums
 * run over a fixed tree (per workgroup, then one workgroup over the partial sums in index order; no floating-point atomics): the same
 * accumulation read twice gives the same bits.
 * Cost: 28 B per pixel that the accumulation owns (an f32 x 3 sum, an f64 x 2 moment), apart from the frame renderer's buffers —
 * rt_render and rt_render_device may be called in between and neither disturbs the other.  The first rt_accum_denoise of a context adds
 * 20 B + 12 B per pixel (the filter's inputs c, y, v in image order and its output), kept for the next like the accumulation's buffers.
 * Across devices: rt_multi_accum_* (the noise of a frame split over devices needs the frame in one piece: the joined context of
 * rt_multi_accum_join delivers it).  Not covered: rt_render_to_noise over an RtMulti (the caller loops add / join / read); the rt_set_progress callback (a
 * host that accumulates has its preview in rt_accum_read).  rt_accum_add gives every pixel the same number of samples; "Adaptive
 * sampling" below gives them to the pixels that still need them. */
typedef struct RtNoise {
    uint32_t spp_done;      /* samples per pixel accumulated so far */
    uint32_t reserved;
    double mean_luminance;  /* (sum_p Ybar_p) / npix */
    double rms_sem;         /* sqrt((sum_p V_p) / npix) */
    double noise;           /* rms_sem / mean_luminance, see above */
} RtNoise;
/* Opens the accumulation of `ctx` (one per context; an open one is dropped) and clears its sums.  Fixes the frame: the camera, nx, ny,
 * the shard fields, max_depth, seed, flags and spp_slice of `params`, and with them the context's lens, motion, planar primitives and
 * lights and the pixel order — each of the calls listed below that could change one ends the accumulation.  params->spp (>= 1) is read
 * only as the expected size of one add, for which the work buffers are requested now (as rt_prepare does); no result depends on it.
 * first_sample: the sample index the first added sample gets.  0 starts the frame rt_render renders; another value lets two contexts
 * or processes take disjoint sample windows of one frame.  RT_ERR_STATE without an uploaded scene. */
int rt_accum_begin(RtCtx* ctx, const RtCamera* cam, const RtParams* params, uint32_t first_sample);
/* Traces samples [first_sample + done, first_sample + done + n_samples) of every pixel of the shard, with the kernels and the slices
 * of rt_render, and adds them to the running sums in sample order.  `stats` (may be NULL; it forces a synchronisation, as in
 * rt_render_device) is what rt_render would report for these samples.  RT_ERR_INVALID: n_samples 0, or first_sample plus everything
 * added would pass 2^32 - 1, the bound of RtParams.spp — nothing has changed then.  RT_ERR_STATE: no open accumulation. */
int rt_accum_add(RtCtx* ctx, uint32_t n_samples, RtStats* stats);
/* The frame so far; any number of times, each pointer may be NULL.  out_rgb_f32 and out_rgb8 are exactly what rt_render writes (sum /
 * (float)done, gamma 2, the flip); out_sem is [rows_local*nx] f32 in the row order of out_rgb_f32.  Before the first add the images are
 * zeros, spp_done is 0, mean_luminance and rms_sem are 0 and noise is +inf.  Synchronises the context's stream once. */
int rt_accum_read(RtCtx* ctx, float* out_rgb_f32, uint8_t* out_rgb8, float* out_sem, RtNoise* noise);
/* Ends the accumulation (RT_OK also when none is open); its buffers are kept for the next.  An accumulation is also ended by
 * rt_ctx_destroy, rt_scene_upload, every successful rt_set_lens / rt_set_motion / rt_set_quads / rt_set_lights (and one that fails on
 * the device) and rt_debug_set_option: the next rt_accum_add or rt_accum_read is RT_ERR_STATE.  rt_render and rt_render_device do not
 * end it. */
int rt_accum_end(RtCtx* ctx);
/* Renders to a quality instead of a count: rt_accum_begin(first_sample 0), then adds of min(spp_step, what is left of params->spp)
 * samples until noise <= target_noise or params->spp samples, the maximum, are done; the outputs as rt_accum_read writes them, `stats`
 * summed over the adds (its times too); the accumulation is ended.  The image is, bit for bit, rt_render with spp = noise->spp_done.
 * After each add the host reads the 24 B of frame figures to decide: one stream synchronisation per step, the price of the decision —
 * choose spp_step so that a step is long against it (DESIGN.md "Accumulation and noise").  RT_ERR_STATE: an accumulation is open.
 * RT_ERR_INVALID: spp_step 0, target_noise NaN or negative, params->spp < 2. */
int rt_render_to_noise(RtCtx* ctx, const RtCamera* cam, const RtParams* params, double target_noise, uint32_t spp_step,
                       float* out_rgb_f32, uint8_t* out_rgb8, float* out_sem, RtNoise* noise, RtStats* stats);

/* -- adaptive sampling: converged pixels stop, the noisy ones go on -----------------------------------------------------------------
 * The sampling half of Rousselle, Knaus, Zwicker 2012, on the moments an accumulation keeps anyway.  The accumulation gains a sample
 * count n_p (u32) and a converged flag per pixel, 5 B per pixel in the local pixel order of its sums, allocated by the first adaptive add.
 * Decision, at the START of rt_accum_add_adaptive, from the moments of the samples a pixel holds so far; every operation one IEEE f64
 * operation, no FMA:
 *   (Ybar_p, V_p) = the figures of "Moments" above with n = n_p;   thr = tolerance * max(Ybar_p, luminance_floor), max(a, b) = a > b ? a : b;
 *   pixel p becomes CONVERGED iff  n_p >= min_samples && V_p <= thr * thr.
 * A comparison with a NaN is false: a pixel that holds a non-finite sample (its V is NaN from two samples on) stays active until the
 * caller stops, and spreads to no other pixel.  Converged is STICKY: no later decision looks at the pixel again.  Every pixel that is
 * still active after the decision then receives the samples [first_sample + n_p, first_sample + n_p + n_samples) — all active pixels
 * share one n_p, the number of samples the accumulation has issued — added in sample order.  Hence the defining property:
 *   pixel p of an adaptive accumulation is, bit for bit (sum, moments, sem), pixel p of rt_render / rt_accum_add with spp = n_p,
 * whatever the queue shards, chains, slices and pixel order (the place a primary ray takes in its queue shard depends on the order in
 * which workgroups arrive there; no result depends on the place).
 * Statistics.  A stopping rule that reads the estimate it stops on is biased: a pixel whose first samples happen to agree stops early
 * and keeps its — too low — variance and whatever mean it had, so rare bright samples it has not seen yet (fireflies) are under-represented.  The bias
 * falls with the number of samples the first decision sees: min_samples bounds it, and uniform warm-up adds raise that number for all.
 * tolerance is a relative standard error of the pixel's mean luminance; luminance_floor keeps dark pixels from asking for an absolute
 * error of 0 (with V_p = 0 — black sky — a pixel converges at min_samples for every tolerance, 0 included).
 * Mixing.  rt_accum_add calls BEFORE the first adaptive add are allowed (a warm-up: n_p starts at what they added); rt_accum_add AFTER
 * an adaptive add is RT_ERR_STATE.  Everything that ends an accumulation ends an adaptive one; rt_render in between disturbs nothing.
 * Reading.  rt_accum_read divides by (float)n_p per pixel; out_sem and the frame figures use n_p per pixel (V_p = 0 where n_p < 2) over
 * the same fixed tree; noise is +inf where any n_p < 2; RtNoise.spp_done = max_p n_p.  rt_accum_denoise takes c, y, v with n_p per pixel;
 * a pixel with n_p < 2 beside done >= 2 (only an imported state holds one: "Accumulation state") has no variance to be compared by: its c
 * is sum / (float)max(n_p, 1) as rt_accum_read writes it, its y and v are NaN, so it stays what it is and spreads to no other pixel.
 * Depth 0 of an adaptive add runs on the materialised ray queue (the fused depth-0 kernels and the candidate lists invert a queue position
 * into a pixel, which a compacted queue does not allow): per traced sample it costs what RT_OPT_MATERIALISE_PRIMARIES costs (DESIGN.md
 * "Adaptive sampling").  Across devices: rt_multi_accum_add_adaptive (the decision is per pixel, so shards need no exchange).  Not covered:
 * rt_render_adaptive over an RtMulti; un-sticking a pixel; per-channel criteria. */
typedef struct RtAdaptive {
    double tolerance;        /* finite, >= 0: relative standard error of the mean luminance at which a pixel stops */
    double luminance_floor;  /* finite, > 0: the mean luminance below which the error is measured against this floor */
    uint32_t min_samples;    /* >= 2: no pixel stops on fewer samples */
    uint32_t reserved;       /* 0 */
} RtAdaptive;
typedef struct RtAdaptiveInfo {
    uint64_t n_active;       /* pixels of the shard not converged, as decided by the last adaptive add (all, before the first) */
    uint64_t n_samples;      /* sum of n_p over the shard */
    uint32_t spp_min, spp_max; /* min_p n_p, max_p n_p */
} RtAdaptiveInfo;
/* The decision above, then n_samples more samples for every pixel still active.  `stats` (may be NULL; it forces a synchronisation) are
 * those of the rays actually traced: n_paths = active pixels x n_samples (0 when every pixel has converged: nothing is traced and no image
 * changes), the depth totals as in rt_accum_add.  RT_ERR_INVALID: `ad` NULL or outside the ranges of RtAdaptive, n_samples 0, or
 * first_sample plus everything issued would pass 2^32 - 1 — nothing has changed then.  RT_ERR_STATE: no open accumulation. */
int rt_accum_add_adaptive(RtCtx* ctx, uint32_t n_samples, const RtAdaptive* ad, RtStats* stats);
/* The sample counts of the open accumulation: out_counts [rows_local*nx] in the row order of out_rgb_f32 (may be NULL), and the sums
 * over the shard (may be NULL).  Before the first adaptive add every n_p is the number of samples added so far and every pixel is
 * active.  Synchronises the context's stream once.  RT_ERR_STATE: no open accumulation. */
int rt_accum_read_counts(RtCtx* ctx, uint32_t* out_counts, RtAdaptiveInfo* info);
/* rt_accum_begin(first_sample 0), then adaptive adds of min(spp_step, what is left of params->spp) samples until no pixel is active or
 * params->spp samples, the maximum, are issued; the outputs as rt_accum_read and rt_accum_read_counts write them (each may be NULL),
 * `stats` summed over the adds; the accumulation is ended.  After each add the host reads n_active with the frame figures: one stream
 * synchronisation per step, as rt_render_to_noise pays.  The add that finds no active pixel traces nothing and is the last.
 * RT_ERR_STATE: an accumulation is open.  RT_ERR_INVALID: spp_step 0, params->spp < 2, `ad` outside its ranges. */
int rt_render_adaptive(RtCtx* ctx, const RtCamera* cam, const RtParams* params, const RtAdaptive* ad, uint32_t spp_step,
                       float* out_rgb_f32, uint8_t* out_rgb8, float* out_sem, uint32_t* out_counts, RtNoise* noise, RtAdaptiveInfo* info,
                       RtStats* stats);
/* The two GPU-free halves of the decision, for a host that plans or checks one (no context, no device).  rt_adaptive_check: RT_OK or
 * RT_ERR_INVALID as rt_accum_add_adaptive judges `ad` and n_samples.  rt_adaptive_converged: 1 when a pixel with the moments (s1, s2)
 * of n samples meets the criterion of `ad`, 0 when not, RT_ERR_INVALID for an `ad` outside its ranges. */
int rt_adaptive_check(const RtAdaptive* ad, uint32_t n_samples);
int rt_adaptive_converged(const RtAdaptive* ad, double s1, double s2, uint32_t n);

/* -- denoising: a non-local-means filter guided by the accumulation's own variance -----------------------------------------------------
 * The two moments of a pixel say how far two pixel means may differ by chance; the filter averages what differs only by that much and
 * keeps what differs by more (Rousselle, Knaus, Zwicker 2012: "Adaptive rendering with non-local means filtering").  Image space: it
 * reads the running sum and the moments an open accumulation owns, through kernels of its own, and changes nothing in them.
 * Every operation is one IEEE f32 operation in the order written, no FMA; `/` is the correctly rounded division.
 * Inputs.  Pixel a in image order, row 0 at the bottom, as out_rgb_f32; the accumulation holds n samples:
 *   c_a = the three channel sums, each divided by (float)n — what rt_accum_read writes;  y_a = (float)Ybar_a;  v_a = (float)V_a,
 *   Ybar and V the f64 figures of "Moments" above.
 * Parameters.  R = radius, 1 .. RT_DENOISE_MAX_RADIUS;  F = patch, 0 .. RT_DENOISE_MAX_PATCH;  k = strength, finite and > 0;
 *   k2 = k * k;  eps = 1e-10f;  cnt = (float)((2F+1)*(2F+1)).
 * Per output pixel p = (px, py): visit delta = (dx, dy) with dy from -R to R in the outer loop and dx from -R to R in the inner one;
 * q = p + delta, skipped where it lies outside the image.
 *   1. Patch distance.  Coordinates are clamped to the image per axis, those of a and of b independently; row sums come first:
 *        S = 0;  for oy = -F..F: { row = 0;  for ox = -F..F: row = row + d(clamp(p + o), clamp(q + o));  S = S + row; }   D = S / cnt;
 *        d(a, b) = ((y_a - y_b) * (y_a - y_b) - (v_a + min(v_a, v_b))) / (eps + k2 * (v_a + v_b)),  min(v_a, v_b) = v_b < v_a ? v_b : v_a.
 *   2. Weight.  m = (D < 0) ? 0 : D (a NaN stays NaN);  u = 1 - 0.25f * m;  u = (u > 0) ? u : 0 (a NaN becomes 0);  w = (u * u) * (u * u).
 *      w follows exp(-m) closely, has compact support (0 from D = 4 on) and needs no transcendental function.
 *   3. Accumulate, only where u != 0:  den = den + w,  and per channel  num = num + w * c_q.
 * Output.  out_p = num / den per channel; out_p = c_p where den == 0.  That happens only where p itself is not finite: its own patch
 * makes every D NaN.  A non-finite pixel does not spread: any patch that holds it has D = NaN, u = 0, and such terms are skipped, not
 * multiplied by 0.  For a finite p the term q = p has D <= 0 and w = 1, so den >= 1.
 * The order of the sums is part of the definition; it lets row sums be shared between neighbouring pixels without changing a bit.
 * Not covered: the distance is on LUMINANCE, the one quantity whose variance an accumulation keeps by default — edges between colours of
 * equal luminance blur; "Channel moments and the colour-guided filter" below keeps a variance per channel (48 B per pixel more, opt-in)
 * and filters on it; the weights are chosen from the
 * image they filter — "Half buffers" below keeps the even and the odd samples apart (56 B per pixel more, opt-in), filters each half with
 * the other's weights and reports the variance that is left; on an RtMulti the filter runs on the joined context (rt_multi_accum_join), not on a shard.
 * DESIGN.md "Denoising". */
typedef struct RtDenoise { uint32_t radius, patch; float strength; uint32_t reserved; } RtDenoise;
#define RT_DENOISE_MAX_RADIUS 10u
#define RT_DENOISE_MAX_PATCH 3u
#define RT_DENOISE_DEFAULT_STRENGTH 1.0f /* of 0.45, 0.7 and 1.0 the one with the lowest error on rendered frames (DESIGN.md "Denoising") */
/* Filters the frame of the open accumulation; `dn` NULL: radius 5, patch 1, strength RT_DENOISE_DEFAULT_STRENGTH.  The outputs are laid
 * out as rt_accum_read lays them out, either may be NULL; out_rgb8 is the filtered image through the quantisation and flip of rt_render.
 * The accumulation is read and not changed: rt_accum_read returns the same bits afterwards and further rt_accum_adds continue as if the
 * call had not happened.  Synchronises the context's stream once.  RT_ERR_STATE: no accumulation is open, or fewer than 2 samples are
 * done (there is no variance yet).  RT_ERR_UNSUPPORTED: shard_count > 1 (the local rows of an interleaved shard are not neighbours in
 * the image).  RT_ERR_INVALID: radius 0 or above the maximum, patch above the maximum, strength non-finite or <= 0, reserved != 0.  A
 * shard without pixels: RT_OK, nothing is written. */
int rt_accum_denoise(RtCtx* ctx, const RtDenoise* dn, float* out_rgb_f32, uint8_t* out_rgb8);

/* -- channel moments and the colour-guided filter ------------------------------------------------------------------------------------------
 * The filter above cannot tell two colours of equal luminance apart, and more samples only make it surer that they are "the same".  An
 * accumulation that TRACKS CHANNELS also keeps, per pixel and channel c in {r, g, b}, two f64 moments of the f32 sample values x_c — the
 * values the running sum reads — every operation one IEEE f64 operation, no FMA:
 *   S1_c += (double)x_c;   S2_c += (double)x_c * (double)x_c   in sample order, across slices and adds, uniform or adaptive.
 * With n samples (n_p of the pixel after adaptive adds):  V_c = max(0, (S2_c - S1_c * S1_c / n) / (n - 1)) / n, V_c = 0 where n < 2; a
 * NaN stays a NaN, as in "Moments".  Cost: 48 B per pixel more, in the local pixel order of the sums, allocated by
 * rt_accum_track_channels and kept for the next accumulation like the other accumulation buffers; the first rt_accum_denoise_channels of a
 * context adds 24 B per pixel (its inputs) to the filter's 12 B output.  Everything an accumulation returned before — the running sum,
 * the luminance moments, out_sem, the frame figures, the counts, rt_accum_denoise, the defining properties of "Progressive accumulation"
 * and "Adaptive sampling" — is unchanged in every bit, with tracking on or off.
 * The colour-guided filter is "Denoising" word for word with these differences:
 *   Inputs.  c_a as there;  v_a,ch = (float)V_ch, the three channel variances of pixel a.
 *   Per-channel term.  d_ch(a, b) = ((c_a,ch - c_b,ch) * (c_a,ch - c_b,ch) - (v_a,ch + min(v_a,ch, v_b,ch))) / (eps + k2 * (v_a,ch + v_b,ch)),
 *     min(x, y) = y < x ? y : x.  The term of one patch offset is e = (d_r + d_g) + d_b.
 *   Patch sum.  S = 0;  for oy = -F..F: { row = 0;  for ox = -F..F: row = row + e(clamp(p + o), clamp(q + o));  S = S + row; }
 *     D = S / cnt3,  cnt3 = (float)(3*(2F+1)*(2F+1)).
 * The clamp per axis, the weight with its NaN rules, "accumulate only where u != 0", out = num / den, out = c_p where den == 0 and the
 * visiting order of delta are those of "Denoising"; a non-finite pixel spreads to no other, for the same reason.
 * Across devices: RT_MULTI_TRACK_CHANNELS and the joined context of rt_multi_accum_join.  Not covered: sharded frames for the filter
 * (RT_ERR_UNSUPPORTED, as rt_accum_denoise); a per-channel adaptive criterion
 * (rt_accum_add_adaptive decides on luminance); rt_render_to_noise and rt_render_adaptive, which open and end their own accumulation — a
 * host that wants the filter drives the adds itself.  DESIGN.md "Channel moments and the colour-guided filter". */
/* Makes the open accumulation track channels and clears the channel moments.  After rt_accum_begin and before the first add, uniform or
 * adaptive: RT_ERR_STATE without an open accumulation or after samples were added.  A second call is RT_OK and changes nothing.  Tracking
 * ends with the accumulation, through every call that rt_accum_end lists as ending one. */
int rt_accum_track_channels(RtCtx* ctx);
/* out_sem_rgb [rows_local*nx*3] = (float)sqrt(V_c), in the row order of out_rgb_f32; with n_p per pixel after adaptive adds.  Works on
 * shards.  Synchronises the context's stream once.  RT_ERR_STATE: no open accumulation, or it does not track channels. */
int rt_accum_read_channel_sem(RtCtx* ctx, float* out_sem_rgb);
/* rt_accum_denoise with the colour-guided filter: the same arguments, defaults, outputs and errors, the accumulation read and not changed.
 * RtDenoise.reserved stays 0.  In addition RT_ERR_STATE where the accumulation does not track channels. */
int rt_accum_denoise_channels(RtCtx* ctx, const RtDenoise* dn, float* out_rgb_f32, uint8_t* out_rgb8);

/* -- accumulation state: export, import and merge -------------------------------------------------------------------------------------------
 * Everything an open accumulation owns, as host arrays: the running f32 sums (NOT divided), the luminance moments, after adaptive adds
 * the per-pixel counts and converged flags, with tracking the channel moments.  A state outlives the accumulation, the context and the
 * process: rt_accum_import puts it into a fresh accumulation, which then goes on as the exported one would have (resume), and
 * rt_accum_merge adds the state of the sample window that FOLLOWS the accumulation's onto it, so that contexts, processes or GPUs can each
 * take a window of one frame (rt_accum_begin(first_sample)) and one of them ends up with all of them.
 * Layout.  Every plane is in the row order of out_rgb_f32, local row 0 lowest — never in the accumulation's local pixel order — so a state
 * does not depend on RT_OPT_PIXEL_ORDER, slices, chains or queue shards.  Cost: 28 B per pixel, + 5 B with counts, + 48 B with channel
 * moments, on the host and once more in a staging buffer on the device that is kept for the next call like the accumulation's buffers.
 * Identity.  frame_id = rt_accum_frame_id(camera, params) says which samples the state holds.  It covers the camera and the RtParams
 * fields a sample depends on.  The SCENE and what rt_set_lens / rt_set_motion / rt_set_quads / rt_set_lights installed are NOT in it:
 * keeping them equal between the exporter and the importer is the caller's duty, and a state imported over another scene is accepted and
 * means nothing.
 * Resume.  After rt_accum_begin(f), adds, rt_accum_export and then — in any context or process with the same scene and sets —
 * rt_accum_begin(f), rt_accum_import, everything the accumulation returns from then on is bit for bit what the uninterrupted one returns:
 * further adds (uniform or adaptive), rt_accum_read, rt_accum_read_counts, rt_accum_read_channel_sem, both filters, the frame figures.
 * Merge.  Per pixel one IEEE operation each, no FMA:  sum_c = sum_c + st.sum_c in f32;  S1 = S1 + st.S1, S2 = S2 + st.S2 in f64;  the six
 * channel moments likewise.  The merged image is therefore NOT rt_render(spp = n1 + n2) in every bit — an f32 sum of n1 + n2 terms was cut
 * in two: ((x0 + .. + x_{n1-1}) + (x_{n1} + .. + x_{n1+n2-1})) — it is the arithmetic above exactly; per channel of non-negative radiance
 * the two differ by at most (2 n + 2) 2^-24 of the larger, n = n1 + n2.  Moments, out_sem and the figures follow from the merged sums.
 * Failed calls leave the accumulation as it was.  A shard without pixels: RT_OK.  Across devices: rt_multi_accum_import splits a whole-frame
 * state over the shards and the joined context exports one; rt_accum_merge stays a single-context call.  Not covered: planes in device memory.
 * DESIGN.md "Accumulation state". */
#define RT_ACCUM_STATE_COUNTS   1u  /* adaptive: counts and converged are part of the state */
#define RT_ACCUM_STATE_CHANNELS 2u  /* channel moments are part of the state */
typedef struct RtAccumState {
    uint32_t nx, rows;           /* the shard: rows = rows_local */
    uint32_t first_sample, done; /* uniform: the window [first_sample, first_sample + done); adaptive: done = samples issued (n_p of the active pixels) */
    uint32_t planes;             /* RT_ACCUM_STATE_* */
    uint32_t reserved;           /* 0 */
    uint64_t frame_id;           /* rt_accum_frame_id of the frame */
    float*    sum;               /* [rows*nx*3] the running f32 sums, NOT divided */
    double*   moments;           /* [rows*nx*2] S1, S2 */
    uint32_t* counts;            /* [rows*nx]   n_p */
    uint8_t*  converged;         /* [rows*nx]   0 / 1 */
    double*   channel_moments;   /* [rows*nx*6] S1_r, S2_r, S1_g, S2_g, S1_b, S2_b */
} RtAccumState;
/* GPU-free.  FNV-1a 64 (offset 0xcbf29ce484222325, prime 0x100000001b3) over these little-endian bytes, in this order: the 12 camera floats
 * as bit patterns in struct order; nx, ny, (uint32_t)max_depth; seed (8 B); shard_band, shard_count, shard_id, with shard_count <= 1 mapped
 * to (0, 1, 0); flags & RT_FLAG_RUSSIAN_ROULETTE.  spp, spp_slice, RT_FLAG_BRUTE_FORCE and the diagnostic bits do not enter: no result
 * depends on them.  0 for a NULL argument. */
uint64_t rt_accum_frame_id(const RtCamera* cam, const RtParams* params);
/* GPU-free.  RT_OK, or RT_ERR_INVALID unless: reserved == 0 and planes holds no unknown bit; sum and moments non-NULL; counts and converged
 * non-NULL exactly when RT_ACCUM_STATE_COUNTS is set, channel_moments exactly when RT_ACCUM_STATE_CHANNELS is; first_sample + done <=
 * 2^32 - 1; with counts every converged[p] is 0 or 1, every counts[p] <= done, and counts[p] == done wherever converged[p] == 0 (all
 * active pixels share one n_p: "Adaptive sampling"). */
int rt_accum_state_check(const RtAccumState* st);
/* Fills the scalar fields of `st` (planes: what the accumulation holds) and writes every plane whose pointer is non-NULL; a NULL pointer
 * skips that plane (all NULL: the scalar fields alone, without any device work).  On a uniform accumulation counts gets `done` and converged 0 for every pixel, as rt_accum_read_counts reports there
 * (clear both pointers before handing such a state to rt_accum_import or rt_accum_merge).  Reads, and changes nothing.  Synchronises the
 * context's stream once.  RT_ERR_STATE: no open accumulation, or channel_moments non-NULL on one that does not track channels. */
int rt_accum_export(RtCtx* ctx, RtAccumState* st);
/* Puts `st` into the open accumulation, which must hold no sample yet: after rt_accum_begin (rt_accum_track_channels may come in between)
 * and before the first add of either kind, else RT_ERR_STATE.  Values are copied as bits: NaN and inf travel unchanged.  A state with
 * channel moments turns tracking on, with the allocation of rt_accum_track_channels; one with counts makes the accumulation adaptive, with
 * the allocation of the first adaptive add; `done` becomes st->done.  RT_ERR_INVALID: rt_accum_state_check fails; nx, rows, frame_id or
 * first_sample differ from the accumulation's; the accumulation tracks channels and the state has none.  Synchronises once. */
int rt_accum_import(RtCtx* ctx, const RtAccumState* st);
/* Adds `st`, the window that continues the open accumulation's, onto it by the arithmetic of "Merge" above: both uniform, st->first_sample
 * == first_sample + done of the accumulation (which may hold no sample yet: the result is 0 + x), nx, rows and frame_id equal, channel
 * moments in both or in neither.  done += st->done; adds of either kind then go on from first_sample + done.  RT_ERR_STATE: no open
 * accumulation.  RT_ERR_UNSUPPORTED: either side is adaptive (windows of pixels with different n_p are not contiguous).  RT_ERR_INVALID:
 * every other mismatch, a state rt_accum_state_check refuses, samples past 2^32 - 1.  Synchronises once. */
int rt_accum_merge(RtCtx* ctx, const RtAccumState* st);

/* -- half buffers: the even and the odd samples of every pixel, the cross-filtered denoise and its residual ---------------------------------
 * "Denoising" chooses its weights from the image it filters, so it leans towards its own noise, and once it has run nothing says how
 * noisy its result still is.  Rousselle, Knaus, Zwicker 2012 (section 4) answer both with two HALF BUFFERS: the even and the odd samples
 * of every pixel are kept apart, each half is filtered with weights taken from the OTHER one, the two results are averaged, and the
 * variance that is left is read off their difference.  The two half images are also what external denoisers ask a renderer for.
 * Tracking.  An accumulation that TRACKS HALVES also keeps, per pixel and half h in {0, 1}, an f32 x 3 sum and the two f64 luminance
 * moments of "Moments": 56 B per pixel more, in the local pixel order of the sums, allocated by rt_accum_track_halves (or
 * rt_accum_import_halves) and kept for the next accumulation like the other accumulation buffers.  The sample with the ABSOLUTE index
 * i = first_sample + k goes to half i & 1, in sample order, with the arithmetic of "Moments" (IEEE f32 / f64 additions, no FMA), across
 * slices and adds, uniform or adaptive.  Of the n samples a pixel holds (n_p after adaptive adds), n_0 = the number of even i in
 * [first_sample, first_sample + n) and n_1 = n - n_0 belong to the halves; they follow from (first_sample, n) and are stored nowhere.
 * Defining property: half h of pixel p is, bit for bit, what the in-order f32 / f64 additions of the pixel's samples of parity h give,
 * however adds and slices are cut, for either pixel order, on shards, and after adaptive adds with n = n_p.
 * Everything an accumulation returned before — the images, sem, the frame figures, the counts, both filters, the exported state — is
 * unchanged in every bit with tracking on or off: the resolve kernels are the same ones, a kernel of its own reads the radiance of a slice
 * a second time for the halves.
 * The cross filter.  Per half, in image order:  c_h = sum_h / (float)max(n_h, 1);  y_h = (float)Ybar_h, v_h = (float)V_h from the half's
 * moments with n = n_h, both NaN where n_h < 2 (as a pixel with n_p < 2 in "Adaptive sampling").  f_h is "Denoising" word for word with the
 * colours c_h and the guide (y, v) = (y_{1-h}, v_{1-h}).  Combine, per channel, every operation one IEEE f32 operation:
 *   a_h = (float)n_h;   out = (f_0 * a_0 + f_1 * a_1) / (a_0 + a_1);   out = f_0 where n_1 == 0, else f_1 where n_0 == 0.
 * Residual, every operation one IEEE f32 operation:  l(x) = (0.2126f x_r + 0.7152f x_g) + 0.0722f x_b;  d = l(f_0) - l(f_1);
 *   e_p = (d * d) * ((a_0 * a_1) / ((a_0 + a_1) * (a_0 + a_1)));   e_p = NaN where n_0 == 0 or n_1 == 0.
 * For two independent estimates with variances sigma^2 / n_h, e_p estimates the variance of their n_h-weighted mean.
 * Frame figures (RtResidual), in f64 over the pixels in image order, on the fixed tree of "Moments" (per workgroup of 256 pixels, then
 * one workgroup over the partial sums in index order; no floating-point atomics):
 *   mean_luminance = sum_p (double)l(out_p) / npix;   residual_rms = sqrt(sum_p (double)e_p / npix);
 *   residual_noise = residual_rms / mean_luminance, with the zero rule of RtNoise.noise; a NaN propagates.
 * WHAT THE FIGURE IS.  The difference of the halves sees the VARIANCE of the filtered frame; it does not see the blur that both halves
 * share.  residual_rms is therefore the variance half of the filtered frame's error — a LOWER BOUND of the error, never the error.
 * Numpy restatement on a synthetic 37 x 21 frame, two halves of 8 heavy-tailed samples, R 5, F 1:
 *   strength   RMSE cross-filtered   RMSE self-guided (16 samples)   residual_rms   true luminance RMSE
 *     0.45          0.1008                  0.0991                      0.064            0.100
 *     1.0           0.1245                  0.0980                      0.031            0.121
 * A NON-FINITE SAMPLE lands in one half.  The other half's guide is finite there, so — unlike in "Denoising" — the half that holds it is
 * filtered with finite weights and carries the value to the pixels within R of it; out, e_p and the frame figures follow (NaN).  The
 * half guided by the bad one keeps it out.  A host that must contain such pixels reads the halves and masks them, or tracks "Sample
 * buckets" below, whose read-out keeps a non-finite sample inside its bucket.
 * Half guides are noisier than the whole pixel's, so the best strength is not that of "Denoising": RT_DENOISE_HALVES_DEFAULT_STRENGTH
 * is chosen by measurement on rendered frames (DESIGN.md "Half buffers").
 * State.  RtAccumHalves carries the four planes in the row order of out_rgb_f32, as RtAccumState carries the accumulation's.  Resume is
 * rt_accum_begin, rt_accum_import, rt_accum_import_halves: from then on everything, the calls of this section included, is bit for bit
 * what the uninterrupted accumulation returns.  rt_accum_import and rt_accum_merge on an accumulation that already tracks halves are
 * RT_ERR_UNSUPPORTED and change nothing (the halves would no longer belong to the sums; a merge of halves is not covered).
 * Tracking can only be turned on while the accumulation holds no sample or — through rt_accum_import_halves — together with the halves
 * that belong to its samples, so a tracking accumulation's halves are always those of its samples.
 * Across devices: RT_MULTI_TRACK_HALVES and the joined context of rt_multi_accum_join.  Not covered: the colour-guided cross filter (channel
 * moments per half); a merge of halves; sharded frames for the filter
 * (RT_ERR_UNSUPPORTED, as rt_accum_denoise; the half images read on shards).  DESIGN.md "Half buffers". */
#define RT_DENOISE_HALVES_DEFAULT_STRENGTH 0.7f /* of 0.45, 0.7 and 1.0 by the rule of RT_DENOISE_DEFAULT_STRENGTH (DESIGN.md "Half buffers") */
typedef struct RtResidual {
    double mean_luminance;   /* (sum_p l(out_p)) / npix of the cross-filtered frame */
    double residual_rms;     /* sqrt((sum_p e_p) / npix): the variance half of the filtered frame's error, a lower bound */
    double residual_noise;   /* residual_rms / mean_luminance, the zero rule of RtNoise.noise */
    uint32_t reserved[2];
} RtResidual;
typedef struct RtAccumHalves {
    uint32_t nx, rows;           /* the shard: rows = rows_local */
    uint32_t first_sample, done; /* those of the accumulation the halves belong to */
    uint32_t reserved[2];        /* 0 */
    uint64_t frame_id;           /* rt_accum_frame_id of the frame */
    float*  sum[2];              /* [rows*nx*3] per half: the running f32 sums, NOT divided */
    double* moments[2];          /* [rows*nx*2] per half: S1, S2 */
} RtAccumHalves;
/* Makes the open accumulation track halves and clears them.  The rules of rt_accum_track_channels: after rt_accum_begin and before the
 * first add, uniform or adaptive, else RT_ERR_STATE (also after an rt_accum_import that brought samples: their halves come through
 * rt_accum_import_halves).  A second call is RT_OK and changes nothing.  Tracking ends with the accumulation.  Combines freely with
 * rt_accum_track_channels. */
int rt_accum_track_halves(RtCtx* ctx);
/* Half h of the frame so far: out_rgb_f32 [rows_local*nx*3] = sum_h / (float)max(n_h, 1); out_sem [rows_local*nx] = (float)sqrt(V_h) with
 * n = n_h, 0 where n_h < 2; the layouts of rt_accum_read, each pointer may be NULL.  Works on shards.  Synchronises the context's stream
 * once.  RT_ERR_INVALID: h > 1.  RT_ERR_STATE: no open accumulation, or it does not track halves. */
int rt_accum_read_halves(RtCtx* ctx, uint32_t h, float* out_rgb_f32, float* out_sem);
/* The cross filter above.  `dn` NULL: radius 5, patch 1, strength RT_DENOISE_HALVES_DEFAULT_STRENGTH.  out_rgb_f32 and out_rgb8 as
 * rt_accum_denoise writes them; out_err [rows_local*nx] = e_p in the row order of out_rgb_f32; each of the four outputs may be NULL.  The
 * accumulation is read and not changed.  Synchronises the context's stream once.  The errors of rt_accum_denoise, and RT_ERR_STATE where
 * the accumulation does not track halves or fewer than 4 samples are done (a uniform accumulation then has a half with n_h < 2). */
int rt_accum_denoise_halves(RtCtx* ctx, const RtDenoise* dn, float* out_rgb_f32, uint8_t* out_rgb8, float* out_err, RtResidual* res);
/* GPU-free.  RT_OK, or RT_ERR_INVALID unless: `hs` non-NULL, both reserved words 0, the four planes non-NULL, first_sample + done <=
 * 2^32 - 1.  Values are not judged. */
int rt_accum_halves_check(const RtAccumHalves* hs);
/* Fills the scalar fields of `hs` and writes every plane whose pointer is non-NULL; a NULL pointer skips that plane (all NULL: the scalar
 * fields alone, without any device work).  Reads, and changes nothing.  Synchronises the context's stream once.  RT_ERR_STATE: no open
 * accumulation, or it does not track halves. */
int rt_accum_export_halves(RtCtx* ctx, RtAccumHalves* hs);
/* Puts `hs` into the open accumulation and turns tracking on, with the allocation of rt_accum_track_halves.  Allowed while the
 * accumulation has had no add (and no merge) since rt_accum_begin — fresh with done 0, or after rt_accum_import — else RT_ERR_STATE.
 * Values are copied as bits.  RT_ERR_INVALID: rt_accum_halves_check fails, or nx, rows, frame_id, first_sample or done differ from the
 * accumulation's.  A failed call leaves the accumulation as it was.  Synchronises once. */
int rt_accum_import_halves(RtCtx* ctx, const RtAccumHalves* hs);

/* -- selected strength: the strength of the cross filter chosen per pixel from the half buffers --------------------------------------------
 * The best strength of "Half buffers" differs from frame to frame and, within a frame, from a flat wall to a contact shadow; and
 * residual_rms there "does not see the blur both halves share".  Both gaps close with what a tracking accumulation already owns: half
 * 1 - h is an independent, unbiased, noisy picture of the truth, so (l(f_h) - y_{1-h})^2 - v_{1-h} estimates the squared error of half h's
 * filtered value, BIAS INCLUDED — the dual-buffer cross-validation of Rousselle, Knaus, Zwicker 2012 / Rousselle, Manzi, Zwicker 2013.
 * It is evaluated for K candidate strengths, smoothed, the smallest picked per pixel, and the candidates blended.  New kernels only,
 * around the unchanged filter.  Every operation is one IEEE f32 operation in the order written, no FMA; f64 only in the frame figures.
 * Parameters (RtSelect).  K = n_strengths, 2 .. RT_SELECT_MAX; k_0 < k_1 < .. < k_{K-1} = strength[0 .. K-1], finite and > 0 (the
 *   entries past K are not looked at);  R = radius and F = patch as in RtDenoise;  S = error_radius and T = blend_radius, 0 .. 4 each;
 *   reserved 0.
 * With c_h, y_h, v_h, n_h, a_h, l() and "combine" exactly as "Half buffers" defines them:
 *   1. Candidates.  For j = 0 .. K-1:  f_{j,h} = the cross filter of "Half buffers" word for word with the strength k_j;
 *      out_j = combine(f_{j,0}, f_{j,1}).  out_j is, bit for bit, what rt_accum_denoise_halves returns at the strength k_j.
 *   2. Error.  r = l(f_{j,h}) - y_{1-h};  E_{j,h} = r * r - v_{1-h};  E_j = 0.5f * (E_{j,0} + E_{j,1}).  Pixel q is USABLE when E_j(q) is
 *      finite for every j (a pixel with an n_h < 2 has a NaN guide and is not).
 *   3. Smoothing.  B_j(p) = sum_{oy = -S..S} ( sum_{ox = -S..S} E_j(clamp(p + o)) ), row sums first, each sum from +0.0f, coordinates
 *      clamped to the image per axis.  The terms of pixels that are not usable are skipped, not added as 0 * x.  U(p) = the number of
 *      usable terms.
 *   4. Choice.  s = K-1, best = B_{K-1};  for j = K-2 down to 0: if (B_j < best) { s = j; best = B_j; }.  Ties go to the stronger filter,
 *      and a window without a usable pixel gives K-1.
 *   5. Blend.  W_j(p) = the number of o in [-T, T]^2 with s(clamp(p + o)) = j, an integer.  Per channel
 *      out(p) = ( sum over j in increasing order, W_j != 0 only, of (float)W_j * out_j(p) ) / (float)((2T+1)*(2T+1)); the sum starts with
 *      its first term (not with 0), so that with T = 0 out(p) = out_{s(p)}(p) in every bit.
 * Outputs.  out_index[p] = s(p);  out_est[p] = B_{s(p)}(p) / (float)U(p), NaN where U(p) = 0.
 * Frame figures (RtSelectInfo), in f64 over the pixels in image order, on the fixed tree of "Moments" (per workgroup of 256 pixels, then
 * one workgroup over the partial sums in index order; no floating-point atomics; a pixel that is not usable adds 0.0):
 *   est_mse[j] = sum_usable (double)E_j / usable;   est_mse_selected = sum_usable (double)E_{s(p)}(p) / usable;
 *   chosen[j] = the number of pixels with s(p) = j;   usable = the number of usable pixels;
 *   best = the argmin of est_mse, by the rule of step 4 (ties to the larger j): the frame-wide choice a host can hand to
 *   rt_accum_denoise_halves.  Entries j >= K are 0.  usable = 0: the figures are NaN and best = K-1.
 * WHAT THE FIGURE IS.  E estimates the LUMINANCE error of a HALF filter (n/2 samples) against the truth, blur included; the combined
 * frame is better by the variance the halves do not share.  It is unbiased only as far as the weights of f_{j,h} are independent of
 * half 1 - h's noise — and they are chosen from that half's guide, so the term -v under-corrects where the filter follows the guide's
 * noise.  est_mse_selected is biased low by the minimum taken in step 4.  DIFFERENCES between candidates are far better determined than
 * the values themselves, because the noise of y_{1-h} is common to all of them and cancels; on small frames with heavy-tailed samples
 * the values scatter by an order of magnitude around the truth while the order of the candidates holds.
 * A NON-FINITE SAMPLE: the half that holds it carries it to the pixels within R, as "Half buffers" says; every such pixel has a
 * non-finite E_j, is not usable, is left out of the windows of step 3 and of the frame figures, and takes the choice of its usable
 * neighbours; out is non-finite there, as every out_j is.
 * MEASURED on two rendered frames (cornell_box 64 x 64, 16 spp, with and without a light set; DESIGN.md "Selected strength"), RMSE of
 * rt_accum_denoise_halves at each strength, of the selection from all four with S 2, T 1, and of the selection with the defaults:
 *                      0.45      0.7       1.0       1.4     four, S 2, T 1   (0.7, 1.0, 1.4), S 0, T 1
 *   with the lights  0.09132   0.07848   0.07084   0.07490      0.07703              0.07078
 *   without          0.10343   0.09295   0.09252   0.09701      0.09476              0.08995
 * THE SELECTION FROM THE FOUR IS NOT BETTER THAN THE BEST SINGLE CANDIDATE: 8.7 % and 2.4 % worse than it, though never as bad as a wrong
 * strength.  The weakest candidate is chosen by 30 % and 55 % of the pixels: where a filter follows its own half's noise the -v term
 * under-corrects in its favour.  est_mse is within 3 to 31 % of the true luminance MSE of the half filters; `best` names the truly best
 * candidate with the lights and the second best (0.5 % behind in RMSE) without.  The defaults of a NULL `sel` are the one choice among
 * the candidate sets and windows measured that is more than 5 % better than (four, S 2, T 1) on both frames (8.1 % and 5.1 %); it is 0.1 %
 * and 2.8 % better than the best single candidate.  Two small frames decide this: a host that knows its frames passes its own RtSelect.
 * Across devices: the joined context of rt_multi_accum_join.  Not covered: selection for the luminance-, channel- or robust-guided
 * filters or on the pyramid; candidates that differ in radius or patch; sharded frames (RT_ERR_UNSUPPORTED, as rt_accum_denoise). */
#define RT_SELECT_MAX 4u
#define RT_SELECT_MAX_WINDOW 4u /* error_radius and blend_radius at the most */
typedef struct RtSelect {
    uint32_t n_strengths;  /* K: 2 .. RT_SELECT_MAX */
    float strength[4];     /* RT_SELECT_MAX of them; strictly increasing over the first K */
    uint32_t radius, patch;               /* as RtDenoise */
    uint32_t error_radius, blend_radius;  /* S, T: 0 .. RT_SELECT_MAX_WINDOW */
    uint32_t reserved;     /* 0 */
} RtSelect;
typedef struct RtSelectInfo {
    double est_mse[4];        /* per candidate: the mean of E_j over the usable pixels */
    double est_mse_selected;  /* the mean of E_{s(p)}(p): biased low by the minimum */
    uint32_t chosen[4];       /* pixels with s(p) = j */
    uint32_t usable, best;    /* usable pixels; the argmin of est_mse, ties to the larger j */
    uint32_t reserved[2];
} RtSelectInfo;
/* GPU-free.  RT_OK, or RT_ERR_INVALID unless `sel` is NULL (the defaults) or within the ranges above. */
int rt_select_check(const RtSelect* sel);
/* The selection above on the open accumulation.  `sel` NULL: strengths 0.7, 1.0, 1.4, radius 5, patch 1, error_radius 0,
 * blend_radius 1 (chosen by measurement on rendered frames: DESIGN.md "Selected strength").  out_rgb_f32 and out_rgb8 as rt_accum_denoise writes them (out_rgb8 through the context's glare and display where
 * set); out_index [rows_local*nx] = s(p) and out_est [rows_local*nx] in the row order of out_rgb_f32; every output may be NULL.  The
 * accumulation is read and not changed.  Synchronises the context's stream once.  The errors of rt_accum_denoise_halves: RT_ERR_STATE
 * without an open accumulation that tracks halves or below 4 samples; RT_ERR_UNSUPPORTED on shard_count > 1; RT_ERR_INVALID where
 * rt_select_check refuses `sel`; a failed call writes nothing.  A shard without pixels: RT_OK, nothing is written. */
int rt_accum_denoise_select(RtCtx* ctx, const RtSelect* sel, float* out_rgb_f32, uint8_t* out_rgb8, uint8_t* out_index, float* out_est,
                            RtSelectInfo* info);

/* -- sample buckets: M sums per pixel by sample index, and the median-of-means read-out that tames a firefly --------------------------------
 * Every read-out above is the plain mean sum / n, so one sample a thousand times brighter than its neighbours — a caustic path, a small
 * emitter found by chance, a NaN out of a degenerate bounce — owns its pixel for thousands of further samples, and the variance-guided
 * filters carry its colour to every pixel inside their window.  The standard remedy is the MEDIAN OF MEANS, here in the Gini-adaptive form
 * of Buisine et al. 2021 (G-MoN): the samples of every pixel are kept in M buckets by sample index, the frame is read out as a trimmed mean
 * of the sorted bucket means, and the trim follows from how unequal the bucket means are.
 * Tracking.  An accumulation that TRACKS BUCKETS also keeps, per pixel and bucket b in [0, M), an f32 x 3 sum (no moments): 12 * M bytes
 * per pixel more, in the local pixel order of the sums, allocated by rt_accum_track_buckets (or rt_accum_import_buckets) and kept for the
 * next accumulation like the other accumulation buffers.  The sample with the ABSOLUTE index i = first_sample + k goes to bucket i % M,
 * in sample order, with one IEEE f32 addition per channel (no FMA), across slices and adds, uniform or adaptive.  Of the n samples a pixel
 * holds (n_p after adaptive adds), n_b = the number of i in [first_sample, first_sample + n) with i % M == b belong to bucket b, evaluated
 * without wrap up to 2^32 - 1; n_b follows from (first_sample, n, M) and is stored nowhere.
 * Defining property: bucket b of pixel p is, bit for bit, the in-order f32 sum of the pixel's samples with i % M == b, however adds and
 * slices are cut, under every pixel order, on shards, and after adaptive adds with n = n_p.
 * Everything an accumulation returned before — the images, sem, the frame figures, the counts, all three filters, the exported states,
 * the launch ledger of an add — is unchanged in every bit with tracking on or off: the resolve kernels are the same ones, a kernel of its
 * own reads the radiance of a slice once more for the buckets.
 * The robust read-out.  Per pixel and per channel, every operation one IEEE f32 operation in this order:
 *   1. For b = 0 .. M - 1 with n_b > 0:  m_b = sum_b / (float)n_b.  The finite ones (m_b - m_b == 0) are kept; K is their number,
 *      x_0 <= .. <= x_{K-1} their ascending order.  Ties and +-0 may sort in any order: every sum below starts from +0, so no output bit
 *      depends on it.  K == 0: out = NaN, t = 0.
 *   2. s = 0; w = 0; for i = 0 .. K - 1:  s = s + x_i;  w = w + (float)(i + 1) * x_i.
 *   3. The trim t per side.  RT_ROBUST_MEDIAN: t = (K - 1) / 2.  RT_ROBUST_TRIM: t = min(RtRobust.trim, (K - 1) / 2).  RT_ROBUST_GINI:
 *      t = 0 when K < 2 or !(s > 0); else  G = (2.0f * w) / ((float)K * s) - ((float)(K + 1) / (float)K);
 *      Gn = G * ((float)K / (float)(K - 1));  t = Gn > 0 ? min((uint32_t)((Gn * (float)K) * 0.5f), (K - 1) / 2) : 0.
 *   4. a = 0; for i = t .. K - 1 - t:  a = a + x_i;  out = a / (float)(K - 2 * t);  out_trim = t.
 * So bucket means that agree give the mean of means (Gn = 0), and bucket means dominated by one or two buckets give their median.  A NaN
 * or inf sample stays inside its bucket and never reaches `out` while another bucket of the pixel is finite: the containment that "Half
 * buffers" left to the host.  out_rgb8 is the quantisation of rt_accum_read applied to `out`.
 * WHAT THE ESTIMATOR IS.  It is BIASED.  A trimmed mean removes energy that belongs to the integral — the bright tail of an honest
 * pixel as well as a firefly — and RtRobustInfo.energy_removed says how much of the frame's luminance went.  It is not a denoiser: where
 * EVERY pixel is heavy-tailed at a low sample count it loses against the plain mean.  Numpy restatement on a 37 x 21 frame, RMSE against
 * the truth:
 *                                                              n     M    plain mean    GINI    MEDIAN
 *   samples U(0.5, 1.5), one in 500 brighter by 200            64    5      0.545       0.296    0.194
 *   the same                                                  1024   9      0.130       0.120    0.201    (MEDIAN now loses: its bias stays)
 *   every sample heavy-tailed (the frame of "Half buffers")     16   5      0.216       0.306    0.338    (both lose)
 * with the frame's mean value at n = 64: 0.583 plain, 0.439 GINI, truth 0.586.  Rendered frames: DESIGN.md "Sample buckets".
 * Frame figures (RtRobustInfo), in f64 over the pixels in image order, on the fixed tree of "Moments" (per workgroup of 256 pixels, then
 * one workgroup over the partial sums in index order; no floating-point atomics), l the f32 luminance of "Half buffers":
 *   mean_luminance_plain = sum_p (double)l(c_p) / npix with c_p = sum_p / (float)max(n_p, 1);  mean_luminance_robust likewise over out_p;
 *   energy_removed = 1 - mean_luminance_robust / mean_luminance_plain, 0 where both are 0; a NaN propagates;
 *   trimmed_fraction = (pixel-channels with t > 0) / (3 npix);  nonfinite_dropped = the bucket means dropped in step 1, an exact count.
 * The filter on robust colours is "Denoising" word for word with the colours c replaced by `out`; the guide (y, v) comes unchanged from the
 * luminance moments.  A firefly pixel's large v still makes its neighbours accept it, but what they now accept is the tamed colour.
 * State.  RtAccumBuckets carries the M planes in the row order of out_rgb_f32.  Resume is rt_accum_begin, rt_accum_import, optionally
 * rt_accum_import_halves, then rt_accum_import_buckets: from then on everything, the calls of this section included, is bit for bit what
 * the uninterrupted accumulation returns.  rt_accum_import and rt_accum_merge on an accumulation that already tracks buckets are
 * RT_ERR_UNSUPPORTED and change nothing.  Tracking can only be turned on while the accumulation holds no sample or — through
 * rt_accum_import_buckets — together with the buckets that belong to its samples.
 * Across devices: RT_MULTI_TRACK_BUCKETS and the joined context of rt_multi_accum_join.  Not covered: a merge of buckets; rt_render_to_noise
 * and rt_render_adaptive, which open their own accumulation; a robust form
 * of the channel-guided and the cross filter; an adaptive criterion on the robust estimate; sharded frames for the filter
 * (RT_ERR_UNSUPPORTED, as rt_accum_denoise; the read-out works on shards).  DESIGN.md "Sample buckets". */
#define RT_BUCKETS_MAX 16u
#define RT_ROBUST_GINI 0u
#define RT_ROBUST_MEDIAN 1u
#define RT_ROBUST_TRIM 2u
typedef struct RtRobust {
    uint32_t mode;         /* RT_ROBUST_* */
    uint32_t trim;         /* RT_ROBUST_TRIM: bucket means dropped per side, clamped to (K - 1) / 2; not looked at otherwise */
    uint32_t reserved[2];  /* 0 */
} RtRobust;
typedef struct RtRobustInfo {
    double mean_luminance_plain;   /* (sum_p l(c_p)) / npix of the plain mean */
    double mean_luminance_robust;  /* (sum_p l(out_p)) / npix of the robust read-out */
    double energy_removed;         /* 1 - robust / plain: the share of the frame's luminance the trim took away (the bias, and the fireflies) */
    double trimmed_fraction;       /* pixel-channels with t > 0, over 3 npix */
    uint64_t nonfinite_dropped;    /* bucket means dropped as NaN or inf */
} RtRobustInfo;
typedef struct RtAccumBuckets {
    uint32_t nx, rows;             /* the shard: rows = rows_local */
    uint32_t first_sample, done;   /* those of the accumulation the buckets belong to */
    uint32_t M, reserved;          /* 3 .. RT_BUCKETS_MAX; 0 */
    uint64_t frame_id;             /* rt_accum_frame_id of the frame */
    float* sum[16];                /* RT_BUCKETS_MAX of them; [rows*nx*3] per bucket b < M: the running f32 sums, NOT divided; the pointers past M are not looked at */
} RtAccumBuckets;
/* Makes the open accumulation track M buckets, 3 <= M <= RT_BUCKETS_MAX, and clears them.  The rules of rt_accum_track_halves: after
 * rt_accum_begin and before the first add, uniform or adaptive, else RT_ERR_STATE (also after an rt_accum_import that brought samples:
 * their buckets come through rt_accum_import_buckets).  A second call with the same M is RT_OK and changes nothing; with another M it is
 * RT_ERR_STATE.  RT_ERR_INVALID: M outside the range.  RT_ERR_NOMEM leaves the accumulation untracked.  Tracking ends with the
 * accumulation.  Combines freely with rt_accum_track_channels and rt_accum_track_halves. */
int rt_accum_track_buckets(RtCtx* ctx, uint32_t M);
/* The robust read-out above.  `rb` NULL: RT_ROBUST_GINI.  out_rgb_f32 and out_rgb8 in the layouts of rt_accum_read; out_trim
 * [rows_local*nx*3] = t per pixel and channel in the row order of out_rgb_f32; every output may be NULL.  The accumulation is read and not
 * changed.  Works on shards.  Synchronises the context's stream once.  RT_ERR_INVALID: a mode above RT_ROBUST_TRIM or a reserved word
 * that is not 0.  RT_ERR_STATE: no open accumulation, it does not track buckets, or fewer than 1 sample is done. */
int rt_accum_read_robust(RtCtx* ctx, const RtRobust* rb, float* out_rgb_f32, uint8_t* out_rgb8, uint8_t* out_trim, RtRobustInfo* info);
/* The filter on robust colours above.  `rb` and `dn` NULL: RT_ROBUST_GINI; radius 5, patch 1, strength RT_DENOISE_DEFAULT_STRENGTH.
 * out_rgb_f32 and out_rgb8 as rt_accum_denoise writes them; either may be NULL.  The errors of rt_accum_denoise and of
 * rt_accum_read_robust. */
int rt_accum_denoise_robust(RtCtx* ctx, const RtRobust* rb, const RtDenoise* dn, float* out_rgb_f32, uint8_t* out_rgb8);
/* GPU-free.  RT_OK, or RT_ERR_INVALID unless: `bs` non-NULL, reserved 0, 3 <= M <= RT_BUCKETS_MAX, sum[0] .. sum[M - 1] non-NULL,
 * first_sample + done <= 2^32 - 1.  Values are not judged. */
int rt_accum_buckets_check(const RtAccumBuckets* bs);
/* Fills the scalar fields of `bs` and writes every plane b < M whose pointer is non-NULL; a NULL pointer skips that plane (all NULL: the
 * scalar fields alone, without any device work).  Reads, and changes nothing.  Synchronises the context's stream once.  RT_ERR_STATE: no
 * open accumulation, or it does not track buckets. */
int rt_accum_export_buckets(RtCtx* ctx, RtAccumBuckets* bs);
/* Puts `bs` into the open accumulation and turns tracking on, with the allocation of rt_accum_track_buckets.  Allowed while the
 * accumulation has had no add (and no merge) since rt_accum_begin — fresh with done 0, or after rt_accum_import — else RT_ERR_STATE.
 * Values are copied as bits.  RT_ERR_INVALID: rt_accum_buckets_check fails, or nx, rows, frame_id, first_sample or done differ from the
 * accumulation's, or M from that of an accumulation that tracks already.  A failed call leaves the accumulation as it was.  Synchronises
 * once. */
int rt_accum_import_buckets(RtCtx* ctx, const RtAccumBuckets* bs);

/* -- multi-scale denoising: the filter on a 2x pyramid ---------------------------------------------------------------------------------------
 * The window of "Denoising" is at most 21 x 21 pixels; noise of a longer wavelength passes it and shows as low-frequency blotches.  The
 * standard cure filters a 2x image pyramid and lets every coarser level replace the low frequencies of the finer one (Rousselle et al.
 * 2012; Delbracio et al. 2014: "Boosting Monte Carlo rendering by ray histogram fusion"; Boughida, Boubekeur 2017), for about
 * 1/4 + 1/16 + .. of the single-scale filter on top of it.  New kernels only, around the unchanged filter of the chosen guide.
 * Every operation is one IEEE f32 operation in the order written, no FMA.
 * Levels.  L = levels, 1 .. RT_DENOISE_MAX_LEVELS.  Level 0 is the frame: nx_0 = nx, rows_0 = rows;  nx_{s+1} = (nx_s + 1) / 2 and
 *   rows_{s+1} = (rows_s + 1) / 2, integer division (rt_denoise_level_size).  There are always exactly L levels; a side of 1 stays 1.
 * Inputs of level 0.  Exactly what the single-scale filter of the guide reads, for uniform and adaptive accumulations alike, the NaN
 *   guide of a pixel with n_p < 2 included.  RT_DENOISE_GUIDE_LUMINANCE: c (3 floats), y, v of "Denoising".  RT_DENOISE_GUIDE_CHANNELS: c
 *   and the three channel variances of "Channel moments and the colour-guided filter"; the guide means are c.
 * Downsample D (level s -> s + 1).  For the coarse pixel (X, Y) and a plane a of level s:
 *   t00 = a(2X, 2Y), t10 = a(2X+1, 2Y), t01 = a(2X, 2Y+1), t11 = a(2X+1, 2Y+1), a tap outside the level-s image +0.0f;
 *   sum = (t00 + t10) + (t01 + t11);   kx = 1 + (2X+1 < nx_s), ky = 1 + (2Y+1 < rows_s), k = kx * ky in {1, 2, 4};
 *   a mean plane — the colour channels, y, the channel means — is sum * (1/k);  a variance plane is sum * (1/(k*k)), the variance of a
 *   mean of k independent pixel means.  The four multipliers 1, 0.5, 0.25, 0.0625 are powers of two: the scale is exact.
 * Filter.  F_s = the filter of the guide over the inputs of level s, with the caller's R, F and strength on every level.
 * Combine, from coarse to fine.  o_{L-1} = F_{L-1}.  For s = L-2 .. 0:
 *   at level s+1, per channel:  e = o_{s+1} - D(F_s), D in the mean form;  an e that is not finite is replaced by +0.0f;
 *   at level s, per pixel (x, y) and channel:
 *     o_s = F_s + ((0.5625f * e(X, Y) + 0.1875f * e(X', Y)) + (0.1875f * e(X, Y') + 0.0625f * e(X', Y'))),
 *     X = x >> 1,  X' = clamp(X + ((x & 1) ? 1 : -1), 0, nx_{s+1} - 1);  Y and Y' likewise from y and rows_{s+1}:
 *   the 2x bilinear interpolation at pixel centres, clamped at the border.
 * Output.  o_0; out_rgb8 is o_0 through the quantisation and flip of rt_render.
 * Properties (tests/denoise_multiscale_ref.py restates all of it in numpy, and the kernels are held to it bit for bit):
 *   L = 1 is the single-scale filter of the same guide, bit for bit.
 *   A non-finite pixel stays itself and spreads to no other: its coarse pixel is non-finite, which the filter leaves alone while it skips
 *   every patch that holds it; the e of that coarse pixel become 0, so its three finite siblings get their level-0 result.
 *   A constant dyadic image without variance comes back bit for bit.
 *   The accumulation is read and not changed.
 * Cost: the levels above 0 take about a third of level 0 in time and memory (DESIGN.md "Multi-scale denoising").
 * Not covered: the cross-filtered halves of "Half buffers" and the robust read-out of "Sample buckets" (both stay single-scale); sharded
 * frames (RT_ERR_UNSUPPORTED, as rt_accum_denoise: on an RtMulti the filter runs on the joined context of rt_multi_accum_join). */
typedef struct RtMultiscale {
    uint32_t levels, guide; /* 1 .. RT_DENOISE_MAX_LEVELS; RT_DENOISE_GUIDE_* */
    uint32_t reserved[2];   /* 0 */
} RtMultiscale;
#define RT_DENOISE_MAX_LEVELS 4u
#define RT_DENOISE_GUIDE_LUMINANCE 0u
#define RT_DENOISE_GUIDE_CHANNELS 1u
#define RT_DENOISE_DEFAULT_LEVELS 2u /* 2 unless 3 is more than 5 % better on both cornell frames (DESIGN.md "Multi-scale denoising") */
/* GPU-free, no context.  The size of level `level` (0 .. RT_DENOISE_MAX_LEVELS - 1) of a frame of nx x rows pixels into *nx_l and
 * *rows_l (each may be NULL).  RT_ERR_INVALID: nx or rows 0, or a level outside the range. */
int rt_denoise_level_size(uint32_t nx, uint32_t rows, uint32_t level, uint32_t* nx_l, uint32_t* rows_l);
/* The multi-scale filter above over the frame of the open accumulation.  `dn` as rt_accum_denoise reads it; `ms` NULL:
 * RT_DENOISE_DEFAULT_LEVELS levels with the luminance guide.  Outputs, the untouched accumulation, the one synchronisation and every
 * error are those of the single-scale call of the same guide — rt_accum_denoise, or rt_accum_denoise_channels with its RT_ERR_STATE where
 * the accumulation does not track channels.  In addition RT_ERR_INVALID: levels 0 or above RT_DENOISE_MAX_LEVELS, an unknown guide,
 * reserved != 0. */
int rt_accum_denoise_multiscale(RtCtx* ctx, const RtDenoise* dn, const RtMultiscale* ms, float* out_rgb_f32, uint8_t* out_rgb8);

/* -- display transform: exposure, tone curve, transfer function and dither behind every 8-bit read-out of an accumulation -----------------
 * Every out_rgb8 above is the reference driver's quantisation, sqrt(c) * 255.99 saturating: radiance above 1 clips (emitters, their
 * surround, fireflies), a dark frame has no exposure, a denoised gradient shows the bands its noise used to dither away, and gamma 2 is
 * not the sRGB a PNG viewer assumes.  A DISPLAY set on a context replaces that one step — on the device, behind the same single wait —
 * for the out_rgb8 of rt_accum_read, rt_accum_denoise, rt_accum_denoise_channels, rt_accum_denoise_halves, rt_accum_denoise_robust,
 * rt_accum_denoise_multiscale and rt_accum_read_robust (and of rt_render_to_noise and rt_render_adaptive, which end in rt_accum_read):
 * out_rgb8 is the transform below of the f32 image the same call returns.  Nothing else changes in any bit: out_rgb_f32, out_sem, every
 * figure, state and export; no sample, sum or moment is touched, and no existing kernel.  It works on a shard; the statistics are then
 * those of the shard's pixels, as the noise figures are.
 * Every f32 operation is one IEEE operation in the order written, no FMA; `/` and sqrtf are correctly rounded.
 * Input.  Pixel c = (r, g, b) of the f32 image in the call's row order; e = the exposure.
 * Statistics (only where exposure_mode is not RT_EXPOSURE_MANUAL, whose e = exposure_value):
 *   Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b in f32.  A pixel is LIT iff Y is finite and Y > 0; n_lit counts them.
 *   RT_EXPOSURE_KEY: S = the sum of log((double)Y) over the lit pixels, in f64 on the fixed tree of the frame figures ("Frame figures":
 *     per 256 consecutive pixels of the image lanes then waves, then one workgroup over those partial sums in index order; a pixel that
 *     is not lit adds 0.0).  Lavg = exp(S / (double)n_lit);  e = (float)((double)exposure_value / Lavg).
 *   RT_EXPOSURE_PERCENTILE: a histogram of the lit pixels over bin = bits(Y) >> 20 — 2048 bins, 8 per octave, integer arithmetic only,
 *     u32 counts.  rank = max(1, ceil((double)percentile * (double)n_lit));  b = the first bin whose cumulative count reaches rank;
 *     L_q = the f32 with the bits (b << 20) | 0x80000, the middle of the bin;  e = (float)((double)exposure_value / (double)L_q).
 *   n_lit == 0, or an e that is zero or not finite: e = 1.
 * Per pixel.  If any channel of c is not finite the pixel counts in n_non_finite and each channel is written as: NaN 0, -inf 0, +inf 255,
 *   a finite one as under RT_TONE_CLAMP below (with the display's transfer and dither).  Otherwise, per channel, x = e * c, then
 *   x = x > 0 ? x : 0.
 * Curve.  RT_TONE_CLAMP: t = x.
 *   RT_TONE_REINHARD: L = the luminance of x by the formula of Y;  s = (1 + L / (white * white)) / (1 + L);  t = x * s per channel
 *     (white = +inf: s = 1 / (1 + L)).
 *   RT_TONE_ACES (Narkowicz 2015, "ACES filmic tone mapping curve"), per channel:  x = x < 65536.0f ? x : 65536.0f;
 *     t = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f).
 * Transfer.  RT_TRANSFER_GAMMA2: y = sqrtf(t).
 *   RT_TRANSFER_SRGB: y = t <= 0.0031308f ? 12.92f * t : 1.055f * p - 0.055f,  p = (float)pow((double)t, 1.0 / 2.4): the power in f64,
 *     rounded to f32 once, the product and the difference in f32.  The f64 pow of a conforming library is within 16 ulp (the device's and
 *     glibc's are within 1), so two implementations agree on p except within 2^-48 of a rounding boundary, where they differ by one ulp
 *     of p; through 1.055f * p - 0.055f, which amplifies a relative error by 1.055 p / y <= 2.36, two y differ by less than 3 ulp of the
 *     product: RT_DISPLAY_SRGB_EPS = 2^-20 relative (14.2 * 2^-24, rounded up) bounds the difference of any two implementations.
 * Quantisation, with k_finalize's row flip: i = the column and r = the row of out_rgb8, 0 at the top.
 *   RT_DITHER_NONE: g = y * 255.99f.
 *   RT_DITHER_BAYER8: g = y * 255.0f + ((float)B(i & 7, r & 7) + 0.5f) / 64.0f,  B(x, y) = the OR over k = 0 .. 2 of
 *     (((x ^ y) >> k) & 1) << (2 * (2 - k) + 1)  |  ((y >> k) & 1) << (2 * (2 - k)):  the standard 8 x 8 Bayer index, a permutation of
 *     0 .. 63 with the first row 0 32 8 40 2 34 10 42.  The offsets are 1/128 .. 127/128: an ordered dither of one level's width.
 *   In both: u = (g == g && g > 0) ? (g >= 255 ? 255 : (uint32_t)g) : 0, the rule of rt_render's quantisation.
 * Properties (tests/display_ref.py restates all of it in numpy; the kernels are held to it bit for bit, under RT_TRANSFER_SRGB outside
 * the values whose level differs between y (1 - eps) and y (1 + eps)):
 *   {RT_EXPOSURE_MANUAL, 1.0f, .., RT_TONE_CLAMP, .., RT_TRANSFER_GAMMA2, RT_DITHER_NONE} gives the out_rgb8 of no display, bit for bit.
 *   The same image gives the same e and the same figures on every run: no floating-point atomic takes part.
 * Not covered: rt_render, rt_render_device, the preview of rt_set_progress and rt_multi_render keep the reference quantisation, and so do
 * the contexts of an RtMulti (the joined context of rt_multi_accum_join included).  DESIGN.md "Display transform". */
enum RtExposureMode { RT_EXPOSURE_MANUAL = 0, RT_EXPOSURE_KEY = 1, RT_EXPOSURE_PERCENTILE = 2 };
enum RtToneCurve { RT_TONE_CLAMP = 0, RT_TONE_REINHARD = 1, RT_TONE_ACES = 2 };
enum RtTransfer { RT_TRANSFER_GAMMA2 = 0, RT_TRANSFER_SRGB = 1 };
enum RtDither { RT_DITHER_NONE = 0, RT_DITHER_BAYER8 = 1 };
#define RT_DISPLAY_SRGB_EPS 9.5367431640625e-07 /* 2^-20 */
typedef struct RtDisplay {
    uint32_t exposure_mode; /* RtExposureMode */
    float exposure_value;   /* MANUAL: the multiplier e; KEY: the key (0.18); PERCENTILE: the linear level the percentile maps to; finite, > 0 */
    float percentile;       /* PERCENTILE: q in (0, 1]; else ignored */
    uint32_t curve;         /* RtToneCurve */
    float white;            /* REINHARD: the white point, > 0, +inf allowed; else ignored */
    uint32_t transfer, dither, reserved; /* RtTransfer, RtDither, 0 */
} RtDisplay;
typedef struct RtDisplayInfo {
    float exposure;             /* the e that was applied */
    float percentile_luminance; /* PERCENTILE: L_q (0 where nothing is lit), else 0 */
    double log_average;         /* KEY: exp(S / n_lit) (0 where nothing is lit), else 0 */
    uint64_t n_lit;             /* pixels with finite Y > 0; MANUAL: 0, no statistics run */
    uint64_t n_non_finite;      /* pixels with a non-finite channel */
    uint64_t n_saturated;       /* channel values written as 255 */
} RtDisplayInfo;
/* A per-context setting, as rt_set_lens and rt_set_progress are, but one that changes no sample: it does NOT end an open accumulation,
 * and rt_scene_upload leaves it.  `display` NULL: no display, the reference quantisation, bit for bit.  RT_ERR_INVALID: what
 * rt_display_check refuses; the display set before stays in force. */
int rt_set_display(RtCtx* ctx, const RtDisplay* display);
/* The figures of the last out_rgb8 this context wrote under a display.  RT_ERR_STATE: there was none. */
int rt_display_info(RtCtx* ctx, RtDisplayInfo* info);
/* GPU-free, no context.  RT_OK, or RT_ERR_INVALID: `display` NULL, an enum out of range, exposure_value not finite or <= 0, percentile
 * outside (0, 1] under RT_EXPOSURE_PERCENTILE, white NaN or <= 0 under RT_TONE_REINHARD, reserved != 0. */
int rt_display_check(const RtDisplay* display);

/* -- Glare: an energy-conserving bloom in front of the display stage ------------------------------------------------------------------------
 * Every stage of the display transform works on one pixel: a light a thousand times brighter than its surround still ends as a hard-edged
 * white disc.  A GLARE set on a context carries a share of every pixel's energy into its neighbourhood — what an eye or a lens does —
 * before the display stage of every out_rgb8 a display can stand behind: rt_accum_read, rt_accum_denoise, rt_accum_denoise_channels,
 * rt_accum_denoise_halves, rt_accum_denoise_robust, rt_accum_denoise_multiscale and rt_accum_read_robust (and rt_render_to_noise and
 * rt_render_adaptive, which end in rt_accum_read).  `out` below replaces "the f32 image" as the display stage's input, for its statistics
 * and for its per-pixel transform; with no display set, `out` goes through the reference quantisation, which is the display of the
 * identity configuration.  Nothing else changes in any bit: out_rgb_f32, out_sem, every figure, state and export, and no existing kernel.
 * Every f32 operation is one IEEE operation in the order written, no FMA.
 * Input.  Pixel c of the f32 image in the call's row order, nx x rows; a = amount; L = levels.
 * 1. Sanitise, per channel: s = (c is finite && c > 0) ? min(c, 0x1p64f) : +0.0f.
 *    No sum below can overflow: s <= 2^64; k <= 1, so b <= s; a mean of up to four such values, their sum at most 2^66 before the scale,
 *    is <= 2^64 (1 + 2^-22) per level; the weights are positive and sum to 1 within Le ulp, and U's weights sum to 1, so every u_l and B
 *    stay below 2^65; a <= 1: (s - a b) + a B < 2^66, far from 2^128.
 * 2. Bright pass.  threshold == 0: b = s.  Otherwise Y = (0.2126f * s_r + 0.7152f * s_g) + 0.0722f * s_b (the display's luminance),
 *    k = Y > threshold ? (Y - threshold) / Y : 0, b = s * k per channel.
 * 3. Down.  d_0 = b, d_l = D(d_{l-1}) for l = 1 .. Le.  D is the mean form of "multi-scale denoising": the four taps of a coarse pixel,
 *    those outside the image +0, summed as (t00 + t10) + (t01 + t11) and scaled by 1 / k for k taps inside.  Level sizes:
 *    rt_denoise_level_size.  Le = min(L, the first level whose larger side is 1); Le = 0 for a 1 x 1 image: out = s where c is finite.
 * 4. Weights (host, f32).  w_1 = 1, w_{l+1} = w_l * spread; W = ((w_1 + w_2) + ..) over l = 1 .. Le in index order; ŵ_l = w_l / W.
 * 5. Up.  u_Le = ŵ_Le * d_Le; u_l = ŵ_l * d_l + U(u_{l+1}) for l = Le - 1 .. 1; B = U(u_1).  U is the clamped 2x bilinear interpolation
 *    of "multi-scale denoising": (0.5625f e(X, Y) + 0.1875f e(X', Y)) + (0.1875f e(X, Y') + 0.0625f e(X', Y')).
 * 6. Combine, per channel.  Every channel of c finite: out = (s - a * b) + a * B.  Otherwise out = c, all three channels unchanged, so
 *    that the display's non-finite rule and count still see the pixel (its finite, positive channels still glow into its neighbours).
 * Properties (tests/glare_ref.py restates all of it in numpy; the kernels are held to it bit for bit, and the host tests prove these on
 * the reference alone):
 *   A constant image stays that constant, within the 9 Le + 4 f32 roundings on the longest path to `out` (tests/glare_ref.py counts them).
 *   With threshold 0 the frame's energy is conserved for light that lies at least 2^(Le+1) pixels from every edge of a frame whose
 *   sides are multiples of 2^Le: D's weights sum to 1 per fine pixel there, U's per coarse pixel.
 *   At the edges the frame continues with its edge values: U clamps, D averages the taps it has.  An emitter on the edge glows as though
 *   it went on beyond it, and a pixel in the last row or column of an odd-sized level counts for more than its neighbours — under the
 *   default glare an impulse in the odd corner (52, 36) of a 53 x 37 frame comes out with 70 % more energy, one in the even corner (0, 0)
 *   with 0.4 % less (with amount 1 ten times that).  That is a consequence of the border rule and is left as it is.
 *   out >= 0 wherever c is finite: a b <= b <= s by the monotonicity of rounding.
 *   amount == 0 gives the out_rgb8 of no glare bit for bit; the f32 `out` differs from c only where c < 0 or c > 2^64 (and in the sign of
 *   a -0), which the quantisation maps to the same level.
 *   The point spread of a pixel depends on where it sits in its 2^l blocks: a property of the pyramid, which is not shift invariant.
 * A shard (shard_count > 1) has no neighbourhoods — its rows are interleaved with other devices': a call that asks for out_rgb8 under a
 * glare is RT_ERR_STATE there; calls that ask for no out_rgb8 are unaffected.
 * Not covered, as for the display: rt_render, rt_render_device, the preview of rt_set_progress, and every context of an RtMulti.
 * Cost: 12 B per pixel for `out` and 8 B for the pyramid; DESIGN.md "Glare". */
#define RT_GLARE_MAX_LEVELS 8u
#define RT_GLARE_DEFAULT_LEVELS 6u
#define RT_GLARE_DEFAULT_AMOUNT 0.1f
#define RT_GLARE_DEFAULT_SPREAD 0.7f
typedef struct RtGlare {
    float amount;    /* a in [0, 1]: the share of the bright pass that leaves its pixel */
    float spread;    /* in (0, 1]: the weight of a level relative to the next finer one; 1: all levels alike, the widest glow */
    float threshold; /* finite, >= 0: the luminance below which a pixel does not glow; 0: every pixel does, and energy is conserved */
    uint32_t levels; /* L in 1 .. RT_GLARE_MAX_LEVELS: the coarsest level's pixels are 2^L wide */
} RtGlare;
typedef struct RtGlareInfo {
    uint32_t levels;                  /* Le */
    uint32_t coarse_nx, coarse_rows;  /* the size of level Le */
    uint32_t reserved;                /* 0 */
} RtGlareInfo;
/* A per-context setting under the rules of rt_set_display: it does NOT end an open accumulation, and rt_scene_upload leaves it.  `glare`
 * NULL: no glare.  RT_ERR_INVALID: what rt_glare_check refuses; the glare set before stays in force. */
int rt_set_glare(RtCtx* ctx, const RtGlare* glare);
/* GPU-free, no context.  RT_OK, or RT_ERR_INVALID: `glare` NULL, a NaN in any field, amount outside [0, 1], spread outside (0, 1],
 * threshold negative or not finite, levels 0 or above RT_GLARE_MAX_LEVELS. */
int rt_glare_check(const RtGlare* glare);
/* Le and the size of the coarsest level of the last out_rgb8 this context wrote under a glare.  RT_ERR_STATE: there was none. */
int rt_glare_info(RtCtx* ctx, RtGlareInfo* info);
/* `out` of that last call: out_rgb_f32 [3 * nx * rows] in the call's row order.  RT_ERR_STATE: there was none. */
int rt_glare_image(RtCtx* ctx, float* out_rgb_f32);

/* -- pixel reconstruction filters: tent, Gaussian, Mitchell-Netravali and Blackman-Harris instead of the box ---------------------------------
 * The running sum of an accumulation is the reference's: sample s of pixel p counts for p alone with weight 1 wherever inside the pixel it
 * fell (main.rs:95-97), a box of radius 0.5.  An accumulation that TRACKS A FILTER also keeps, per pixel, (sum w r, sum w g, sum w b,
 * sum w) in f32 — 16 B per pixel more, in the local pixel order of the sums — over the samples of the pixel AND of its neighbours, each
 * weighted by a separable filter of one radius R, in pixels, at its distance from the pixel's centre.  The sub-pixel position of a sample
 * is not stored: it is the first two draws of the path's key (DESIGN.md "RNG", counters 0 and 1), recomputed from (seed, pixel, sample).
 * The filter.  f(|x|) for |x| <= R, RT_FILTER_MIN_RADIUS <= R <= RT_FILTER_MAX_RADIUS:
 *   RT_FILTER_BOX             1
 *   RT_FILTER_TENT            1 - x / R
 *   RT_FILTER_GAUSSIAN        exp(-x^2 / (2 sigma^2)) - exp(-R^2 / (2 sigma^2)),  sigma = p0 > 0
 *   RT_FILTER_MITCHELL        with B = p0, C = p1 and t = 2 x / R:  ((12 - 9B - 6C) t^3 + (-18 + 12B + 6C) t^2 + (6 - 2B)) / 6 for t < 1,
 *                             ((-B - 6C) t^3 + (6B + 30C) t^2 + (-12B - 48C) t + (8B + 24C)) / 6 else (negative lobes where C > 0)
 *   RT_FILTER_BLACKMAN_HARRIS 0.35875 + 0.48829 cos(a) + 0.14128 cos(2a) + 0.01168 cos(3a),  a = pi x / R
 * The TABLE.  The host evaluates f in f64 at the midpoints x_k = (k + 0.5) R / RT_FILTER_TABLE, k = 0 .. RT_FILTER_TABLE - 1, and rounds each
 * value once to f32 (rt_pixel_filter_table returns exactly what the device uses).  The device evaluates no profile: it looks the table up.
 * The REACH.  D = ceil(R + 0.5) - 1 pixels: R 0.5 -> 0, (0.5, 1.5] -> 1, (1.5, 2.5] -> 2, (2.5, 3] -> 3.
 * Defining property.  With (jx, jy) = the draws 0 and 1 of path_key(seed, q, i) as f32 in [0, 1), every operation below one IEEE f32
 * operation without contraction, for the samples i of the accumulation in ascending order:
 *   for dy = -D .. D ascending, for dx = -D .. D ascending, q = (i_p + dx, j_p + dy) inside the frame (and, in an adaptive add, active):
 *     ox = ((float)dx + jx) - 0.5f;  ax = |ox|;  skip where ax > R;  kx = min((uint32_t)(ax * (256.0f / R)), 255);   likewise oy, ay, ky
 *     w = table[kx] * table[ky];   sum.rgb += w * radiance(q, i).rgb;   sum.w += w
 * The plane is that, bit for bit, however adds and slices are cut and for either pixel order: a gather, no atomics.  A pixel that has
 * converged in an adaptive accumulation gets no samples of its own and keeps receiving those of its active neighbours.
 * Read-out.  c = sum.rgb / sum.w and W = sum.w; where !(W > 0) — no sample yet, or a negative-lobe filter whose weights cancel — the pixel
 * is the box mean of rt_accum_read.  out_rgb8 goes where the denoisers' goes: the reference quantisation, or the context's glare and
 * display.  With RT_FILTER_BOX at R 0.5 the plane's rgb is the accumulation's sum, W is (float)n and the read-out is rt_accum_read's, bit
 * for bit.
 * Everything an accumulation returned before is unchanged in every bit with tracking on or off: a kernel of its own reads the radiance of a
 * slice a second time.
 * State.  RtAccumFilter carries the filter and the plane in the row order of out_rgb_f32.  Resume is rt_accum_begin, rt_accum_import,
 * rt_accum_import_filter: from then on the plane and the read-out are bit for bit those of the uninterrupted accumulation.
 * rt_accum_import and rt_accum_merge on an accumulation that tracks a filter are RT_ERR_UNSUPPORTED and change nothing.
 * Not covered: sharded frames and rt_multi_accum_* (a row-interleaved shard has no neighbourhoods: RT_ERR_STATE); a merge of filter planes;
 * a denoiser on the filtered image (its pixels are correlated, and the variance guides do not describe it); anisotropic radii.
 * DESIGN.md "Pixel reconstruction filters". */
#define RT_FILTER_BOX             0u
#define RT_FILTER_TENT            1u
#define RT_FILTER_GAUSSIAN        2u /* p0 = sigma */
#define RT_FILTER_MITCHELL        3u /* p0 = B, p1 = C */
#define RT_FILTER_BLACKMAN_HARRIS 4u
#define RT_FILTER_TABLE 256u
#define RT_FILTER_MIN_RADIUS 0.5f
#define RT_FILTER_MAX_RADIUS 3.0f
typedef struct RtPixelFilter {
    uint32_t kind;   /* RT_FILTER_* */
    float radius;    /* R, in pixels */
    float p0, p1;    /* the kind's parameters; finite, 0 where the kind has none */
} RtPixelFilter;
typedef struct RtAccumFilter {
    uint32_t nx, rows;           /* the frame: rows = ny (no shards) */
    uint32_t first_sample, done; /* those of the accumulation the plane belongs to */
    uint32_t reserved[2];        /* 0 */
    uint64_t frame_id;           /* rt_accum_frame_id of the frame */
    RtPixelFilter filter;        /* the filter the plane was summed under */
    float* plane;                /* [rows*nx*4]: sum w r, sum w g, sum w b, sum w — NOT divided */
} RtAccumFilter;
/* GPU-free, no context.  RT_OK, or RT_ERR_INVALID: `filter` NULL, a kind outside the enum, a non-finite field, a radius outside
 * [RT_FILTER_MIN_RADIUS, RT_FILTER_MAX_RADIUS], a Gaussian with sigma <= 0. */
int rt_pixel_filter_check(const RtPixelFilter* filter);
/* GPU-free, no context.  table [RT_FILTER_TABLE] and *reach = D as defined above; either may be NULL.  RT_ERR_INVALID: what
 * rt_pixel_filter_check refuses. */
int rt_pixel_filter_table(const RtPixelFilter* filter, float* table, uint32_t* reach);
/* Makes the open accumulation track `filter` and clears the plane.  The rules of rt_accum_track_halves: after rt_accum_begin and before
 * the first add, else RT_ERR_STATE; a second call with the same filter is RT_OK and changes nothing, with another one RT_ERR_STATE.
 * RT_ERR_STATE on a sharded accumulation (shard_count > 1).  RT_ERR_INVALID: what rt_pixel_filter_check refuses.  Tracking ends with the
 * accumulation.  Combines freely with the other rt_accum_track_* calls and with adaptive adds. */
int rt_accum_track_filter(RtCtx* ctx, const RtPixelFilter* filter);
/* The read-out above: out_rgb_f32 [ny*nx*3] and out_rgb8 as rt_accum_denoise writes them, out_weight [ny*nx] = W in the row order of
 * out_rgb_f32; each may be NULL.  The accumulation is read and not changed.  Synchronises the context's stream once.  RT_ERR_STATE: no open
 * accumulation, or it does not track a filter. */
int rt_accum_read_filtered(RtCtx* ctx, float* out_rgb_f32, uint8_t* out_rgb8, float* out_weight);
/* GPU-free.  RT_OK, or RT_ERR_INVALID unless: `fs` non-NULL, both reserved words 0, the plane non-NULL, first_sample + done <= 2^32 - 1,
 * a filter rt_pixel_filter_check accepts.  Values are not judged. */
int rt_accum_filter_check(const RtAccumFilter* fs);
/* Fills the scalar fields and the filter of `fs` and writes the plane where its pointer is non-NULL.  Reads, and changes nothing.
 * Synchronises the context's stream once.  RT_ERR_STATE: no open accumulation, or it does not track a filter. */
int rt_accum_export_filter(RtCtx* ctx, RtAccumFilter* fs);
/* Puts `fs` into the open accumulation and turns tracking on under its filter.  Allowed while the accumulation has had no add (and no
 * merge) since rt_accum_begin — fresh with done 0, or after rt_accum_import — else RT_ERR_STATE; RT_ERR_STATE on a sharded accumulation.
 * Values are copied as bits.  RT_ERR_INVALID: rt_accum_filter_check fails, nx, rows, frame_id, first_sample or done differ from the
 * accumulation's, or the accumulation tracks a filter already and the snapshot's is another one.  A failed call leaves the accumulation
 * as it was.  Synchronises once. */
int rt_accum_import_filter(RtCtx* ctx, const RtAccumFilter* fs);

/* -- First-hit features: albedo, normal and depth of the primary hit, with their second moments -------------------------------------------
 * What a feature-guided denoiser (Rousselle, Manzi, Zwicker 2013) or a compositor asks a renderer for.  An accumulation that TRACKS
 * FEATURES also keeps one RtFeaturePixel per pixel, 64 B more.  Nothing is taken from the paths that are traced: the first hit of sample s
 * of pixel p is a function of the frame, the scene and (p, s), and a kernel of its own (csrc/rt_features.h) recomputes it — the primary ray
 * exactly as the render makes it (the pixel jitter, the thin lens of rt_set_lens), its time under rt_set_motion, the closest hit as the
 * context's search finds it (the tree, or every primitive under RT_FLAG_BRUTE_FORCE; quads and triangles of rt_set_quads included; a light
 * set changes nothing), and a constant medium's scatter decision at depth 0 with the draws the render uses.
 * Which samples.  Sample s, by its absolute index (first_sample + the samples before it), contributes iff s % stride == 0.  So the planes
 * after the samples [a, b) are the same bits however [a, b) is cut into adds and slices.  In an adaptive add a converged pixel takes none.
 * What sample s contributes, as (a, n, hit, z):
 *   miss                       a = (1, 1, 1), n = 0, no hit
 *   surface                    hit, z = t of the hit; n = the world-space, face-forwarded unit normal the shading uses (spheres, rectangles,
 *                              planar primitives, unwound through Translate / RotateY wrappers, chains of any length); a by material tag:
 *                              0, 1, 2, 5 .. 11 the material's first texture at the hit, at the (uv, p) the shading evaluates it at;
 *                              3 (Metal) the material's colour; 4 (Dielectric) and 12 (DisneyClearcoat) (1, 1, 1); any other tag 0;
 *                              then per channel a NaN becomes 0 and the value is clamped to [0, 1]
 *   medium scatter at depth 0  hit, z = t of the scatter; n = 0; a = the medium's Isotropic texture, NaN -> 0, clamped likewise
 * and what the record does with it, every operation one IEEE operation without contraction, in ascending order of s:
 *   albedo[c] += a[c], normal[c] += n[c] (f32);   n_f += 1;
 *   a2 += ((double)a[0] * (double)a[0] + (double)a[1] * (double)a[1]) + (double)a[2] * (double)a[2];   n2 likewise over n;
 *   hit:  n_h += 1;  z1 += (double)z;  z2 += (double)z * (double)z.
 * Read-out (rt_accum_read_features), per pixel, with N = (float)n_f:  albedo / N and normal / N per component (0 where n_f == 0);
 * depth = (float)(z1 / (double)n_h) (0 where n_h == 0);  hit = (float)n_h / N (0 where n_f == 0);  var = the variance of the MEAN of
 * albedo, normal and depth: for the vectors, with S = ((double)sum[0]^2 + (double)sum[1]^2) + (double)sum[2]^2 and n = (double)n_f,
 * q = (a2 - S / n) / (n - 1), clamped below at 0, then (float)(q / n); for the depth the same on (z2, z1 * z1, n_h).  0 where the count
 * is below 2.
 * Everything an accumulation returned before is unchanged in every bit with tracking on or off, and an accumulation that does not track
 * features launches no kernel it did not launch before.
 * State.  RtAccumFeatures carries the stride and the records in the row order of out_rgb_f32.  Resume is rt_accum_begin, rt_accum_import,
 * rt_accum_import_features: from then on the records are bit for bit those of the uninterrupted accumulation.
 * Not covered, refused with RT_ERR_UNSUPPORTED and a message: a sharded accumulation (shard_count > 1), hence rt_multi_accum_begin with
 * RT_MULTI_UNSUPPORTED_FEATURES (the joined context of an RtMulti refuses the call as it refuses every rt_accum_track_*: RT_ERR_STATE);
 * rt_accum_merge and rt_accum_import on an accumulation that tracks features.  The denoisers stay colour-guided.  DESIGN.md "First-hit
 * features". */
#define RT_FEATURES_MIN_STRIDE 1u
#define RT_FEATURES_MAX_STRIDE 64u
typedef struct RtFeatures {
    uint32_t stride;   /* RT_FEATURES_MIN_STRIDE .. RT_FEATURES_MAX_STRIDE: every stride-th sample, by absolute index */
    uint32_t reserved; /* 0 */
} RtFeatures;
typedef struct RtFeaturePixel {
    float albedo[3]; /* sum of a */
    uint32_t n_f;    /* feature samples taken */
    float normal[3]; /* sum of n */
    uint32_t n_h;    /* of which hit a surface or scattered in a medium */
    double a2, n2, z1, z2; /* sum |a|^2, sum |n|^2, sum z, sum z^2 */
} RtFeaturePixel;
typedef struct RtAccumFeatures {
    uint32_t nx, rows;           /* the frame: rows = ny (no shards) */
    uint32_t first_sample, done; /* those of the accumulation the records belong to */
    uint32_t reserved[2];        /* 0 */
    uint64_t frame_id;           /* rt_accum_frame_id of the frame */
    RtFeatures features;         /* the stride the records were summed under */
    RtFeaturePixel* plane;       /* [rows*nx] */
} RtAccumFeatures;
/* GPU-free, no context.  RT_OK, or RT_ERR_INVALID: `features` NULL, a stride outside its range, reserved not 0. */
int rt_features_check(const RtFeatures* features);
/* Makes the open accumulation track features and clears the records.  The rules of rt_accum_track_filter: after rt_accum_begin and before
 * the first add, else RT_ERR_STATE; a second call with the same stride is RT_OK and changes nothing, with another one RT_ERR_STATE;
 * RT_ERR_STATE on the joined context of an RtMulti.  RT_ERR_UNSUPPORTED on a sharded accumulation.  RT_ERR_INVALID: what rt_features_check
 * refuses.  Tracking ends with the accumulation.  Combines freely with the other rt_accum_track_* calls and with adaptive adds. */
int rt_accum_track_features(RtCtx* ctx, const RtFeatures* features);
/* The read-out above, in image order as rt_accum_read lays its outputs out: out_albedo [ny*nx*3], out_normal [ny*nx*3], out_depth [ny*nx],
 * out_hit [ny*nx], out_var [ny*nx*3] (albedo, normal, depth); each may be NULL.  The accumulation is read and not changed.  Synchronises the
 * context's stream once.  RT_ERR_STATE: no open accumulation, or it does not track features. */
int rt_accum_read_features(RtCtx* ctx, float* out_albedo, float* out_normal, float* out_depth, float* out_hit, float* out_var);
/* GPU-free.  RT_OK, or RT_ERR_INVALID unless: `fs` non-NULL, both reserved words 0, the plane non-NULL, first_sample + done <= 2^32 - 1,
 * features that rt_features_check accepts.  Values are not judged. */
int rt_accum_features_check(const RtAccumFeatures* fs);
/* Fills the scalar fields and the stride of `fs` and writes the records where its pointer is non-NULL.  Reads, and changes nothing.
 * Synchronises the context's stream once.  RT_ERR_STATE: no open accumulation, or it does not track features. */
int rt_accum_export_features(RtCtx* ctx, RtAccumFeatures* fs);
/* Puts `fs` into the open accumulation and turns tracking on under its stride.  Allowed while the accumulation has had no add (and no
 * merge) since rt_accum_begin — fresh with done 0, or after rt_accum_import — else RT_ERR_STATE; RT_ERR_UNSUPPORTED on a sharded
 * accumulation.  Values are copied as bits.  RT_ERR_INVALID: rt_accum_features_check fails, nx, rows, frame_id, first_sample or done differ
 * from the accumulation's, or the accumulation tracks features already and the snapshot's stride is another one.  A failed call leaves the
 * accumulation as it was.  Synchronises once. */
int rt_accum_import_features(RtCtx* ctx, const RtAccumFeatures* fs);

/* -- The feature-guided filter: rt_accum_denoise with the first-hit features beside the colour guide (Rousselle, Manzi, Zwicker 2013) -------
 * Inputs per pixel, in image order: c, y, v as in "Denoising"; from the pixel's RtFeaturePixel the means abar = albedo / (float)n_f and
 * nbar = normal / (float)n_f per component, zbar = (float)(z1 / (double)n_h) (0 where n_h == 0), and the variances of the mean va, vn, vz
 * exactly as rt_accum_read_features returns them (vz 0 where n_h < 2).  A pixel with n_f < 2 has NaN for all ten: it stays what it is and
 * spreads to no other pixel.
 * Demodulation (demodulate != 0), before anything else, per pixel: a'[ch] = abar[ch] > 1/64 ? abar[ch] : 1/64;
 * Ya = (0.2126f a'[0] + 0.7152f a'[1]) + 0.0722f a'[2];  c[ch] = c[ch] / a'[ch];  y = y / Ya;  v = v / (Ya * Ya).
 * Per pair (p, q), q in the window of radius R inside the image, in the order of "Denoising":
 *   D_c = the patch distance of "Denoising" on (y, v): the same operands in the same order.
 *   for each feature f in `use` (= use_mask), in the order albedo, normal, depth, with f_p, f_q the means and vf_p, vf_q the variances:
 *     s2 = (dx dx + dy dy) + dz dz over the components of f_p - f_q (depth: dz dz alone);  vmin = vf_q < vf_p ? vf_q : vf_p;
 *     floor = tau_albedo, tau_normal, or tau_depth * (zbar_p * zbar_p);  vs = vf_p + vf_q;  vmax = vs > floor ? vs : floor;
 *     d_f = (s2 - (vf_p + vmin)) / (1e-10f + (k_f * k_f) * vmax)
 *   m = D_c < 0 ? 0 : D_c;  then for each used f in that order: m = d_f > m ? d_f : m.   (The min-of-weights rule of the 2013 paper: the
 *   weight falls monotonically in m, so one weight is evaluated.)
 *   u = 1 - 0.25f m;  u = u > 0 ? u : 0;  where D_c or a used d_f is NaN: u = 0.   Then w, den and num as in "Denoising".
 * Output per channel: den != 0 ? num / den : c (the possibly demodulated c of p), times a'[ch] of p where demodulate != 0.
 * With use == 0 and demodulate == 0 the output is rt_accum_denoise's, bit for bit.  out_rgb8 goes where rt_accum_denoise's goes.
 * Defaults (RT_FEATURE_GUIDE_DEFAULT_*): k 0.6 for each feature and tau 1e-3, the paper's values; no error figure of this filter on this
 * renderer's frames exists yet (DESIGN.md "First-hit features").  The half, select, multi-scale and robust filters stay colour-guided. */
#define RT_FEATURE_USE_ALBEDO 1u
#define RT_FEATURE_USE_NORMAL 2u
#define RT_FEATURE_USE_DEPTH  4u
#define RT_FEATURE_GUIDE_DEFAULT_K 0.6f
#define RT_FEATURE_GUIDE_DEFAULT_TAU 1e-3f
typedef struct RtFeatureGuide {
    float k_albedo, k_normal, k_depth;       /* strengths: finite, > 0 */
    float tau_albedo, tau_normal, tau_depth; /* variance floors: finite, >= 0; tau_depth is relative to zbar_p^2 */
    uint32_t use_mask;                       /* `use`: RT_FEATURE_USE_* (the field is not named `use`, a keyword of Rust) */
    uint32_t demodulate;                     /* 0, or anything else: filter c / albedo and multiply the albedo back */
    uint32_t reserved[2];                    /* 0 */
} RtFeatureGuide;
/* GPU-free, no context.  RT_OK, or RT_ERR_INVALID: `guide` NULL, a strength not finite or <= 0, a floor not finite or < 0, a bit of `use`
 * above RT_FEATURE_USE_DEPTH, a reserved word not 0. */
int rt_feature_guide_check(const RtFeatureGuide* guide);
/* The filter above over the open accumulation; `dn` as for rt_accum_denoise (NULL: its defaults), `guide` must not be NULL.  Outputs as
 * rt_accum_denoise's.  The accumulation is read and not changed.  Synchronises the context's stream once.  RT_ERR_STATE: no accumulation
 * is open, it does not track features, fewer than 2 samples are done, or fewer than 2 feature samples were taken (the samples done hold
 * fewer than 2 multiples of the stride).  RT_ERR_UNSUPPORTED: a shard.  RT_ERR_INVALID: what rt_feature_guide_check or rt_accum_denoise
 * refuses of its parameters. */
int rt_accum_denoise_features(RtCtx* ctx, const RtDenoise* dn, const RtFeatureGuide* guide, float* out_rgb_f32, uint8_t* out_rgb8);

/* -- multi-GPU: one process, the GPUs of one node, the framebuffer gather inside the library ---------------------
 * SURVEY.md 8(b)/(e).  The reference's only parallelism is the per-column fan-out over a thread pool with the
 * world shared read-only (main.rs:72-108); here the scene is replicated on every device, device r renders the image
 * rows of the row-interleaved bands (j / band) % n == r (RNG keyed by pixel and sample: the frame does not depend on
 * n), ONE gather over RCCL/xGMI — a group of ncclSend / ncclRecv to the first device — brings the equal-sized band buffers
 * together and the first device restores row order.  librccl is opened at rt_multi_create (dlopen); the single-GPU entry points do not depend on it. */
typedef struct RtMulti RtMulti;
/* One RtCtx per listed HIP device + ncclCommInitAll over them.  Replaces main.rs:72-73 for a node.
 * N > 1 over RCCL is UNVERIFIED ON HARDWARE until an 8-GPU run of `bench.py --in-library` has been recorded (no box with
 * more than one GPU has been available to the build); everything around the collective — one host thread per context,
 * padded band buffers, the de-interleave, the statistics — runs for n = 2, 3 on one GPU through rt_multi_create_ex. */
int rt_multi_create(const int* device_ids, int n_devices, RtMulti** out);
/* Same with flags.  RT_MULTI_COPY_GATHER: the RCCL gather is replaced by device-to-device copies into the same gathered
 * layout and librccl is not opened at all; a device id may then be listed several times (several contexts rendering
 * side by side on one GPU).  The test hook that reaches rt_multi_render's n > 1 code on a one-GPU box; frames are
 * bit-identical to rt_render either way. */
#define RT_MULTI_COPY_GATHER 1u
int rt_multi_create_ex(const int* device_ids, int n_devices, uint32_t flags, RtMulti** out);
void rt_multi_destroy(RtMulti* m);
int rt_multi_device_count(const RtMulti* m);
/* Last error text of `m` (or of the calling thread's last failed rt_multi_create if NULL). */
const char* rt_multi_last_error(const RtMulti* m);
/* rt_scene_upload on every device. */
int rt_multi_scene_upload(RtMulti* m, const RtFlatScene* scene);
/* Renders the WHOLE frame of `params` (nx x ny, spp; shard_count / shard_id are ignored, shard_band = rows per band,
 * 0 = 8) split over the devices and gathers it: out_rgb_f32 [ny*nx*3] row 0 = bottom, out_rgb8 [ny*nx*3] flipped,
 * either may be NULL.  `stats` sums the counters of the devices and takes the maximum of their times. */
int rt_multi_render(RtMulti* m, const RtCamera* cam, const RtParams* params, float* out_rgb_f32, uint8_t* out_rgb8,
                    RtStats* stats);

/* -- progressive accumulation across devices ------------------------------------------------------------------------
 * The accumulation line ("Progressive accumulation" .. "Multi-scale denoising") on the devices of an RtMulti.  Device i holds an ordinary
 * accumulation over shard (band, n, i) of the frame; an add is the same rt_accum_add / rt_accum_add_adaptive on every device, one host
 * thread each, so the shards stay in lock-step with one `done` for all.  The adaptive decision is per pixel, so — unlike the sample
 * windows of rt_accum_merge — row-interleaved shards combine with adaptive sampling.  A shard's rows are not neighbours in the image, so
 * no filter runs on one and its frame figures are not the frame's: rt_multi_accum_join is the spatial join.  It brings every plane of
 * every shard to the first device, device to device (the two gather mechanisms of rt_multi_render; no host staging), and installs them in
 * a whole-frame accumulation there, on which every reading call of this header runs unchanged.
 *
 * The joined context.  rt_multi_accum_join hands out an RtCtx that the RtMulti owns: created by the first rt_multi_accum_begin (users of
 * rt_multi_render pay nothing), the same pointer for the life of `m`, destroyed by rt_multi_destroy — never by the caller.  It holds the
 * accumulation of the frame with shard_count 1, the same camera, first_sample and done, adaptive / channels / halves / buckets as the
 * shards have them, in the local pixel order that one context with this scene and default options picks, so that every read-out is what
 * ONE context returns after the same adds, bit for bit: rt_accum_read, _read_counts, _read_channel_sem, _denoise, _denoise_channels,
 * _denoise_halves, _denoise_robust, _denoise_multiscale, _read_halves, _read_robust, _export, _export_halves, _export_buckets.  It is a
 * MIRROR: rt_accum_begin, _add, _add_adaptive, _import, _import_halves, _import_buckets, _merge, _track_channels, _track_halves,
 * _track_buckets and _end on it are RT_ERR_STATE and change nothing (so are rt_render_to_noise and rt_render_adaptive, which begin an
 * accumulation).  It has no scene and no work buffers.  A join may follow every add; each rewrites every pixel, since every pixel
 * belongs to exactly one shard.  Between rt_multi_accum_begin (or _end) and the next join it holds no accumulation: reading calls are
 * RT_ERR_STATE.
 *
 * Errors.  Arguments are checked before any device is touched where this header says so; otherwise an invalid argument or a call out of
 * order is refused by every device alike, the code and text are the first device's and nothing has changed.  A device-side failure
 * (RT_ERR_NOMEM, RT_ERR_DEVICE) on any device ENDS the accumulation on all of them — the shards no longer belong together —, every later
 * call but rt_multi_accum_begin and rt_multi_accum_end is RT_ERR_STATE, and rt_multi_last_error names the device.  rt_multi_render may
 * run between two adds; rt_multi_scene_upload and rt_multi_set_* end the accumulation as their single-context forms do.
 * RCCL: as rt_multi_create says, every step over RCCL with n > 1 — here the one group of byte-counted ncclSend / ncclRecv of the join —
 * is UNVERIFIED ON HARDWARE; RT_MULTI_COPY_GATHER runs everything else for n = 2, 3 on one GPU.
 * Not covered: a sample-window split inside rt_multi_*; driver loops (the caller loops add / join / read); rt_debug_set_option on the
 * contexts of an RtMulti; denoising without a join (a halo exchange between shards).  DESIGN.md "Accumulation across devices". */
#define RT_MULTI_TRACK_CHANNELS 1u /* rt_accum_track_channels on every shard */
#define RT_MULTI_TRACK_HALVES   2u /* rt_accum_track_halves */
#define RT_MULTI_TRACK_BUCKETS  4u /* rt_accum_track_buckets(M) */
/* No track flag: the bit that would ask for rt_accum_track_features on every shard, which is not covered.  rt_multi_accum_begin knows it
 * in order to answer RT_ERR_UNSUPPORTED with a message, and begins nothing. */
#define RT_MULTI_UNSUPPORTED_FEATURES 32u
/* rt_accum_begin on every device: device i on shard (band, n, i) of the frame of `params` — band = shard_band, 0 = 8; shard_count and
 * shard_id are ignored, as in rt_multi_render —, then the tracking that `track` names.  RT_ERR_INVALID before any device is touched: cam or
 * params NULL, a bit in `track` that is no RT_MULTI_TRACK_*, M outside 3 .. RT_BUCKETS_MAX with RT_MULTI_TRACK_BUCKETS (M is not looked
 * at without it).  RT_ERR_UNSUPPORTED, likewise before any device is touched: RT_MULTI_UNSUPPORTED_FEATURES.  Everything else as rt_accum_begin refuses it.  A failure leaves no accumulation open anywhere.  An open one is replaced. */
int rt_multi_accum_begin(RtMulti* m, const RtCamera* cam, const RtParams* params, uint32_t first_sample, uint32_t track, uint32_t M);
/* rt_accum_add / rt_accum_add_adaptive on every device.  `stats` (may be NULL) sums the devices' as rt_multi_render does.  Complete on return. */
int rt_multi_accum_add(RtMulti* m, uint32_t n_samples, RtStats* stats);
int rt_multi_accum_add_adaptive(RtMulti* m, uint32_t n_samples, const RtAdaptive* ad, RtStats* stats);
/* Joins the shards into the joined context (above) and stores it in *joined (also on failure, once it exists).  Complete on return.
 * RT_ERR_STATE: no accumulation begun, or a context of `m` was ended or changed behind its back. */
int rt_multi_accum_join(RtMulti* m, RtCtx** joined);
/* The resume of a multi-device render: a WHOLE-FRAME snapshot — what the joined context, or one context over the frame, exported — is
 * split on the host by rows into the n shard snapshots (frame_id of each: rt_accum_frame_id with that shard's params) and each is imported
 * on its device with rt_accum_import [, _import_halves][, _import_buckets].  `st` required; `hs`, `bs` may be NULL.  Right after
 * rt_multi_accum_begin, under the rules of those three calls (so: begun without halves and buckets tracking, which the import turns on).
 * RT_ERR_INVALID before any device is touched: a snapshot that its _check refuses, or whose nx, rows (= ny), frame_id (of the frame with
 * shard_count 1) or first_sample are not the frame's, or halves / buckets whose first_sample and done are not the state's.  A snapshot
 * written on n devices resumes on any other number, and on one context through rt_accum_import. */
int rt_multi_accum_import(RtMulti* m, const RtAccumState* st, const RtAccumHalves* hs, const RtAccumBuckets* bs);
/* rt_accum_end on every device; the joined context holds no accumulation afterwards.  RT_OK also where none is open. */
int rt_multi_accum_end(RtMulti* m);

/* rt_set_lens on every device (all or none: the values are checked by the first). */
int rt_multi_set_lens(RtMulti* m, const RtLens* lens);
/* rt_set_motion on every device.  An invalid motion is refused by the first device and none has changed; a device-side failure
 * (RT_ERR_NOMEM, RT_ERR_DEVICE) on a later device leaves every device with NO motion (the static renderer), not the previous one. */
int rt_multi_set_motion(RtMulti* m, const RtMotion* motion);
/* rt_set_quads on every device, all or none as rt_multi_set_motion: a refusal comes from the first device and none has changed; a
 * device-side failure on a later device leaves every device WITHOUT planar primitives. */
int rt_multi_set_quads(RtMulti* m, const RtQuads* quads);
/* rt_set_lights on every device, all or none as rt_multi_set_quads: a refusal comes from the first device and none has changed; a
 * device-side failure on a later device leaves every device WITHOUT a light set. */
int rt_multi_set_lights(RtMulti* m, const RtLights* lights);
/* The de-interleave step on its own: `d_gathered` is a DEVICE buffer of n_shards band buffers, each
 * max_r rt_shard_rows(ny, band, n_shards, r) rows of nx*3 floats (what the gather delivers); writes the frame in
 * image row order to d_out_rgb_f32 [ny*nx*3] and / or the quantised, flipped image to d_out_rgb8 (device pointers,
 * either may be NULL).  `stream` as in rt_render_device. */
int rt_deinterleave_bands(RtCtx* ctx, const void* d_gathered, uint32_t nx, uint32_t ny, uint32_t band, uint32_t n_shards,
                          void* d_out_rgb_f32, void* d_out_rgb8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_MI355X_H */
