/*
 * rtow_mi355x_debug.h — test hooks and diagnostics of librtow_mi355x.so.
 *
 * Nothing here is part of the drop-in boundary: a host that replaces main.rs:62-129 binds include/rtow_mi355x.h alone
 * (lifecycle, scene upload, render, multi-GPU, progress).  The entry points below live in the same library so that the
 * parity tests can drive single bounces, hold equivalent search structures against each other and read what upload built;
 * the benchmark reads per-depth and first-frame timings through them.  Same conventions as rtow_mi355x.h.
 */
#ifndef RTOW_MI355X_DEBUG_H
#define RTOW_MI355X_DEBUG_H

#include "rtow_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- diagnostic RtParams.flags ------------------------------------------------------------------------------------- */
/* Record HIP events around the kernels of every depth of the FIRST slice; read them back with
 * rt_get_depth_timings().  Diagnostic only (adds two event records per depth). */
#define RT_FLAG_TIME_DEPTHS 4u
/* rt_debug_bounce only: run the rays through the ray queue and the SAME kernels rt_render launches for a depth >= 1
 * (the scene's closest-hit kernel with persistent lanes, then the class-sorting shading kernel with its wave64
 * compaction) instead of the unsorted single-kernel test path.  The per-path RNG key is then the one the renderer
 * derives from the slot: ray i gets path_key(seed 0, pixel i, sample 0) and in_key is ignored; out_attenuation,
 * out_o and out_d are filled for surviving rays only (a finished path keeps no ray), out_radiance for finished ones. */
#define RT_FLAG_PRODUCTION_KERNELS 8u

/* Per-depth device times of the first slice of the last render that had RT_FLAG_TIME_DEPTHS set:
 * isect_ms[d] = closest-hit kernel, shade_ms[d] = shading kernel, rays[d] = rays traced at depth d
 * in that slice.
 * Returns the number of depths written (<= max_n), or a negative RT_ERR_*. */
int rt_get_depth_timings(RtCtx* ctx, uint32_t max_n, float* isect_ms, float* shade_ms, uint64_t* rays);

/* Host-side timeline of the last rt_render / rt_render_device of `ctx`: a JSON object {"label": milliseconds, ...} in call order
 * (work-buffer allocations one by one, the hardware-queue probe = the first kernel launch of a process, the candidate lists with
 * the one in-frame synchronisation, enqueueing every launch, waiting for the device).  The first frame of a process is what the
 * reference's own timer covers (main.rs:62-129, utils.rs:15-18); bench.py reports its parts from here.  Writes at most cap bytes
 * (NUL-terminated) and returns the size needed, or a negative RT_ERR_*. */
int rt_debug_render_parts(const RtCtx* ctx, char* buf, uint32_t cap);

/* -- debug / tuning options (test hooks) ---------------------------------------------------------------------------
 * Per context (not per process: the library reads no environment variable); every setting renders the same image — the
 * options select between equivalent search structures, placements and orders so that tests can hold them against each
 * other, and so that measurements can vary one thing.  Same BITS with one stated exception: the closest-hit searches
 * (list walk, tree, grid, candidate lists) agree on every ray except those for which fp32 Sphere::hit (hitable.rs:75-91)
 * reports a root although the ray misses the sphere in exact arithmetic (cancellation at grazing incidence), and those for which
 * fp32 reports a hit on a primitive below Translate / RotateY wrappers although the ray misses it under the exact ray map of its
 * chain (hitable.rs:404-520 with the stored f32 offsets and sin / cos; the fp32 map rounds at the magnitude of every intermediate
 * coordinate); a box or cell test may cull such a false positive, the list walk cannot.  Every culling bound holds the exact
 * world region of its primitive widened by the rounding of that f32 map for rays that start among the primitives of the chain
 * (rt_debug_world_bounds, error model in csrc/rt_api.hip).  A ray from farther out below a deep chain (1 per Translate plus 12 per
 * RotateY summing to more than about 60) may meet two primitives at exact roots closer than the map can tell apart; which of the
 * two a search reports is then a matter of rounding.  Measured: at most 8 of the 1.35e9 rays of config 2, each
 * proven a false positive in float64 by the tests.  Which of them the reference's own binary BvhNode would cull is unpinned.  0 is the library's own choice for every option.  Options marked
 * (upload) take effect at the next rt_scene_upload, the others at the next render. */
enum RtDebugOption {
    RT_OPT_TREE_PLACEMENT = 0,        /* (upload) 1: the BVH is read through L2 even when it would fit LDS */
    RT_OPT_PRIMARY_LISTS = 1,         /* 1: no per-pixel candidate lists, depth 0 walks the tree */
    RT_OPT_PIXEL_ORDER = 2,           /* 1: path slots enumerate pixels row by row, 2: in 8 x 8 tiles wherever the frame allows */
    RT_OPT_TEXEL_POOL = 3,            /* (upload) 1: float4 texel pool even when every texel is k/255 */
    RT_OPT_GRID = 4,                  /* 1: no uniform grid, sphere-only scenes walk the tree at every depth */
    RT_OPT_GRID_CELL = 5,             /* (upload) grid cell edge in 1/1000 of the median sphere diameter */
    RT_OPT_CHAINS = 6,                /* 1: one chain of launches per slice, 2: two shard groups on two streams */
    RT_OPT_GENERAL_KERNELS = 7,       /* (upload) 1: the general-scene kernel instantiations on a sphere-only scene */
    RT_OPT_GENERAL_LDS = 8,           /* (upload) 1: wrapper / medium tables stay in HBM */
    RT_OPT_QUEUE_SHARDS = 9,          /* n: queue shards (default 8 per CU) */
    RT_OPT_ISECT_WORKGROUPS = 10,     /* n: closest-hit workgroups per launch */
    RT_OPT_MATERIALISE_PRIMARIES = 11,/* 1: primary rays are written to the queue by their own kernel instead of regenerated */
    RT_OPT_MEDIUM_SEARCH = 12,        /* (upload) 1: ConstantMedium::hit evaluates its boundary twice, as the reference does, also where one
                                       * evaluation answers both searches (a box, a sphere) */
    RT_OPT_POOL_CHUNK_DELAY_US = 13,  /* n: the helper thread that backs the work-buffer pool (csrc/rt_pool.h) takes n microseconds longer per
                                       * 128 MB chunk — a device that hands out memory slowly, for the test of frames that start in what
                                       * has arrived so far */
    RT_OPT__COUNT = 14
};
int rt_debug_set_option(RtCtx* ctx, uint32_t option, uint32_t value);
int rt_debug_get_option(const RtCtx* ctx, uint32_t option, uint32_t* value);

/* What rt_scene_upload built for the closest-hit search of the uploaded scene. */
typedef struct RtSceneInfo {
    uint32_t n_entries;            /* world entries: primitives that are not a medium boundary + media */
    uint32_t n_tree_nodes, tree_depth;
    uint32_t tree_in_lds;          /* 1: the BVH4 is staged in LDS, 0: read through L2 */
    uint32_t general_kernels;      /* 1: rectangles / wrappers / media (or forced) */
    uint32_t closest_hit_lds_bytes;
    uint32_t grid;                 /* 1: depth >= 1 walks a uniform grid (sphere-only scenes, csrc/rt_grid.h) */
    uint32_t grid_cells[3];
    uint32_t grid_refs;            /* sphere references in the cell lists */
    uint32_t grid_always;          /* large spheres tested for every ray */
    uint32_t grid_lds_bytes;
    float grid_cell_size[3];
    uint32_t general_tables_in_lds; /* 1: the wrapper / medium tables of a general scene are staged in LDS beside the tree or its stacks */
    uint32_t nest;                  /* 1: the scene nests beyond what the kernels keep in registers (a wrapper chain of more than 4, more
                                     * than 32 media, a wrapper around a medium): the instantiations with the loops run (csrc/rt_device.h) */
} RtSceneInfo;
int rt_debug_scene_info(const RtCtx* ctx, RtSceneInfo* info);

/* The planar primitives of `ctx` (rt_set_quads): how many there are and where the kernels read their plane data — 0: through L2 (the
 * only placement so far, DESIGN.md "Planar primitives"), 1: staged in LDS.  Either pointer may be NULL. */
int rt_debug_planar_info(const RtCtx* ctx, uint32_t* n_planar, uint32_t* plane_data_in_lds);
/* The culling bounds rt_set_quads gives the primitives of `quads` (host code only: no context, no GPU; the same function rt_set_quads
 * calls), for tests of their derivation.  `world_mag` = the largest coordinate magnitude of the scene's bounds the set is attached to
 * (0: the set alone); the set's own corners are added to it.  box[6 n] = the box of the corners grown by slack[i] (min xyz, max xyz),
 * before the tree's own pad; slack[n] as rtow_mi355x.h states it.  RT_ERR_INVALID where rt_set_quads would refuse the geometry. */
int rt_debug_planar_bounds(const RtQuads* quads, float world_mag, float* box, float* slack);

/* The uniform grid rt_scene_upload would build over the spheres of `scene` (host code only: no context, no GPU), for tests of
 * its construction.  cell_per_mille as RT_OPT_GRID_CELL (0 = default), lds_budget in bytes (0 = 80 KiB, two workgroups per CU).
 * Returns RT_ERR_UNSUPPORTED when the scene gets no grid, RT_ERR_INVALID when a buffer is too small (the needed sizes are
 * then in *n_cells / *n_refs), else RT_OK with: grid[0..2] = min corner, grid[3..5] = cell edges, grid[6] = pad, grid[7] =
 * origin-coordinate limit; dims[0..2] = cells per axis; cells[c] = offset << 12 | count (x fastest); refs = sphere ids of the
 * cell lists; large[0..*n_large) = the spheres tested for every ray. */
int rt_debug_grid_build(const RtFlatScene* scene, uint32_t cell_per_mille, uint32_t lds_budget, float grid[8], uint32_t dims[3],
                        uint32_t* cells, uint32_t* n_cells, uint16_t* refs, uint32_t* n_refs, uint32_t large[4], uint32_t* n_large);

/* The world-space bounds rt_scene_upload culls with (host code only: no context, no GPU; the same function upload calls), for tests
 * of the bounds of primitives below Translate / RotateY wrappers.  Arrays are caller-owned, any of them may be NULL; n_prims =
 * n_spheres + n_rects (spheres first):
 *   prim_box[6 * n_prims]         world box of every primitive after its wrapper chain, before the tree's pad (min xyz, max xyz);
 *   prim_box_padded[6 * n_prims]  the box the tree builder stores for it;
 *   world_sphere[4 * n_spheres]   centre and radius of every sphere in world space (a bare sphere: its own);
 *   *n_entries                    in: capacity of the entry arrays, out: the number of world entries (primitives that are not a
 *                                 medium boundary, then the media);
 *   entry_id[*n_entries]          primitive i, or n_prims + medium m;
 *   entry_box_padded[6 * ...]     the box the tree stores for the entry (a medium: around all of its boundary primitives);
 *   entry_bs[4 * ...]             the bounding sphere k_primary_lists tests for it.
 * Returns RT_ERR_INVALID for a scene rt_scene_upload would refuse for its geometry, wrappers or medium tags (a medium without
 * boundary primitives included), or when *n_entries is too small (the
 * needed count is then in *n_entries), else RT_OK. */
int rt_debug_world_bounds(const RtFlatScene* scene, float* prim_box, float* prim_box_padded, float* world_sphere, uint32_t* n_entries,
                          uint32_t* entry_id, float* entry_box_padded, float* entry_bs);

/* The bounds rt_set_motion built for the uploaded scene with its motion (RT_ERR_STATE when none is set), for tests of their
 * conservativeness.  Arrays are caller-owned:
 *   entry_box_padded[6 * n]  the box the tree stores for every world entry (a moving sphere: around the region it sweeps);
 *   entry_sphere[4 * n]      the bounding sphere k_primary_lists tests for it;
 *   entry_id[n]              primitive i, or n_prims + medium m;          entry_cap = capacity of these three, *n_entries = n;
 *   grid[0..2] = min corner, grid[3..5] = cell edges, dims = cells per axis (all 0: the scene with its motion has no grid);
 *   cell_begin[n_moving + 1], cell_id[*n_cell_ids]: the cells (x fastest) that list moving sphere k are cell_id[cell_begin[k] ..
 *   cell_begin[k + 1]); a single entry 0xFFFFFFFF: the sphere is "large" and tested for every ray.  cell_cap = capacity of cell_id.
 * Returns RT_ERR_INVALID when a buffer is missing or too small (the needed counts are then in *n_entries / *n_cell_ids). */
int rt_debug_motion_bounds(const RtCtx* ctx, float* entry_box_padded, float* entry_sphere, uint32_t* entry_id, uint32_t entry_cap, uint32_t* n_entries,
                           float grid[6], uint32_t dims[3], uint32_t* cell_begin, uint32_t* cell_id, uint32_t cell_cap, uint32_t* n_cell_ids);

/* -- the launch ledger (test hooks, host code only) -----------------------------------------------------------------
 * k_shade, k_intersect and k_debug_bounce are families of instantiations over feature flags; a key is the set of its flags, one bit
 * each (csrc/rt_api.hip "kernel variants").  A ledger holds one bit per key: bit (k & 31) of word k >> 5 for the 256 keys of k_shade
 * and of k_intersect, bit k of debug_bounce[form] for the 8 keys of each search form of k_debug_bounce, and one bit per closest-hit
 * kernel that launch_intersect selects outside the tables (RT_UNTABLED_*).  tests/test_variant_matrix.py holds what a context has
 * launched against what its rows claim, and tests/test_variant_matrix_host.py the union of the claims against the tables. */
#define RT_LEDGER_WORDS 8
#define RT_FAMILY_SHADE 0u
#define RT_FAMILY_INTERSECT 1u
#define RT_FAMILY_DEBUG_BOUNCE 2u
#define RT_FAMILY_UNTABLED 3u
#define RT_FAMILY_DEBUG_FORMS 4u /* rt_debug_variant_flag_names only: the names of the RT_DEBUG_FORM_* in index order */
#define RT_DEBUG_FORM_TREE_L2 0
#define RT_DEBUG_FORM_TREE_LDS 1
#define RT_DEBUG_FORM_BRUTE 2
#define RT_UNTABLED_GRID_FLAT 1u         /* k_intersect_grid<true>: a grid one cell high */
#define RT_UNTABLED_GRID 2u              /* k_intersect_grid<false> */
#define RT_UNTABLED_GRID_MOTION_FLAT 4u  /* k_intersect_grid_motion<true> */
#define RT_UNTABLED_GRID_MOTION 8u       /* k_intersect_grid_motion<false> */
#define RT_UNTABLED_LIST 16u             /* k_intersect_list */
#define RT_UNTABLED_LIST_MOTION 32u      /* k_intersect_list_motion */
#define RT_UNTABLED_LIST_PLANAR 64u      /* k_intersect_list_planar */
typedef struct RtVariantLedger {
    uint32_t shade[8];
    uint32_t intersect[8];
    uint32_t debug_bounce[3];
    uint32_t untabled;
} RtVariantLedger;
/* The keys that have a kernel, read from the tables the launch functions index (no context, no GPU). */
int rt_debug_variant_tables(RtVariantLedger* exists);
/* The names of a family's flags in bit order, separated by blanks (RT_FAMILY_UNTABLED: the kernels of the RT_UNTABLED_* bits, RT_FAMILY_DEBUG_FORMS:
 * the search forms that index RtVariantLedger.debug_bounce).  Writes at
 * most cap bytes (NUL-terminated) and returns the size needed, or a negative RT_ERR_*. */
int rt_debug_variant_flag_names(uint32_t family, char* buf, uint32_t cap);
/* The keys `ctx` has launched since the last reset (launch_shade, launch_intersect, the table lookup of rt_debug_bounce); reset != 0
 * clears them after reading.  `launched` may be NULL. */
int rt_debug_launched_variants(RtCtx* ctx, RtVariantLedger* launched, int reset);

#ifdef RT_PROFILE_LANES
/* Diagnostic builds only (-DRT_PROFILE_LANES; absent from the product library): the lane-occupancy counters of
 * csrc/rt_kernels.h, optionally reset after reading. */
int rt_debug_lane_stats(unsigned long long* out24, int reset);
#endif

/* -- single-bounce evaluation (test hook) --------------------------------------------------
 * Runs ONE closest-hit + shade step (main.rs:44-58 for one depth) over `n` caller-given
 * rays on the GPU without queue compaction and returns the per-ray outcome, so that each
 * material / texture / sky branch can be compared with the CPU oracle function by
 * function.  Arrays are host pointers, n entries each (vec3 as 3 floats).
 */
typedef struct RtBounceIO {
    uint32_t n;
    uint32_t depth;            /* RNG counter block = depth (see DESIGN.md "RNG") */
    const float* in_o;         /* [3n] */
    const float* in_d;         /* [3n] */
    const uint32_t* in_key;    /* [2n] per-path RNG key (k0,k1) */
    int32_t* out_hit;          /* [n] primitive index (sphere i, or n_spheres + rect i) or -1 */
    float* out_t;              /* [n] */
    float* out_radiance;       /* [3n] emitted or sky term of this segment (untinted) */
    float* out_attenuation;    /* [3n] */
    float* out_o;              /* [3n] scattered ray */
    float* out_d;              /* [3n] */
    uint8_t* out_alive;        /* [n] 1 = scatter returned true */
    uint32_t flags;            /* RT_FLAG_* (RT_FLAG_BRUTE_FORCE selects the list walk) */
} RtBounceIO;
int rt_debug_bounce(RtCtx* ctx, const RtBounceIO* io);

/* Test hook for the arithmetic routines of the kernels that are not the compiler's operators (csrc/rt_device.h; host arrays
 * of n floats):
 *   RT_ARITH_SHARED_DIVISION  out[i] = x[i] / a[i] as the kernels compute the roots of a ray (divisor |d|^2, hitable.rs:85-89) and
 *       the normal of a sphere (divisor r, hitable.rs:95): the compiler's own fp32 division sequence with the refined reciprocal
 *       of the divisor shared between the quotients and without the operand scaling that only extreme exponents need;
 *   RT_ARITH_SQRT             out[i] = sqrt(x[i]) as the kernels take it of a discriminant and of a squared length: the compiler's
 *       own sequence without the scaling of arguments below 2^-96 (`a` is not read);
 *   RT_ARITH_TO_I32, _TO_U32  out[i] = the BITS of `x[i] as i32` / `x[i] as u32` with Rust's rule (toward zero, saturating, NaN -> 0;
 *       math.rs:137-152 offset_hit_point, texture.rs:183-193): v_cvt_i32_f32 / v_cvt_u32_f32 (`a` is not read);
 *   RT_ARITH_ACOS, _ATAN2, _SIN, _COS, _LOG  out[i] = acosf(x[i]), atan2f(x[i], a[i]) (`x` is y, `a` is x), sinf(x[i]), cosf(x[i]),
 *       logf(x[i]): the very calls of Sphere::get_uv (hitable.rs:65-71), CheckerTex / PerlinTex (texture.rs:40-49, 164-168),
 *       world_to_local_with_rot (hitable.rs:37-41) and gtr1 (pbr.rs:72-79) in the kernels (`a` is read by _ATAN2 only).
 * The test holds the first two against IEEE bit for bit over the operand range the kernels use them on and maps where they may
 * differ, the conversions against the Rust rule over every kind of argument, and the math library's functions against float64 to
 * the single-precision ulp bounds of the OpenCL full profile (acos 4, atan2 6, sin and cos 4, log 3). */
#define RT_ARITH_SHARED_DIVISION 0u
#define RT_ARITH_SQRT 1u
#define RT_ARITH_TO_I32 2u
#define RT_ARITH_TO_U32 3u
#define RT_ARITH_ACOS 4u
#define RT_ARITH_ATAN2 5u
#define RT_ARITH_SIN 6u
#define RT_ARITH_COS 7u
#define RT_ARITH_LOG 8u
int rt_debug_arithmetic(RtCtx* ctx, uint32_t op, uint32_t n, const float* x, const float* a, float* out);

/* Test hook for the filter of rt_accum_denoise (rtow_mi355x.h "denoising"): the same kernel over host arrays in image order — rgb
 * [3 * nx * rows] = c, y and v [nx * rows] — with `dn` as rt_accum_denoise reads it (NULL: the defaults); out_rgb_f32 [3 * nx * rows].
 * No scene and no accumulation is needed: the tests feed borders, NaNs and zero variances at chosen sizes.  RT_ERR_INVALID: a NULL
 * array, nx * rows outside 1 .. 2^28, or parameters rt_accum_denoise would refuse. */
int rt_debug_denoise(RtCtx* ctx, uint32_t nx, uint32_t rows, const float* rgb, const float* y, const float* v, const RtDenoise* dn,
                     float* out_rgb_f32);
/* The same for the colour-guided filter of rt_accum_denoise_channels (rtow_mi355x.h "channel moments and the colour-guided filter"):
 * rgb [3 * nx * rows] = c and var_rgb [3 * nx * rows] = the three channel variances, both in image order; errors as rt_debug_denoise. */
int rt_debug_denoise_channels(RtCtx* ctx, uint32_t nx, uint32_t rows, const float* rgb, const float* var_rgb, const RtDenoise* dn,
                              float* out_rgb_f32);
/* Test hook for rt_accum_denoise_multiscale (rtow_mi355x.h "multi-scale denoising"): the same kernels over host arrays in image order, as
 * the two hooks above take them.  guide RT_DENOISE_GUIDE_LUMINANCE: rgb [3 * nx * rows] = c, mean and var [nx * rows] = y and v;
 * RT_DENOISE_GUIDE_CHANNELS: `mean` is not read (may be NULL) and var [3 * nx * rows] holds the three channel variances.  out_rgb_f32
 * [3 * nx * rows] = o_0.  The probe arrays that are not NULL receive the filter's INPUTS of level probe_level < levels, sized by
 * rt_denoise_level_size: probe_rgb [3 * n] = c, probe_mean and probe_var [n] = y and v, or with the channels guide probe_mean = c again
 * and probe_var [3 * n] — so that a wrong downsample shows apart from a wrong combine.  RT_ERR_INVALID: a NULL array, nx * rows outside
 * 1 .. 2^28, parameters rt_accum_denoise_multiscale would refuse, a probe array with probe_level >= levels. */
int rt_debug_denoise_multiscale(RtCtx* ctx, uint32_t nx, uint32_t rows, uint32_t guide, const float* rgb, const float* mean, const float* var,
                                const RtDenoise* dn, uint32_t levels, float* out_rgb_f32, uint32_t probe_level, float* probe_rgb,
                                float* probe_mean, float* probe_var);
/* Test hook for rt_accum_denoise_select (rtow_mi355x.h "selected strength"): the same kernels over host arrays in image order.  c0 and
 * c1 [3 * nx * rows] = c_0 and c_1; yv0 and yv1 [2 * nx * rows] = (y_h, v_h) per pixel, interleaved, NaN where the half has no variance.
 * The sample counts n_h follow from (first_sample, n) as in "Half buffers", with n = counts[p] per pixel where `counts` [nx * rows] is not
 * NULL.  `sel` as rt_accum_denoise_select reads it (NULL: the defaults).  out_rgb_f32 [3 * nx * rows], out_index and out_est [nx * rows]
 * and `info` as that call writes them, each may be NULL.  The probe arrays that are not NULL receive out_j [3 * nx * rows] and E_j
 * [nx * rows] of the candidate j = probe_candidate < K — so that a wrong candidate shows apart from a wrong choice or blend.  No scene and
 * no accumulation is needed.  RT_ERR_INVALID: a NULL input array, nx * rows outside 1 .. 2^28, an RtSelect rt_select_check refuses, a probe
 * array with probe_candidate >= K. */
int rt_debug_denoise_select(RtCtx* ctx, uint32_t nx, uint32_t rows, const float* c0, const float* c1, const float* yv0, const float* yv1,
                            const uint32_t* counts, uint32_t first_sample, uint32_t n, const RtSelect* sel, float* out_rgb_f32,
                            uint8_t* out_index, float* out_est, RtSelectInfo* info, uint32_t probe_candidate, float* probe_out, float* probe_err);
/* Which filter chain the selection of this context runs, the hook above and the product call alike; both give the same bits.
 * RT_SELECT_CHAIN_AUTO: the library's choice; _PLAIN: 2 K launches of the filter of "Denoising"; _FUSED: one launch per half that filters
 * with all K strengths.  A per-context setting that changes no sample: it does not end an open accumulation.  RT_ERR_INVALID: another value. */
#define RT_SELECT_CHAIN_AUTO 0u
#define RT_SELECT_CHAIN_PLAIN 1u
#define RT_SELECT_CHAIN_FUSED 2u
int rt_debug_select_chain(RtCtx* ctx, uint32_t chain);
/* Test hook for the display transform (rtow_mi355x.h "display transform"): the same kernels over a host image in the row order of an
 * out_rgb_f32 — rgb [3 * nx * rows] — under `display` (not the context's, which it neither reads nor changes; nor does it touch what
 * rt_display_info returns); out_rgb8 [3 * nx * rows], rows flipped as every out_rgb8, and `info` (may be NULL) the figures of this run.
 * No scene and no accumulation is needed.  RT_ERR_INVALID: a NULL array or display, nx * rows outside 1 .. 2^28, or a display
 * rt_display_check refuses. */
int rt_debug_display(RtCtx* ctx, uint32_t nx, uint32_t rows, const float* rgb, const RtDisplay* display, uint8_t* out_rgb8, RtDisplayInfo* info);
/* Test hook for the glare (rtow_mi355x.h "Glare"): the same kernels over a host image in the row order of an out_rgb_f32 — rgb
 * [3 * nx * rows] — under `glare` and, behind it, `display` (NULL: the reference quantisation); neither is the context's, which the hook
 * neither reads nor changes, nor does it touch what rt_glare_info, rt_glare_image and rt_display_info return.  out_rgb_f32 [3 * nx * rows]
 * (may be NULL): `out`; out_rgb8 [3 * nx * rows] (may be NULL), rows flipped as every out_rgb8; `info` (may be NULL): Le and the coarsest
 * level of this run.  No scene and no accumulation is needed.  RT_ERR_INVALID: a NULL rgb or glare, nx * rows outside 1 .. 2^28, a glare
 * rt_glare_check refuses or a display rt_display_check refuses. */
int rt_debug_glare(RtCtx* ctx, uint32_t nx, uint32_t rows, const float* rgb, const RtGlare* glare, const RtDisplay* display, float* out_rgb_f32,
                   uint8_t* out_rgb8, RtGlareInfo* info);
/* Which down chain the glare of this context runs, the hook above and the product calls alike; both give the same bits.
 * RT_GLARE_CHAIN_AUTO: the library's choice; _PLAIN: one launch per level; _FUSED: levels 1 .. 3 in one launch wherever Le >= 3.
 * A per-context setting that changes no sample: it does not end an open accumulation.  RT_ERR_INVALID: another value. */
#define RT_GLARE_CHAIN_AUTO 0u
#define RT_GLARE_CHAIN_PLAIN 1u
#define RT_GLARE_CHAIN_FUSED 2u
int rt_debug_glare_chain(RtCtx* ctx, uint32_t chain);

/* Test hook for adaptive sampling (rtow_mi355x.h "adaptive sampling"): overwrites the two luminance moments (S1, S2) of pixel `pixel` of
 * the open accumulation, `pixel` an index into out_sem (row order of out_rgb_f32).  The tests plant a NaN with it: such a pixel never
 * converges and spreads to no other.  The f32 sum and n_p stay.  RT_ERR_STATE: no open accumulation; RT_ERR_INVALID: pixel outside the shard. */
int rt_debug_accum_set_moments(RtCtx* ctx, uint32_t pixel, double s1, double s2);
/* Test hook for the pixel filters (rtow_mi355x.h "pixel reconstruction filters"): the production kernel k_resolve_filter<false> over a host
 * array of radiance, rad [n_samples][rows][nx][3] in the row order of out_rgb_f32, as the samples with the absolute indices i0 .. i0 +
 * n_samples - 1, onto the filter plane of the open accumulation ONLY: its sums, moments, counts and `done` are untouched.  Designed radiance
 * (an impulse, a NaN, 1e30) reaches the kernel without a trace.  RT_ERR_STATE: no open accumulation, or it does not track a filter;
 * RT_ERR_INVALID: rad NULL, n_samples 0 or above 4096, i0 + n_samples above 2^32. */
int rt_debug_filter_add(RtCtx* ctx, uint32_t i0, uint32_t n_samples, const float* rad);
/* Test hook for the first-hit features (rtow_mi355x.h "First-hit features"): the production kernel k_features over the samples with the
 * absolute indices i0 .. i0 + n_samples - 1 of every pixel, onto the feature records of the open accumulation ONLY: nothing is traced, and
 * its sums, moments, counts and `done` are untouched.  The search form is the one an add would use: the tree as the scene upload placed it,
 * or every primitive where the context has no tree or the accumulation's RtParams hold RT_FLAG_BRUTE_FORCE.  RT_ERR_STATE: no open
 * accumulation, or it does not track features; RT_ERR_INVALID: n_samples 0 or above 4096, i0 + n_samples above 2^32. */
int rt_debug_features_add(RtCtx* ctx, uint32_t i0, uint32_t n_samples);
/* Test hook for the feature-guided filter (rtow_mi355x.h "The feature-guided filter"): the kernels of rt_accum_denoise_features — the
 * demodulation, then k_denoise_features — over host arrays in image order: rgb [rows*nx*3], y and v [rows*nx], feat_mean [rows*nx*7]
 * (abar 3, nbar 3, zbar) and feat_var [rows*nx*3] (va, vn, vz) -> out_rgb_f32 [rows*nx*3].  No accumulation is needed.  RT_ERR_INVALID: a
 * NULL array, nx * rows outside 1 .. 2^28, what rt_accum_denoise refuses of `dn`, what rt_feature_guide_check refuses of `guide`. */
int rt_debug_denoise_features(RtCtx* ctx, uint32_t nx, uint32_t rows, const float* rgb, const float* y, const float* v, const float* feat_mean, const float* feat_var,
                              const RtDenoise* dn, const RtFeatureGuide* guide, float* out_rgb_f32);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_MI355X_DEBUG_H */
