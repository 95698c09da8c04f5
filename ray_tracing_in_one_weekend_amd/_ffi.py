"""ctypes declarations of the two C ABIs (include/rtow_mi355x.h + its test hooks in include/rtow_mi355x_debug.h, include/rtow_host.h).

Plumbing only: struct layouts, library loading and argument types.  The GPU library is
mandatory for rendering; `load_gpu_library()` raises if it is missing — there is no CPU
fallback in the product path.
"""
import ctypes as C
import os

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# RTOW_GPU_LIB selects an alternative build of the SAME sources (A/B experiments, scripts/ only)
GPU_LIB_PATH = os.environ.get("RTOW_GPU_LIB") or os.path.join(_PKG_DIR, "librtow_mi355x.so")
HOST_LIB_PATH = os.path.join(_PKG_DIR, "librtow_host.so")

RT_NO_TEX = 0xFFFFFFFF
ERR_INVALID, ERR_DEVICE, ERR_NOMEM, ERR_UNSUPPORTED, ERR_STATE = 1, 2, 3, 4, 5  # magnitudes of the negative RT_ERR_* codes
FLAG_BRUTE_FORCE = 1
FLAG_RUSSIAN_ROULETTE = 2
FLAG_TIME_DEPTHS = 4
FLAG_PRODUCTION_KERNELS = 8  # rt_debug_bounce through the ray queue and the kernels rt_render launches
RTH_INVALID = 0xFFFFFFFF

# enum RtMatType
(MAT_EMISSION, MAT_DIFFUSE, MAT_LAMBERT, MAT_METAL, MAT_DIELECTRIC, MAT_ISOTROPIC, MAT_OREN_NAYAR,
 MAT_BURLEY_DIFFUSE, MAT_ROUGH_PLASTIC, MAT_DISNEY_DIFFUSE, MAT_DISNEY_METAL, MAT_DISNEY_SHEEN,
 MAT_DISNEY_CLEARCOAT) = range(13)
# enum RtTexType
TEX_CONSTANT, TEX_CHECKER, TEX_PERLIN, TEX_IMAGE = range(4)
# enum RtRectAxis
RECT_YZ, RECT_XZ, RECT_XY = range(3)
# enum RtXformType
XF_TRANSLATE, XF_ROTATE_Y = range(2)
NO_XFORM = 0xFFFFFFFF
# enum RtSkyType
SKY_GRADIENT, SKY_BLACK, SKY_ENV = range(3)

_f = C.POINTER(C.c_float)
_u8 = C.POINTER(C.c_uint8)
_u16 = C.POINTER(C.c_uint16)
_u32 = C.POINTER(C.c_uint32)
_u64 = C.POINTER(C.c_uint64)


class RtFlatScene(C.Structure):
    _fields_ = [
        ("n_spheres", C.c_uint32),
        ("sph_cx", _f), ("sph_cy", _f), ("sph_cz", _f), ("sph_r", _f), ("sph_mat", _u32),
        ("n_rects", C.c_uint32),
        ("rect_axis", _u8), ("rect_min", _f), ("rect_max", _f), ("rect_mat", _u32),
        ("n_xforms", C.c_uint32),
        ("xf_type", _u8), ("xf_param", _f), ("xf_parent", _u32), ("sph_xform", _u32), ("rect_xform", _u32),
        ("n_media", C.c_uint32),
        ("med_neg_inv_density", _f), ("med_mat", _u32), ("sph_medium", _u32), ("rect_medium", _u32), ("med_xform", _u32),
        ("n_materials", C.c_uint32),
        ("mat_type", _u8), ("mat_color", _f), ("mat_p0", _f), ("mat_p1", _f), ("mat_p2", _f), ("mat_p3", _f),
        ("mat_tex0", _u32), ("mat_tex1", _u32),
        ("n_textures", C.c_uint32),
        ("tex_type", _u8), ("tex_color0", _f), ("tex_color1", _f), ("tex_scale", _f), ("tex_aux", _u32),
        ("n_perlin", C.c_uint32),
        ("perlin_vec", _f), ("perlin_perm", _u16),
        ("n_images", C.c_uint32),
        ("img_w", _u32), ("img_h", _u32), ("img_offset", _u64), ("texels", _f), ("n_texel_floats", C.c_uint64),
        ("sky_type", C.c_uint32), ("sky_image", C.c_uint32),
    ]


class RtCamera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("lower_left_corner", C.c_float * 3)]


class RtLens(C.Structure):
    """rt_set_lens: the book's thin lens, lens_radius = aperture / 2; lens_radius 0 = the pinhole."""
    _fields_ = [("lens_radius", C.c_float), ("focus_dist", C.c_float)]


class RtMotion(C.Structure):
    """rt_set_motion: sphere `sphere[k]` moves linearly from its RtFlatScene centre (time 0) to center1[3 k ..] (time 1); a path's
    time lies in [shutter_open, shutter_close]."""
    _fields_ = [("n_moving", C.c_uint32), ("sphere", C.POINTER(C.c_uint32)), ("center1", C.POINTER(C.c_float)),
                ("shutter_open", C.c_float), ("shutter_close", C.c_float)]


class RtQuads(C.Structure):
    """rt_set_quads: planar primitive i is the quad Q + a u + b v (kind 0) or the triangle Q, Q + u, Q + v (kind 1) with material
    mat[i] of the uploaded scene; it is primitive n_spheres + n_rects + n_media + i."""
    _fields_ = [("n", C.c_uint32), ("q", C.POINTER(C.c_float)), ("u", C.POINTER(C.c_float)), ("v", C.POINTER(C.c_float)),
                ("kind", C.POINTER(C.c_uint8)), ("mat", C.POINTER(C.c_uint32))]


class RtLights(C.Structure):
    """rt_set_lights: light i is the world-space parallelogram Q + a u + b v, a sampling target only (no geometry, no material)."""
    _fields_ = [("n", C.c_uint32), ("q", C.POINTER(C.c_float)), ("u", C.POINTER(C.c_float)), ("v", C.POINTER(C.c_float))]


MAX_LIGHTS = 16
PLANAR_QUAD, PLANAR_TRIANGLE = 0, 1
PLANAR_MIN_SIN2 = 2.0 ** -20
PLANAR_REACH = 16.0


class RtParams(C.Structure):
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("spp", C.c_uint32), ("max_depth", C.c_int32),
                ("seed", C.c_uint64), ("shard_band", C.c_uint32), ("shard_count", C.c_uint32),
                ("shard_id", C.c_uint32), ("spp_slice", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class RtStats(C.Structure):
    _fields_ = [("n_paths", C.c_uint64), ("n_rays", C.c_uint64), ("n_rays_secondary", C.c_uint64),
                ("n_texture_fetches", C.c_uint64), ("n_bad_dir", C.c_uint64), ("seconds_total", C.c_double),
                ("seconds_trace", C.c_double), ("seconds_device", C.c_double), ("bytes_algorithmic", C.c_uint64),
                ("bytes_trace_algorithmic", C.c_uint64), ("n_trace_launches", C.c_uint32), ("n_slices", C.c_uint32),
                ("rays_per_depth", C.c_uint64 * 64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "rays_per_depth"}
        d["rays_per_depth"] = list(self.rays_per_depth)
        return d


class RtNoise(C.Structure):
    """rt_accum_read / rt_render_to_noise: the frame figures of an accumulation (rtow_mi355x.h "progressive accumulation")."""
    _fields_ = [("spp_done", C.c_uint32), ("reserved", C.c_uint32), ("mean_luminance", C.c_double), ("rms_sem", C.c_double),
                ("noise", C.c_double)]


class RtDenoise(C.Structure):
    """rt_accum_denoise: window radius (1..MAX), patch radius (0..MAX) and strength k of the variance-guided non-local-means filter
    (rtow_mi355x.h "denoising")."""
    _fields_ = [("radius", C.c_uint32), ("patch", C.c_uint32), ("strength", C.c_float), ("reserved", C.c_uint32)]


class RtAdaptive(C.Structure):
    """rt_accum_add_adaptive / rt_render_adaptive: a pixel stops once it holds min_samples samples and the variance of its mean luminance
    is at most (tolerance * max(mean luminance, luminance_floor))^2 (rtow_mi355x.h "adaptive sampling")."""
    _fields_ = [("tolerance", C.c_double), ("luminance_floor", C.c_double), ("min_samples", C.c_uint32), ("reserved", C.c_uint32)]


class RtAdaptiveInfo(C.Structure):
    """rt_accum_read_counts: pixels still active, the sum of the per-pixel sample counts and their extremes over the shard."""
    _fields_ = [("n_active", C.c_uint64), ("n_samples", C.c_uint64), ("spp_min", C.c_uint32), ("spp_max", C.c_uint32)]


ACCUM_STATE_COUNTS, ACCUM_STATE_CHANNELS = 1, 2  # RT_ACCUM_STATE_*


class RtAccumState(C.Structure):
    """rt_accum_export / rt_accum_import / rt_accum_merge: what an accumulation owns, as host arrays in the row order of the f32 image
    (rtow_mi355x.h "accumulation state")."""
    _fields_ = [("nx", C.c_uint32), ("rows", C.c_uint32), ("first_sample", C.c_uint32), ("done", C.c_uint32), ("planes", C.c_uint32),
                ("reserved", C.c_uint32), ("frame_id", C.c_uint64), ("sum", _f), ("moments", C.POINTER(C.c_double)), ("counts", _u32),
                ("converged", _u8), ("channel_moments", C.POINTER(C.c_double))]


DENOISE_MAX_RADIUS, DENOISE_MAX_PATCH = 10, 3
DENOISE_DEFAULT_STRENGTH = 1.0  # RT_DENOISE_DEFAULT_STRENGTH
DENOISE_HALVES_DEFAULT_STRENGTH = 0.7  # RT_DENOISE_HALVES_DEFAULT_STRENGTH


DENOISE_MAX_LEVELS, DENOISE_DEFAULT_LEVELS = 4, 2  # RT_DENOISE_MAX_LEVELS, RT_DENOISE_DEFAULT_LEVELS
DENOISE_GUIDE_LUMINANCE, DENOISE_GUIDE_CHANNELS = 0, 1  # RT_DENOISE_GUIDE_*


class RtMultiscale(C.Structure):
    """rt_accum_denoise_multiscale: the levels of the 2x pyramid (1..MAX) and which filter runs on them (rtow_mi355x.h "multi-scale
    denoising")."""
    _fields_ = [("levels", C.c_uint32), ("guide", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RtResidual(C.Structure):
    """rt_accum_denoise_halves: the frame figures of the cross-filtered frame (rtow_mi355x.h "half buffers"); residual_rms is the variance
    half of the filtered frame's error, a lower bound."""
    _fields_ = [("mean_luminance", C.c_double), ("residual_rms", C.c_double), ("residual_noise", C.c_double), ("reserved", C.c_uint32 * 2)]


class RtAccumHalves(C.Structure):
    """rt_accum_export_halves / rt_accum_import_halves: the two half buffers of an accumulation, as host arrays in the row order of the f32
    image (rtow_mi355x.h "half buffers")."""
    _fields_ = [("nx", C.c_uint32), ("rows", C.c_uint32), ("first_sample", C.c_uint32), ("done", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("frame_id", C.c_uint64), ("sum", _f * 2), ("moments", C.POINTER(C.c_double) * 2)]


SELECT_MAX, SELECT_MAX_WINDOW = 4, 4  # RT_SELECT_MAX, RT_SELECT_MAX_WINDOW
SELECT_CHAIN_AUTO, SELECT_CHAIN_PLAIN, SELECT_CHAIN_FUSED = range(3)  # rt_debug_select_chain
SELECT_DEFAULT_STRENGTHS = (0.7, 1.0, 1.4)  # `sel` NULL of rt_accum_denoise_select, with radius 5, patch 1, error_radius 0, blend_radius 1


class RtSelect(C.Structure):
    """rt_accum_denoise_select: the candidate strengths of the cross filter, its window and patch, and the radii of the window the error
    estimate is smoothed over and of the one the choice is blended over (rtow_mi355x.h "selected strength")."""
    _fields_ = [("n_strengths", C.c_uint32), ("strength", C.c_float * 4), ("radius", C.c_uint32), ("patch", C.c_uint32),
                ("error_radius", C.c_uint32), ("blend_radius", C.c_uint32), ("reserved", C.c_uint32)]


class RtSelectInfo(C.Structure):
    """rt_accum_denoise_select: per candidate the estimated luminance MSE of a half filter over the usable pixels, that of the selection
    (biased low by the minimum), how many pixels chose each candidate, and `best`, the frame-wide choice."""
    _fields_ = [("est_mse", C.c_double * 4), ("est_mse_selected", C.c_double), ("chosen", C.c_uint32 * 4), ("usable", C.c_uint32),
                ("best", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def as_dict(self):
        return {"est_mse": list(self.est_mse), "est_mse_selected": self.est_mse_selected, "chosen": list(self.chosen), "usable": self.usable,
                "best": self.best}


BUCKETS_MAX = 16  # RT_BUCKETS_MAX
ROBUST_GINI, ROBUST_MEDIAN, ROBUST_TRIM = 0, 1, 2  # RT_ROBUST_*


class RtRobust(C.Structure):
    """rt_accum_read_robust / rt_accum_denoise_robust: how the trim of the sorted bucket means is chosen (rtow_mi355x.h "sample buckets")."""
    _fields_ = [("mode", C.c_uint32), ("trim", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RtRobustInfo(C.Structure):
    """rt_accum_read_robust: the frame figures of the robust read-out; energy_removed is the share of the frame's luminance the trim took
    away — the estimator is biased."""
    _fields_ = [("mean_luminance_plain", C.c_double), ("mean_luminance_robust", C.c_double), ("energy_removed", C.c_double),
                ("trimmed_fraction", C.c_double), ("nonfinite_dropped", C.c_uint64)]


class RtAccumBuckets(C.Structure):
    """rt_accum_export_buckets / rt_accum_import_buckets: the M bucket sums of an accumulation, as host arrays in the row order of the f32
    image (rtow_mi355x.h "sample buckets")."""
    _fields_ = [("nx", C.c_uint32), ("rows", C.c_uint32), ("first_sample", C.c_uint32), ("done", C.c_uint32), ("M", C.c_uint32),
                ("reserved", C.c_uint32), ("frame_id", C.c_uint64), ("sum", _f * BUCKETS_MAX)]


# enum RtExposureMode, RtToneCurve, RtTransfer, RtDither (rt_set_display)
EXPOSURE_MANUAL, EXPOSURE_KEY, EXPOSURE_PERCENTILE = range(3)
TONE_CLAMP, TONE_REINHARD, TONE_ACES = range(3)
TRANSFER_GAMMA2, TRANSFER_SRGB = range(2)
DITHER_NONE, DITHER_BAYER8 = range(2)
DISPLAY_SRGB_EPS = 2.0 ** -20  # RT_DISPLAY_SRGB_EPS


class RtDisplay(C.Structure):
    """rt_set_display: exposure (manual, or measured from the frame), tone curve, transfer function and dither behind every out_rgb8 of
    the accumulation family (rtow_mi355x.h "display transform")."""
    _fields_ = [("exposure_mode", C.c_uint32), ("exposure_value", C.c_float), ("percentile", C.c_float), ("curve", C.c_uint32),
                ("white", C.c_float), ("transfer", C.c_uint32), ("dither", C.c_uint32), ("reserved", C.c_uint32)]


class RtDisplayInfo(C.Structure):
    """rt_display_info: the exposure that was applied and the figures of the last out_rgb8 written under a display."""
    _fields_ = [("exposure", C.c_float), ("percentile_luminance", C.c_float), ("log_average", C.c_double), ("n_lit", C.c_uint64),
                ("n_non_finite", C.c_uint64), ("n_saturated", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# rt_accum_track_filter
FILTER_BOX, FILTER_TENT, FILTER_GAUSSIAN, FILTER_MITCHELL, FILTER_BLACKMAN_HARRIS = range(5)  # RT_FILTER_*
FILTER_TABLE, FILTER_MIN_RADIUS, FILTER_MAX_RADIUS = 256, 0.5, 3.0  # RT_FILTER_TABLE, RT_FILTER_MIN_RADIUS, RT_FILTER_MAX_RADIUS


class RtPixelFilter(C.Structure):
    """rt_accum_track_filter: the separable reconstruction filter of an accumulation, its radius in pixels and the parameters of its kind
    (rtow_mi355x.h "pixel reconstruction filters")."""
    _fields_ = [("kind", C.c_uint32), ("radius", C.c_float), ("p0", C.c_float), ("p1", C.c_float)]


class RtAccumFilter(C.Structure):
    """rt_accum_export_filter / rt_accum_import_filter: the filter and the plane (sum w rgb, sum w) of an accumulation, as a host array in the
    row order of the f32 image."""
    _fields_ = [("nx", C.c_uint32), ("rows", C.c_uint32), ("first_sample", C.c_uint32), ("done", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("frame_id", C.c_uint64), ("filter", RtPixelFilter), ("plane", _f)]


# rt_accum_track_features
FEATURES_MIN_STRIDE, FEATURES_MAX_STRIDE = 1, 64  # RT_FEATURES_MIN_STRIDE, RT_FEATURES_MAX_STRIDE


class RtFeatures(C.Structure):
    """rt_accum_track_features: every stride-th sample, by absolute index, takes a first-hit feature sample (rtow_mi355x.h "First-hit
    features")."""
    _fields_ = [("stride", C.c_uint32), ("reserved", C.c_uint32)]


class RtFeaturePixel(C.Structure):
    """The feature record of one pixel: the f32 sums of albedo and normal with their counts, and the f64 moments."""
    _fields_ = [("albedo", C.c_float * 3), ("n_f", C.c_uint32), ("normal", C.c_float * 3), ("n_h", C.c_uint32),
                ("a2", C.c_double), ("n2", C.c_double), ("z1", C.c_double), ("z2", C.c_double)]


FEATURE_USE_ALBEDO, FEATURE_USE_NORMAL, FEATURE_USE_DEPTH = 1, 2, 4  # RT_FEATURE_USE_*
FEATURE_GUIDE_DEFAULT_K, FEATURE_GUIDE_DEFAULT_TAU = 0.6, 1e-3  # RT_FEATURE_GUIDE_DEFAULT_*


class RtFeatureGuide(C.Structure):
    """rt_accum_denoise_features: the strengths and variance floors of the three feature distances, which of them are used, and whether
    the colour is filtered demodulated by the albedo (rtow_mi355x.h "The feature-guided filter")."""
    _fields_ = [("k_albedo", C.c_float), ("k_normal", C.c_float), ("k_depth", C.c_float), ("tau_albedo", C.c_float), ("tau_normal", C.c_float),
                ("tau_depth", C.c_float), ("use_mask", C.c_uint32), ("demodulate", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RtAccumFeatures(C.Structure):
    """rt_accum_export_features / rt_accum_import_features: the stride and the records of an accumulation, as a host array in the row order
    of the f32 image."""
    _fields_ = [("nx", C.c_uint32), ("rows", C.c_uint32), ("first_sample", C.c_uint32), ("done", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("frame_id", C.c_uint64), ("features", RtFeatures), ("plane", C.POINTER(RtFeaturePixel))]


# rt_set_glare
GLARE_MAX_LEVELS, GLARE_DEFAULT_LEVELS = 8, 6
GLARE_DEFAULT_AMOUNT, GLARE_DEFAULT_SPREAD = 0.1, 0.7
GLARE_CHAIN_AUTO, GLARE_CHAIN_PLAIN, GLARE_CHAIN_FUSED = range(3)  # rt_debug_glare_chain


class RtGlare(C.Structure):
    """rt_set_glare: the share of every pixel's bright pass that a 2x pyramid spreads over its neighbourhood, in front of the display
    stage of every out_rgb8 of the accumulation family (rtow_mi355x.h "Glare")."""
    _fields_ = [("amount", C.c_float), ("spread", C.c_float), ("threshold", C.c_float), ("levels", C.c_uint32)]


class RtGlareInfo(C.Structure):
    """rt_glare_info: the effective levels Le and the size of the coarsest level of the last out_rgb8 written under a glare."""
    _fields_ = [("levels", C.c_uint32), ("coarse_nx", C.c_uint32), ("coarse_rows", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RtBounceIO(C.Structure):
    _fields_ = [("n", C.c_uint32), ("depth", C.c_uint32), ("in_o", _f), ("in_d", _f), ("in_key", _u32),
                ("out_hit", C.POINTER(C.c_int32)), ("out_t", _f), ("out_radiance", _f), ("out_attenuation", _f),
                ("out_o", _f), ("out_d", _f), ("out_alive", _u8), ("flags", C.c_uint32)]


# void (*RtProgressFn)(void* user, uint32_t spp_done, uint32_t spp_total, const uint8_t* rgb8, uint32_t nx, uint32_t rows)
RtProgressFn = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32)

MULTI_COPY_GATHER = 1  # RT_MULTI_COPY_GATHER (rt_multi_create_ex)
MULTI_TRACK_CHANNELS, MULTI_TRACK_HALVES, MULTI_TRACK_BUCKETS = 1, 2, 4  # RT_MULTI_TRACK_* (rt_multi_accum_begin)
MULTI_UNSUPPORTED_FEATURES = 32  # RT_MULTI_UNSUPPORTED_FEATURES: declared so that it can be refused (RT_ERR_UNSUPPORTED); 8 and 16 are no track bits
# enum RtDebugOption (rt_debug_set_option): per context, every setting renders the same bits
(OPT_TREE_PLACEMENT, OPT_PRIMARY_LISTS, OPT_PIXEL_ORDER, OPT_TEXEL_POOL, OPT_GRID, OPT_GRID_CELL, OPT_CHAINS,
 OPT_GENERAL_KERNELS, OPT_GENERAL_LDS, OPT_QUEUE_SHARDS, OPT_ISECT_WORKGROUPS, OPT_MATERIALISE_PRIMARIES, OPT_MEDIUM_SEARCH, OPT_POOL_CHUNK_DELAY_US) = range(14)
OPT_NAMES = {"tree_placement": OPT_TREE_PLACEMENT, "primary_lists": OPT_PRIMARY_LISTS, "pixel_order": OPT_PIXEL_ORDER,
             "texel_pool": OPT_TEXEL_POOL, "grid": OPT_GRID, "grid_cell": OPT_GRID_CELL, "chains": OPT_CHAINS,
             "general_kernels": OPT_GENERAL_KERNELS, "general_lds": OPT_GENERAL_LDS, "queue_shards": OPT_QUEUE_SHARDS,
             "isect_workgroups": OPT_ISECT_WORKGROUPS, "materialise_primaries": OPT_MATERIALISE_PRIMARIES,
             "medium_search": OPT_MEDIUM_SEARCH, "pool_chunk_delay_us": OPT_POOL_CHUNK_DELAY_US}


class RtSceneInfo(C.Structure):
    _fields_ = [("n_entries", C.c_uint32), ("n_tree_nodes", C.c_uint32), ("tree_depth", C.c_uint32), ("tree_in_lds", C.c_uint32),
                ("general_kernels", C.c_uint32), ("closest_hit_lds_bytes", C.c_uint32), ("grid", C.c_uint32),
                ("grid_cells", C.c_uint32 * 3), ("grid_refs", C.c_uint32), ("grid_always", C.c_uint32),
                ("grid_lds_bytes", C.c_uint32), ("grid_cell_size", C.c_float * 3), ("general_tables_in_lds", C.c_uint32), ("nest", C.c_uint32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("grid_cells", "grid_cell_size")}
        d["grid_cells"], d["grid_cell_size"] = list(self.grid_cells), [float(x) for x in self.grid_cell_size]
        return d


class RtVariantLedger(C.Structure):
    """rt_debug_variant_tables / rt_debug_launched_variants: one bit per key of a kernel family (bit k & 31 of word k >> 5), one word per
    search form of k_debug_bounce, one bit per closest-hit kernel outside the tables."""
    _fields_ = [("shade", C.c_uint32 * 8), ("intersect", C.c_uint32 * 8), ("debug_bounce", C.c_uint32 * 3), ("untabled", C.c_uint32)]


# RT_FAMILY_* of rt_debug_variant_flag_names (tests/test_abi.py holds them against the header); every NAME comes from the library
FAMILY_SHADE, FAMILY_INTERSECT, FAMILY_DEBUG_BOUNCE, FAMILY_UNTABLED, FAMILY_DEBUG_FORMS = range(5)

EXPECTED_ABI = 11  # RT_ABI_VERSION the struct layouts and prototypes below were written for
GPU_SYMBOLS = ["rt_abi_version", "rt_build_id", "rt_ctx_create", "rt_ctx_destroy", "rt_last_error", "rt_scene_upload",
               "rt_shard_rows", "rt_shard_row_to_image_row", "rt_prepare", "rt_render", "rt_render_device", "rt_debug_bounce", "rt_debug_arithmetic",
               "rt_get_depth_timings", "rt_set_progress", "rt_host_alloc", "rt_host_free", "rt_debug_set_option", "rt_debug_get_option",
               "rt_debug_scene_info", "rt_debug_grid_build", "rt_debug_world_bounds", "rt_debug_render_parts", "rt_multi_create", "rt_multi_create_ex", "rt_multi_destroy", "rt_multi_device_count",
               "rt_multi_last_error", "rt_multi_scene_upload", "rt_multi_render", "rt_deinterleave_bands", "rt_set_lens", "rt_multi_set_lens",
               "rt_set_motion", "rt_multi_set_motion", "rt_debug_motion_bounds",
               "rt_set_quads", "rt_multi_set_quads", "rt_debug_planar_info", "rt_debug_planar_bounds",
               "rt_set_lights", "rt_multi_set_lights",
               "rt_accum_begin", "rt_accum_add", "rt_accum_read", "rt_accum_end", "rt_render_to_noise",
               "rt_accum_denoise", "rt_debug_denoise",
               "rt_accum_track_channels", "rt_accum_read_channel_sem", "rt_accum_denoise_channels", "rt_debug_denoise_channels",
               "rt_denoise_level_size", "rt_accum_denoise_multiscale", "rt_debug_denoise_multiscale",
               "rt_accum_add_adaptive", "rt_accum_read_counts", "rt_render_adaptive", "rt_adaptive_check", "rt_adaptive_converged",
               "rt_debug_accum_set_moments",
               "rt_accum_frame_id", "rt_accum_state_check", "rt_accum_export", "rt_accum_import", "rt_accum_merge",
               "rt_accum_track_halves", "rt_accum_read_halves", "rt_accum_denoise_halves", "rt_accum_halves_check", "rt_accum_export_halves",
               "rt_accum_import_halves",
               "rt_select_check", "rt_accum_denoise_select", "rt_debug_denoise_select", "rt_debug_select_chain",
               "rt_accum_track_buckets", "rt_accum_read_robust", "rt_accum_denoise_robust", "rt_accum_buckets_check", "rt_accum_export_buckets",
               "rt_accum_import_buckets",
               "rt_multi_accum_begin", "rt_multi_accum_add", "rt_multi_accum_add_adaptive", "rt_multi_accum_join", "rt_multi_accum_import", "rt_multi_accum_end",
               "rt_set_display", "rt_display_info", "rt_display_check", "rt_debug_display",
               "rt_set_glare", "rt_glare_check", "rt_glare_info", "rt_glare_image", "rt_debug_glare", "rt_debug_glare_chain",
               "rt_pixel_filter_check", "rt_pixel_filter_table", "rt_accum_track_filter", "rt_accum_read_filtered", "rt_accum_filter_check",
               "rt_accum_export_filter", "rt_accum_import_filter", "rt_debug_filter_add",
               "rt_features_check", "rt_accum_track_features", "rt_accum_read_features", "rt_accum_features_check", "rt_accum_export_features",
               "rt_accum_import_features", "rt_debug_features_add", "rt_feature_guide_check", "rt_accum_denoise_features", "rt_debug_denoise_features",
               "rt_debug_variant_tables", "rt_debug_variant_flag_names", "rt_debug_launched_variants"]
HOST_SYMBOLS = ["rth_last_error", "rth_register_image", "rth_rng_reseed", "rth_scene_build", "rth_scene_new",
                "rth_tex_constant", "rth_tex_checker", "rth_tex_perlin", "rth_tex_image", "rth_material",
                "rth_sphere", "rth_rect", "rth_gbox", "rth_translate", "rth_rotate_y", "rth_constant_medium", "rth_hitable_bbox", "rth_set_sky", "rth_set_camera", "rth_scene_finish", "rth_scene_flat",
                "rth_scene_camera", "rth_scene_sphere_name", "rth_scene_free", "rth_png_write", "rth_output_file_name",
                "rth_set_camera_lens", "rth_scene_lens",
                "rth_moving_sphere", "rth_set_camera_shutter", "rth_scene_motion",
                "rth_quad", "rth_triangle", "rth_scene_quads", "rth_scene_lights"]

_gpu_lib = None
_host_lib = None


class GpuLibraryMissing(RuntimeError):
    pass


def load_gpu_library():
    """Loads librtow_mi355x.so (hand-written HIP kernels + C-ABI).  Raises if it is not built."""
    global _gpu_lib
    if _gpu_lib is not None:
        return _gpu_lib
    if not os.path.exists(GPU_LIB_PATH):
        raise GpuLibraryMissing(
            f"{GPU_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the render path.")
    lib = C.CDLL(GPU_LIB_PATH)
    vp = C.c_void_p
    lib.rt_abi_version.restype = C.c_uint32
    if lib.rt_abi_version() != EXPECTED_ABI:  # a stale .so would be read with the wrong struct layouts
        raise GpuLibraryMissing(f"{GPU_LIB_PATH} has ABI version {lib.rt_abi_version()}, this package expects {EXPECTED_ABI}: "
                                "rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
    lib.rt_build_id.restype = C.c_char_p
    lib.rt_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.rt_ctx_create.restype = C.c_int
    lib.rt_ctx_destroy.argtypes = [vp]
    lib.rt_ctx_destroy.restype = None
    lib.rt_last_error.argtypes = [vp]
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_scene_upload.argtypes = [vp, C.POINTER(RtFlatScene)]
    lib.rt_scene_upload.restype = C.c_int
    lib.rt_shard_rows.argtypes = [C.c_uint32] * 4
    lib.rt_shard_rows.restype = C.c_uint32
    lib.rt_shard_row_to_image_row.argtypes = [C.c_uint32] * 4
    lib.rt_shard_row_to_image_row.restype = C.c_uint32
    lib.rt_prepare.argtypes = [vp, C.POINTER(RtParams)]
    lib.rt_prepare.restype = C.c_int
    lib.rt_render.argtypes = [vp, C.POINTER(RtCamera), C.POINTER(RtParams), _f, _u8, C.POINTER(RtStats)]
    lib.rt_render.restype = C.c_int
    lib.rt_render_device.argtypes = [vp, C.POINTER(RtCamera), C.POINTER(RtParams), vp, vp, C.POINTER(RtStats)]
    lib.rt_render_device.restype = C.c_int
    lib.rt_get_depth_timings.argtypes = [vp, C.c_uint32, _f, _f, _u64]
    lib.rt_get_depth_timings.restype = C.c_int
    lib.rt_debug_bounce.argtypes = [vp, C.POINTER(RtBounceIO)]
    lib.rt_debug_bounce.restype = C.c_int
    lib.rt_debug_arithmetic.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.rt_debug_arithmetic.restype = C.c_int
    lib.rt_set_progress.argtypes = [vp, RtProgressFn, vp]
    lib.rt_set_progress.restype = C.c_int
    lib.rt_set_lens.argtypes = [vp, C.POINTER(RtLens)]
    lib.rt_set_lens.restype = C.c_int
    lib.rt_multi_set_lens.argtypes = [vp, C.POINTER(RtLens)]
    lib.rt_multi_set_lens.restype = C.c_int
    lib.rt_set_motion.argtypes = [vp, C.POINTER(RtMotion)]
    lib.rt_set_motion.restype = C.c_int
    lib.rt_multi_set_motion.argtypes = [vp, C.POINTER(RtMotion)]
    lib.rt_multi_set_motion.restype = C.c_int
    lib.rt_debug_motion_bounds.argtypes = [vp, vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32), C.c_float * 6, C.c_uint32 * 3, vp, vp, C.c_uint32,
                                           C.POINTER(C.c_uint32)]
    lib.rt_debug_motion_bounds.restype = C.c_int
    lib.rt_set_quads.argtypes = [vp, C.POINTER(RtQuads)]
    lib.rt_set_quads.restype = C.c_int
    lib.rt_multi_set_quads.argtypes = [vp, C.POINTER(RtQuads)]
    lib.rt_multi_set_quads.restype = C.c_int
    lib.rt_set_lights.argtypes = [vp, C.POINTER(RtLights)]
    lib.rt_set_lights.restype = C.c_int
    lib.rt_multi_set_lights.argtypes = [vp, C.POINTER(RtLights)]
    lib.rt_multi_set_lights.restype = C.c_int
    lib.rt_accum_begin.argtypes = [vp, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_uint32]
    lib.rt_accum_begin.restype = C.c_int
    lib.rt_accum_add.argtypes = [vp, C.c_uint32, C.POINTER(RtStats)]
    lib.rt_accum_add.restype = C.c_int
    lib.rt_accum_read.argtypes = [vp, _f, _u8, _f, C.POINTER(RtNoise)]
    lib.rt_accum_read.restype = C.c_int
    lib.rt_accum_end.argtypes = [vp]
    lib.rt_accum_end.restype = C.c_int
    lib.rt_render_to_noise.argtypes = [vp, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_double, C.c_uint32, _f, _u8, _f, C.POINTER(RtNoise),
                                       C.POINTER(RtStats)]
    lib.rt_render_to_noise.restype = C.c_int
    lib.rt_accum_denoise.argtypes = [vp, C.POINTER(RtDenoise), _f, _u8]
    lib.rt_accum_denoise.restype = C.c_int
    lib.rt_debug_denoise.argtypes = [vp, C.c_uint32, C.c_uint32, _f, _f, _f, C.POINTER(RtDenoise), _f]
    lib.rt_debug_denoise.restype = C.c_int
    lib.rt_accum_track_channels.argtypes = [vp]
    lib.rt_accum_track_channels.restype = C.c_int
    lib.rt_accum_read_channel_sem.argtypes = [vp, _f]
    lib.rt_accum_read_channel_sem.restype = C.c_int
    lib.rt_accum_denoise_channels.argtypes = [vp, C.POINTER(RtDenoise), _f, _u8]
    lib.rt_accum_denoise_channels.restype = C.c_int
    lib.rt_debug_denoise_channels.argtypes = [vp, C.c_uint32, C.c_uint32, _f, _f, C.POINTER(RtDenoise), _f]
    lib.rt_debug_denoise_channels.restype = C.c_int
    lib.rt_denoise_level_size.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _u32, _u32]
    lib.rt_denoise_level_size.restype = C.c_int
    lib.rt_accum_denoise_multiscale.argtypes = [vp, C.POINTER(RtDenoise), C.POINTER(RtMultiscale), _f, _u8]
    lib.rt_accum_denoise_multiscale.restype = C.c_int
    lib.rt_debug_denoise_multiscale.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, _f, _f, _f, C.POINTER(RtDenoise), C.c_uint32, _f, C.c_uint32, _f, _f, _f]
    lib.rt_debug_denoise_multiscale.restype = C.c_int
    lib.rt_accum_add_adaptive.argtypes = [vp, C.c_uint32, C.POINTER(RtAdaptive), C.POINTER(RtStats)]
    lib.rt_accum_add_adaptive.restype = C.c_int
    lib.rt_accum_read_counts.argtypes = [vp, _u32, C.POINTER(RtAdaptiveInfo)]
    lib.rt_accum_read_counts.restype = C.c_int
    lib.rt_render_adaptive.argtypes = [vp, C.POINTER(RtCamera), C.POINTER(RtParams), C.POINTER(RtAdaptive), C.c_uint32, _f, _u8, _f, _u32,
                                       C.POINTER(RtNoise), C.POINTER(RtAdaptiveInfo), C.POINTER(RtStats)]
    lib.rt_render_adaptive.restype = C.c_int
    lib.rt_adaptive_check.argtypes = [C.POINTER(RtAdaptive), C.c_uint32]
    lib.rt_adaptive_check.restype = C.c_int
    lib.rt_adaptive_converged.argtypes = [C.POINTER(RtAdaptive), C.c_double, C.c_double, C.c_uint32]
    lib.rt_adaptive_converged.restype = C.c_int
    lib.rt_debug_accum_set_moments.argtypes = [vp, C.c_uint32, C.c_double, C.c_double]
    lib.rt_debug_accum_set_moments.restype = C.c_int
    lib.rt_accum_frame_id.argtypes = [C.POINTER(RtCamera), C.POINTER(RtParams)]
    lib.rt_accum_frame_id.restype = C.c_uint64
    lib.rt_accum_state_check.argtypes = [C.POINTER(RtAccumState)]
    lib.rt_accum_state_check.restype = C.c_int
    lib.rt_accum_export.argtypes = [vp, C.POINTER(RtAccumState)]
    lib.rt_accum_export.restype = C.c_int
    lib.rt_accum_import.argtypes = [vp, C.POINTER(RtAccumState)]
    lib.rt_accum_import.restype = C.c_int
    lib.rt_accum_merge.argtypes = [vp, C.POINTER(RtAccumState)]
    lib.rt_accum_merge.restype = C.c_int
    lib.rt_accum_track_halves.argtypes = [vp]
    lib.rt_accum_track_halves.restype = C.c_int
    lib.rt_accum_read_halves.argtypes = [vp, C.c_uint32, _f, _f]
    lib.rt_accum_read_halves.restype = C.c_int
    lib.rt_accum_denoise_halves.argtypes = [vp, C.POINTER(RtDenoise), _f, _u8, _f, C.POINTER(RtResidual)]
    lib.rt_accum_denoise_halves.restype = C.c_int
    lib.rt_accum_halves_check.argtypes = [C.POINTER(RtAccumHalves)]
    lib.rt_accum_halves_check.restype = C.c_int
    lib.rt_accum_export_halves.argtypes = [vp, C.POINTER(RtAccumHalves)]
    lib.rt_accum_export_halves.restype = C.c_int
    lib.rt_accum_import_halves.argtypes = [vp, C.POINTER(RtAccumHalves)]
    lib.rt_accum_import_halves.restype = C.c_int
    lib.rt_pixel_filter_check.argtypes = [C.POINTER(RtPixelFilter)]
    lib.rt_pixel_filter_check.restype = C.c_int
    lib.rt_pixel_filter_table.argtypes = [C.POINTER(RtPixelFilter), _f, _u32]
    lib.rt_pixel_filter_table.restype = C.c_int
    lib.rt_accum_track_filter.argtypes = [vp, C.POINTER(RtPixelFilter)]
    lib.rt_accum_track_filter.restype = C.c_int
    lib.rt_accum_read_filtered.argtypes = [vp, _f, _u8, _f]
    lib.rt_accum_read_filtered.restype = C.c_int
    lib.rt_accum_filter_check.argtypes = [C.POINTER(RtAccumFilter)]
    lib.rt_accum_filter_check.restype = C.c_int
    lib.rt_accum_export_filter.argtypes = [vp, C.POINTER(RtAccumFilter)]
    lib.rt_accum_export_filter.restype = C.c_int
    lib.rt_accum_import_filter.argtypes = [vp, C.POINTER(RtAccumFilter)]
    lib.rt_accum_import_filter.restype = C.c_int
    lib.rt_debug_filter_add.argtypes = [vp, C.c_uint32, C.c_uint32, _f]
    lib.rt_debug_filter_add.restype = C.c_int
    lib.rt_features_check.argtypes = [C.POINTER(RtFeatures)]
    lib.rt_features_check.restype = C.c_int
    lib.rt_accum_track_features.argtypes = [vp, C.POINTER(RtFeatures)]
    lib.rt_accum_track_features.restype = C.c_int
    lib.rt_accum_read_features.argtypes = [vp, _f, _f, _f, _f, _f]
    lib.rt_accum_read_features.restype = C.c_int
    lib.rt_accum_features_check.argtypes = [C.POINTER(RtAccumFeatures)]
    lib.rt_accum_features_check.restype = C.c_int
    lib.rt_accum_export_features.argtypes = [vp, C.POINTER(RtAccumFeatures)]
    lib.rt_accum_export_features.restype = C.c_int
    lib.rt_accum_import_features.argtypes = [vp, C.POINTER(RtAccumFeatures)]
    lib.rt_accum_import_features.restype = C.c_int
    lib.rt_debug_features_add.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.rt_debug_features_add.restype = C.c_int
    lib.rt_feature_guide_check.argtypes = [C.POINTER(RtFeatureGuide)]
    lib.rt_feature_guide_check.restype = C.c_int
    lib.rt_accum_denoise_features.argtypes = [vp, C.POINTER(RtDenoise), C.POINTER(RtFeatureGuide), _f, _u8]
    lib.rt_accum_denoise_features.restype = C.c_int
    lib.rt_debug_denoise_features.argtypes = [vp, C.c_uint32, C.c_uint32, _f, _f, _f, _f, _f, C.POINTER(RtDenoise), C.POINTER(RtFeatureGuide), _f]
    lib.rt_debug_denoise_features.restype = C.c_int
    lib.rt_select_check.argtypes = [C.POINTER(RtSelect)]
    lib.rt_select_check.restype = C.c_int
    lib.rt_accum_denoise_select.argtypes = [vp, C.POINTER(RtSelect), _f, _u8, _u8, _f, C.POINTER(RtSelectInfo)]
    lib.rt_accum_denoise_select.restype = C.c_int
    lib.rt_debug_denoise_select.argtypes = [vp, C.c_uint32, C.c_uint32, _f, _f, _f, _f, _u32, C.c_uint32, C.c_uint32, C.POINTER(RtSelect), _f, _u8, _f,
                                            C.POINTER(RtSelectInfo), C.c_uint32, _f, _f]
    lib.rt_debug_denoise_select.restype = C.c_int
    lib.rt_debug_select_chain.argtypes = [vp, C.c_uint32]
    lib.rt_debug_select_chain.restype = C.c_int
    lib.rt_accum_track_buckets.argtypes = [vp, C.c_uint32]
    lib.rt_accum_track_buckets.restype = C.c_int
    lib.rt_accum_read_robust.argtypes = [vp, C.POINTER(RtRobust), _f, _u8, _u8, C.POINTER(RtRobustInfo)]
    lib.rt_accum_read_robust.restype = C.c_int
    lib.rt_accum_denoise_robust.argtypes = [vp, C.POINTER(RtRobust), C.POINTER(RtDenoise), _f, _u8]
    lib.rt_accum_denoise_robust.restype = C.c_int
    lib.rt_accum_buckets_check.argtypes = [C.POINTER(RtAccumBuckets)]
    lib.rt_accum_buckets_check.restype = C.c_int
    lib.rt_accum_export_buckets.argtypes = [vp, C.POINTER(RtAccumBuckets)]
    lib.rt_accum_export_buckets.restype = C.c_int
    lib.rt_accum_import_buckets.argtypes = [vp, C.POINTER(RtAccumBuckets)]
    lib.rt_accum_import_buckets.restype = C.c_int
    lib.rt_set_display.argtypes = [vp, C.POINTER(RtDisplay)]
    lib.rt_set_display.restype = C.c_int
    lib.rt_display_info.argtypes = [vp, C.POINTER(RtDisplayInfo)]
    lib.rt_display_info.restype = C.c_int
    lib.rt_display_check.argtypes = [C.POINTER(RtDisplay)]
    lib.rt_display_check.restype = C.c_int
    lib.rt_debug_display.argtypes = [vp, C.c_uint32, C.c_uint32, _f, C.POINTER(RtDisplay), _u8, C.POINTER(RtDisplayInfo)]
    lib.rt_debug_display.restype = C.c_int
    lib.rt_set_glare.argtypes = [vp, C.POINTER(RtGlare)]
    lib.rt_set_glare.restype = C.c_int
    lib.rt_glare_check.argtypes = [C.POINTER(RtGlare)]
    lib.rt_glare_check.restype = C.c_int
    lib.rt_glare_info.argtypes = [vp, C.POINTER(RtGlareInfo)]
    lib.rt_glare_info.restype = C.c_int
    lib.rt_glare_image.argtypes = [vp, _f]
    lib.rt_glare_image.restype = C.c_int
    lib.rt_debug_glare.argtypes = [vp, C.c_uint32, C.c_uint32, _f, C.POINTER(RtGlare), C.POINTER(RtDisplay), _f, _u8, C.POINTER(RtGlareInfo)]
    lib.rt_debug_glare.restype = C.c_int
    lib.rt_debug_glare_chain.argtypes = [vp, C.c_uint32]
    lib.rt_debug_glare_chain.restype = C.c_int
    lib.rt_debug_planar_info.argtypes =[vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.rt_debug_planar_info.restype = C.c_int
    lib.rt_debug_planar_bounds.argtypes = [C.POINTER(RtQuads), C.c_float, vp, vp]
    lib.rt_debug_planar_bounds.restype = C.c_int
    lib.rt_debug_variant_tables.argtypes = [C.POINTER(RtVariantLedger)]
    lib.rt_debug_variant_tables.restype = C.c_int
    lib.rt_debug_variant_flag_names.argtypes = [C.c_uint32, C.c_char_p, C.c_uint32]
    lib.rt_debug_variant_flag_names.restype = C.c_int
    lib.rt_debug_launched_variants.argtypes = [vp, C.POINTER(RtVariantLedger), C.c_int]
    lib.rt_debug_launched_variants.restype = C.c_int
    lib.rt_host_alloc.argtypes = [C.c_size_t]
    lib.rt_host_alloc.restype = vp
    lib.rt_host_free.argtypes = [vp]
    lib.rt_host_free.restype = None
    lib.rt_debug_set_option.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.rt_debug_set_option.restype = C.c_int
    lib.rt_debug_get_option.argtypes = [vp, C.c_uint32, _u32]
    lib.rt_debug_get_option.restype = C.c_int
    lib.rt_debug_scene_info.argtypes = [vp, C.POINTER(RtSceneInfo)]
    lib.rt_debug_scene_info.restype = C.c_int
    lib.rt_debug_render_parts.argtypes = [vp, C.c_char_p, C.c_uint32]
    lib.rt_debug_render_parts.restype = C.c_int
    lib.rt_debug_grid_build.argtypes = [C.POINTER(RtFlatScene), C.c_uint32, C.c_uint32, C.c_float * 8, C.c_uint32 * 3, _u32, _u32, _u16, _u32,
                                        C.c_uint32 * 4, _u32]
    lib.rt_debug_grid_build.restype = C.c_int
    lib.rt_debug_world_bounds.argtypes = [C.POINTER(RtFlatScene), _f, _f, _f, _u32, _u32, _f, _f]
    lib.rt_debug_world_bounds.restype = C.c_int
    lib.rt_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    lib.rt_multi_create.restype = C.c_int
    lib.rt_multi_create_ex.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_uint32, C.POINTER(vp)]
    lib.rt_multi_create_ex.restype = C.c_int
    lib.rt_multi_destroy.argtypes = [vp]
    lib.rt_multi_destroy.restype = None
    lib.rt_multi_device_count.argtypes = [vp]
    lib.rt_multi_device_count.restype = C.c_int
    lib.rt_multi_last_error.argtypes = [vp]
    lib.rt_multi_last_error.restype = C.c_char_p
    lib.rt_multi_scene_upload.argtypes = [vp, C.POINTER(RtFlatScene)]
    lib.rt_multi_scene_upload.restype = C.c_int
    lib.rt_multi_render.argtypes = [vp, C.POINTER(RtCamera), C.POINTER(RtParams), _f, _u8, C.POINTER(RtStats)]
    lib.rt_multi_render.restype = C.c_int
    lib.rt_multi_accum_begin.argtypes = [vp, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_uint32, C.c_uint32, C.c_uint32]
    lib.rt_multi_accum_begin.restype = C.c_int
    lib.rt_multi_accum_add.argtypes = [vp, C.c_uint32, C.POINTER(RtStats)]
    lib.rt_multi_accum_add.restype = C.c_int
    lib.rt_multi_accum_add_adaptive.argtypes = [vp, C.c_uint32, C.POINTER(RtAdaptive), C.POINTER(RtStats)]
    lib.rt_multi_accum_add_adaptive.restype = C.c_int
    lib.rt_multi_accum_join.argtypes = [vp, C.POINTER(vp)]
    lib.rt_multi_accum_join.restype = C.c_int
    lib.rt_multi_accum_import.argtypes = [vp, C.POINTER(RtAccumState), C.POINTER(RtAccumHalves), C.POINTER(RtAccumBuckets)]
    lib.rt_multi_accum_import.restype = C.c_int
    lib.rt_multi_accum_end.argtypes = [vp]
    lib.rt_multi_accum_end.restype = C.c_int
    lib.rt_deinterleave_bands.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
    lib.rt_deinterleave_bands.restype = C.c_int
    _gpu_lib = lib
    return lib


def load_host_library():
    """Loads librtow_host.so (C++ mirror of the reference's construction API; no GPU code)."""
    global _host_lib
    if _host_lib is not None:
        return _host_lib
    if not os.path.exists(HOST_LIB_PATH):
        raise RuntimeError(f"{HOST_LIB_PATH} is missing: run __graft_entry__.build()")
    lib = C.CDLL(HOST_LIB_PATH)
    vp = C.c_void_p
    f3 = C.c_float * 3
    lib.rth_last_error.restype = C.c_char_p
    lib.rth_register_image.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, _f]
    lib.rth_register_image.restype = C.c_int
    lib.rth_rng_reseed.argtypes = [C.c_uint64]
    lib.rth_rng_reseed.restype = None
    lib.rth_scene_build.argtypes = [C.c_char_p, C.c_float, C.POINTER(vp)]
    lib.rth_scene_build.restype = C.c_int
    lib.rth_scene_new.argtypes = [C.POINTER(vp)]
    lib.rth_scene_new.restype = C.c_int
    lib.rth_tex_constant.argtypes = [vp, f3]
    lib.rth_tex_constant.restype = C.c_uint32
    lib.rth_tex_checker.argtypes = [vp, f3, f3]
    lib.rth_tex_checker.restype = C.c_uint32
    lib.rth_tex_perlin.argtypes = [vp, C.c_float]
    lib.rth_tex_perlin.restype = C.c_uint32
    lib.rth_tex_image.argtypes = [vp, C.c_char_p]
    lib.rth_tex_image.restype = C.c_uint32
    lib.rth_material.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, f3, C.c_float * 4]
    lib.rth_material.restype = C.c_uint32
    lib.rth_sphere.argtypes = [vp, f3, C.c_float, C.c_uint32, C.c_char_p]
    lib.rth_sphere.restype = C.c_uint32
    lib.rth_rect.argtypes = [vp, C.c_uint32, f3, f3, C.c_uint32]
    lib.rth_rect.restype = C.c_uint32
    lib.rth_gbox.argtypes = [vp, f3, f3, C.c_uint32]
    lib.rth_gbox.restype = C.c_uint32
    lib.rth_translate.argtypes = [vp, C.c_uint32, f3]
    lib.rth_translate.restype = C.c_uint32
    lib.rth_rotate_y.argtypes = [vp, C.c_uint32, C.c_float]
    lib.rth_rotate_y.restype = C.c_uint32
    lib.rth_constant_medium.argtypes = [vp, C.c_uint32, C.c_float, C.c_uint32]
    lib.rth_constant_medium.restype = C.c_uint32
    lib.rth_hitable_bbox.argtypes = [vp, C.c_uint32, C.c_float * 6]
    lib.rth_hitable_bbox.restype = C.c_int
    lib.rth_set_sky.argtypes = [vp, C.c_uint32, C.c_char_p]
    lib.rth_set_sky.restype = C.c_int
    lib.rth_set_camera.argtypes = [vp, f3, f3, f3, C.c_float, C.c_float]
    lib.rth_set_camera.restype = C.c_int
    lib.rth_scene_finish.argtypes = [vp, C.c_int]
    lib.rth_scene_finish.restype = C.c_int
    lib.rth_scene_flat.argtypes = [vp]
    lib.rth_scene_flat.restype = C.POINTER(RtFlatScene)
    lib.rth_scene_camera.argtypes = [vp, C.POINTER(RtCamera)]
    lib.rth_scene_camera.restype = C.c_int
    lib.rth_set_camera_lens.argtypes = [vp, f3, f3, f3, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.rth_set_camera_lens.restype = C.c_int
    lib.rth_scene_lens.argtypes = [vp, C.POINTER(RtLens)]
    lib.rth_scene_lens.restype = C.c_int
    lib.rth_moving_sphere.argtypes = [vp, f3, f3, C.c_float, C.c_uint32, C.c_char_p]
    lib.rth_moving_sphere.restype = C.c_uint32
    lib.rth_set_camera_shutter.argtypes = [vp, C.c_float, C.c_float]
    lib.rth_set_camera_shutter.restype = C.c_int
    lib.rth_scene_motion.argtypes = [vp, C.POINTER(RtMotion)]
    lib.rth_scene_motion.restype = C.c_int
    lib.rth_quad.argtypes = [vp, f3, f3, f3, C.c_uint32]
    lib.rth_quad.restype = C.c_uint32
    lib.rth_triangle.argtypes = [vp, f3, f3, f3, C.c_uint32]
    lib.rth_triangle.restype = C.c_uint32
    lib.rth_scene_quads.argtypes = [vp, C.POINTER(RtQuads)]
    lib.rth_scene_quads.restype = C.c_int
    lib.rth_scene_lights.argtypes = [vp, C.POINTER(RtLights), C.POINTER(C.c_uint32)]
    lib.rth_scene_lights.restype = C.c_int
    lib.rth_scene_sphere_name.argtypes = [vp, C.c_uint32]
    lib.rth_scene_sphere_name.restype = C.c_char_p
    lib.rth_scene_free.argtypes = [vp]
    lib.rth_png_write.argtypes = [C.c_char_p, _u8, C.c_uint32, C.c_uint32]
    lib.rth_png_write.restype = C.c_int
    lib.rth_output_file_name.argtypes = [C.c_int64, C.c_char_p, C.c_uint32]
    lib.rth_output_file_name.restype = C.c_int
    lib.rth_scene_free.restype = None
    _host_lib = lib
    return lib
