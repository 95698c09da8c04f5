"""MI355X-native wavefront path tracer behind the construction API of
zhouhang95/ray_tracing_in_one_weekend."""
from . import _ffi
from ._ffi import (GpuLibraryMissing, RtAccumBuckets, RtAccumHalves, RtAccumState, RtAdaptive, RtAdaptiveInfo, RtCamera, RtDenoise, RtDisplay, RtDisplayInfo, RtFlatScene, RtGlare, RtGlareInfo, RtLens, RtLights, RtMotion, RtMultiscale, RtNoise, RtParams, RtQuads, RtResidual, RtRobust, RtRobustInfo, RtStats)
from .api import AccumBuckets, AccumHalves, AccumState, MultiRenderer, Renderer, RtError, Scene, accum_frame_id, adaptive_check, adaptive_converged, denoise_level_size, display_check, glare_check, grid_build, make_adaptive, make_display, make_glare, make_lights, make_motion, make_params, make_quads, planar_bounds, output_file_name, save_png, variant_flag_names, variant_tables, world_bounds
from .images import decode_rgb32f, register_default_images, register_image

__all__ = ["AccumState", "AccumHalves", "AccumBuckets", "RtAccumBuckets", "RtRobust", "RtRobustInfo", "RtAccumHalves", "RtResidual", "RtAccumState", "accum_frame_id", "make_adaptive", "adaptive_check", "adaptive_converged", "RtAdaptive", "RtAdaptiveInfo", "Renderer", "MultiRenderer", "Scene", "RtError", "make_params", "make_motion", "make_quads", "RtQuads", "make_lights", "RtLights", "RtCamera", "RtFlatScene", "RtLens", "RtMotion", "RtParams", "RtStats", "RtNoise", "RtDenoise", "RtMultiscale", "denoise_level_size", "RtDisplay", "RtDisplayInfo", "make_display", "display_check", "RtGlare", "RtGlareInfo", "make_glare", "glare_check",
           "GpuLibraryMissing", "variant_tables", "variant_flag_names", "save_png", "output_file_name", "register_default_images", "register_image", "decode_rgb32f", "_ffi"]
