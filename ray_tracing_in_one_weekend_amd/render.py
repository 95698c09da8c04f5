"""The reference's `main()` (main.rs:62-129) on the accelerated path:

    python -m ray_tracing_in_one_weekend_amd.render --scene sphere_scene --nx 1920 --ny 1080 --spp 256

builds the scene with the host mirror of demo_scene.rs, renders it on the GPU, prints progress, saves partial
images while rendering and the final PNG under the reference's time-stamped name.  Defaults are the constants in
main.rs: 800x400, aspect nx/ny, 128 spp, MAX_DEPTH 50, seed base 95, test_sphere.
There is no CPU fallback: without librtow_mi355x.so and a GPU this exits with the library's error."""
import argparse
import os
import sys
import time

import numpy as np

from . import make_feature_guide, feature_guide_check, AccumBuckets, AccumFeatures, AccumFilter, AccumState, features_check, make_pixel_filter, pixel_filter_check, MultiRenderer, Renderer, RtError, Scene, display_check, glare_check, make_display, make_glare, make_params, make_select, select_check, output_file_name, register_default_images, save_png
from . import _ffi
from .images import write_pfm

# --robust without --buckets: of 5, 9 and 15 by the rule of RT_DENOISE_DEFAULT_STRENGTH on rendered frames (DESIGN.md "Sample buckets")
DEFAULT_BUCKETS = 5
DEFAULT_FEATURE_STRIDE = 4  # (11 % of a 64-sample add of sphere_scene at 1920 x 1080, 2.7 % of cornell_box: DESIGN.md 4.18)

SCENES = ("test_sphere", "sphere_scene", "moving_sphere_scene", "quads_scene", "mesh_scene", "simple_light_scene", "cornell_box", "final_scene", "earth_env_scene",
          "pbr_sweep_scene")


class _MultiAccum:
    """--devices: a MultiRenderer behind the Renderer calls the functions below make.  What builds the accumulation goes to every device
    (rt_multi_accum_*: tracking is asked for at begin and an import takes the state and its buckets in one call, so a later accum_track_*
    or accum_import_buckets begins again with what is known by then; nothing has been sampled at that point).  Everything that reads goes
    to the joined context, joined again after every add."""

    def __init__(self, devices, copy_gather):
        self._mr = MultiRenderer(devices, copy_gather=copy_gather)
        self._begin = self._state = self._joined = None
        self._track = dict(channels=False, halves=False, buckets=0)
        for name in ("upload", "set_lens", "set_motion", "set_quads", "set_lights", "render"):
            setattr(self, name, getattr(self._mr, name))

    def _rebegin(self):
        self._mr.accum_begin(*self._begin, **self._track)
        self._joined = None

    def accum_begin(self, camera, params, first_sample=0):
        self._begin, self._state = (camera, params, first_sample), None
        self._track = dict(channels=False, halves=False, buckets=0)
        self._rebegin()

    def accum_track_channels(self):
        self._track["channels"] = True
        self._rebegin()

    def accum_track_halves(self):
        self._track["halves"] = True
        self._rebegin()

    def accum_track_buckets(self, M):
        self._track["buckets"] = int(M)
        self._rebegin()

    def accum_import(self, state):
        self._state = state
        self._mr.accum_import(state)
        self._joined = None

    def accum_import_buckets(self, buckets):
        self._rebegin()
        self._mr.accum_import(self._state, buckets=buckets)

    def accum_add(self, n):
        self._joined = None
        return self._mr.accum_add(n)

    def accum_add_adaptive(self, n, tolerance, luminance_floor=0.01, min_samples=16):
        self._joined = None
        return self._mr.accum_add_adaptive(n, tolerance, luminance_floor, min_samples)

    def accum_end(self):
        self._joined = None
        self._mr.accum_end()

    def __getattr__(self, name):  # every reading call: accum_read, accum_counts, accum_denoise*, accum_robust, accum_export*
        if not name.startswith("accum_"):
            raise AttributeError(name)
        if self._joined is None:
            self._joined = self._mr.accum_join()
        return getattr(self._joined, name)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="test_sphere", choices=SCENES)          # main.rs:74
    ap.add_argument("--nx", type=int, default=800)                             # main.rs:66
    ap.add_argument("--ny", type=int, default=400)                             # main.rs:67
    ap.add_argument("--spp", type=int, default=128)                            # main.rs:64
    ap.add_argument("--max-depth", type=int, default=50)                       # main.rs:36
    ap.add_argument("--seed", type=int, default=95)                            # main.rs:82
    ap.add_argument("--russian-roulette", action="store_true", help="main.rs:49-53 (commented out there)")
    ap.add_argument("--preview-every", type=int, default=0, metavar="SPP",
                    help="save a partial image every SPP samples (main.rs:114-123 saves every 10 columns)")
    ap.add_argument("--out", default=None, help="default: the reference's <local time>.png (main.rs:110-112)")
    ap.add_argument("--aperture", type=float, default=0.0,
                    help="thin-lens aperture of the book's Camera::new (chapter 13; the cover: 0.1); 0 = pinhole")
    ap.add_argument("--focus-dist", type=float, default=10.0, help="distance of the plane of focus (with --aperture)")
    ap.add_argument("--shutter", type=float, nargs=2, default=None, metavar=("OPEN", "CLOSE"),
                    help="shutter interval within [0, 1] for a scene with moving spheres (default: the scene camera's, [0, 1])")
    ap.add_argument("--light-sampling", action="store_true",
                    help="aim half of the diffuse bounces at the scene's emissive rectangles and quads (Scene.lights): same mean, less noise")
    ap.add_argument("--noise-target", type=float, default=None, metavar="X",
                    help="render to a quality: add samples until the frame's noise (RMS standard error of the pixels' mean luminance over "
                         "the mean luminance, RtNoise.noise) is at most X; --spp is then the maximum")
    ap.add_argument("--spp-step", type=int, default=64, metavar="N",
                    help="samples per pixel between two looks at the noise (with --noise-target); a step costs about 2 ms beyond its samples at "
                         "1920 x 1080 (DESIGN.md \"Accumulation and noise\"): 64 keeps that below a fifth")
    ap.add_argument("--adaptive-tolerance", type=float, default=None, metavar="T",
                    help="adaptive sampling: in steps of --spp-step, a pixel stops once the standard error of its mean luminance is at most "
                         "T x max(mean luminance, --luminance-floor); the others go on until --spp, the maximum (rt_render_adaptive)")
    ap.add_argument("--min-spp", type=int, default=16, metavar="N", help="with --adaptive-tolerance: no pixel stops on fewer samples (>= 2)")
    ap.add_argument("--luminance-floor", type=float, default=0.01, metavar="L",
                    help="with --adaptive-tolerance: below this mean luminance the error is measured against L (a floor near the frame's "
                         "mean luminance makes the criterion an absolute one for the darker pixels)")
    ap.add_argument("--counts-out", default=None, metavar="FILE",
                    help="with --adaptive-tolerance: the per-pixel sample counts as a grey PNG, white = --spp")
    ap.add_argument("--denoise", action="store_true",
                    help="save the frame through the variance-guided non-local-means filter (rt_accum_denoise); needs --spp >= 2")
    ap.add_argument("--denoise-radius", type=int, default=5, metavar="R", help="search window radius, 1..%d" % _ffi.DENOISE_MAX_RADIUS)
    ap.add_argument("--denoise-patch", type=int, default=1, metavar="F", help="patch radius, 0..%d" % _ffi.DENOISE_MAX_PATCH)
    ap.add_argument("--denoise-strength", type=float, default=None, metavar="K",
                    help="how many standard errors two pixels may differ and still be averaged (default %g)" % _ffi.DENOISE_DEFAULT_STRENGTH)
    ap.add_argument("--denoise-guide", choices=("luminance", "channels", "halves", "features"), default="luminance",
                    help="what the filter measures distance on: the mean luminance and its variance (rt_accum_denoise), the three channels and "
                         "theirs (rt_accum_denoise_channels: 48 B per pixel more, keeps edges between colours of equal luminance), or, per half "
                         "of the samples, the luminance of the OTHER half (rt_accum_denoise_halves: 56 B per pixel more, default strength %g, "
                         "reports the variance left in the filtered frame)" % _ffi.DENOISE_HALVES_DEFAULT_STRENGTH)
    ap.add_argument("--denoise-levels", type=int, default=None, metavar="L",
                    help="with --denoise and --denoise-guide luminance or channels: filter a 2x pyramid of L levels, 1..%d, each coarser level "
                         "replacing the low frequencies of the finer one (rt_accum_denoise_multiscale); 1 is the single-scale filter"
                         % _ffi.DENOISE_MAX_LEVELS)
    ap.add_argument("--denoise-select", default=None, metavar="K0,K1[,K2[,K3]]",
                    help="with --denoise --denoise-guide halves: 2..%d strictly increasing candidate strengths; the cross filter runs at each, its "
                         "error is estimated per pixel against the other half, and every pixel takes the candidate with the smallest "
                         "(rt_accum_denoise_select; the library's candidates are %s).  Prints the frame-wide best candidate and the estimated "
                         "error of each" % (_ffi.SELECT_MAX, ",".join("%g" % k for k in _ffi.SELECT_DEFAULT_STRENGTHS)))
    ap.add_argument("--select-error-radius", type=int, default=0, metavar="S", help="radius of the window the error estimate is summed over, 0..%d" % _ffi.SELECT_MAX_WINDOW)
    ap.add_argument("--select-blend-radius", type=int, default=1, metavar="T", help="radius of the window the choice is blended over, 0..%d" % _ffi.SELECT_MAX_WINDOW)
    ap.add_argument("--select-map-out", default=None, metavar="FILE",
                    help="with --denoise-select: write the index map (the candidate every pixel chose, u8) and the error map (est, f32) to FILE, an "
                         ".npz with `index`, `est` and `strengths`, rows as the saved image has them (row 0 on top)")
    ap.add_argument("--residual-target", type=float, default=None, metavar="X",
                    help="render until the DENOISED frame is clean: samples in steps of --spp-step, the cross filter of --denoise-guide halves "
                         "after each, until its residual_noise <= X or --spp are done.  The figure is the variance half of the filtered "
                         "frame's relative error, a lower bound: blur is not in it")
    ap.add_argument("--checkpoint", default=None, metavar="FILE",
                    help="drive the samples in steps of --spp-step and write the accumulation's state (AccumState, an .npz) to FILE after every "
                         "--checkpoint-every-th step and at the end, each time through a temporary file: a killed render leaves a whole checkpoint")
    ap.add_argument("--checkpoint-every", type=int, default=64, metavar="K",
                    help="with --checkpoint: write after every K-th step, and always at the end.  A checkpoint of a 1920 x 1080 frame is 58 MB "
                         "and costs 54 ms (158 MB and 143 ms with channel moments), four to eleven 64-sample steps of sphere_scene: every 64th "
                         "step keeps that at 6 to 17 %% and puts at most a second of rendering at risk (DESIGN.md \"Accumulation state\")")
    ap.add_argument("--resume", default=None, metavar="FILE",
                    help="begin from the state in FILE (same scene, frame and flags) and go on until the stopping rule of this command line is "
                         "met: --spp samples, --noise-target or --adaptive-tolerance; the image is, bit for bit, the uninterrupted render's")
    ap.add_argument("--first-sample", type=int, default=None, metavar="S",
                    help="render the sample window [S, S + spp) of the frame instead of [0, spp); with --checkpoint its state is the product, "
                         "for another process to --merge")
    ap.add_argument("--merge", nargs="+", default=None, metavar="FILE",
                    help="states of further sample windows, merged in the order given behind what was rendered or resumed, before the image is "
                         "written; each must begin where the samples so far end (uniform states only)")
    ap.add_argument("--buckets", type=int, default=None, metavar="M",
                    help="keep the samples of every pixel in M buckets by sample index (3..%d, 12 M bytes per pixel more; default %d with "
                         "--robust): what --robust and --firefly-map read, carried by --checkpoint in FILE.buckets.npz, which --resume picks up with its own M" % (_ffi.BUCKETS_MAX, DEFAULT_BUCKETS))
    ap.add_argument("--robust", default=None, metavar="{gini,median,trim:N}",
                    help="write the robust read-out instead of the plain mean (rt_accum_read_robust): the trimmed mean of the sorted bucket means, "
                         "the trim chosen by their Gini coefficient (gini), the median (median) or N per side (trim:N).  It tames fireflies and "
                         "keeps a NaN sample out; it is BIASED — the line printed with the image says how much energy it removed.  With "
                         "--denoise: the luminance-guided filter on the robust colours (rt_accum_denoise_robust)")
    ap.add_argument("--firefly-map", default=None, metavar="PATH",
                    help="with --robust: the number of bucket means trimmed per side, per pixel the largest of its three channels, as a grey PNG "
                         "(white = the most possible, (M - 1) / 2)")
    ap.add_argument("--exposure", type=float, default=None, metavar="E",
                    help="display transform (rt_set_display): multiply the linear image by E before the 8-bit step; with --auto-exposure the "
                         "level the measured luminance maps to instead (default 0.18 for key, 0.8 for percentile)")
    ap.add_argument("--auto-exposure", choices=("key", "percentile"), default=None,
                    help="measure the exposure from the frame on the device: key maps the log-average luminance of the lit pixels onto "
                         "--exposure, percentile the --percentile quantile of their luminance histogram")
    ap.add_argument("--percentile", type=float, default=0.99, metavar="Q", help="with --auto-exposure percentile: the quantile, in (0, 1]")
    ap.add_argument("--tone", choices=("clamp", "reinhard", "aces"), default=None,
                    help="tone curve: clamp (the reference's: radiance above 1 saturates), extended Reinhard on the luminance (--white), or the "
                         "ACES filmic fit per channel")
    ap.add_argument("--white", type=float, default=float("inf"), metavar="W", help="with --tone reinhard: the luminance that maps to 1 (default: none)")
    ap.add_argument("--srgb", action="store_true", help="the sRGB transfer function instead of the reference's gamma 2: what a PNG viewer assumes")
    ap.add_argument("--dither", action="store_true",
                    help="8 x 8 ordered dither of the 8-bit step: a denoised gradient keeps no bands")
    ap.add_argument("--hdr-out", default=None, metavar="FILE.pfm",
                    help="also write the linear f32 image as a PFM (a plain render only: not with --noise-target, --adaptive-tolerance, "
                         "--denoise, --checkpoint and their kin)")
    ap.add_argument("--glare", type=float, default=None, metavar="A",
                    help="glare (rt_set_glare): the share A in [0, 1] of every pixel's light that a 2x image pyramid spreads over its "
                         "neighbourhood before the 8-bit step, so that a bright light looks bright; the frame's energy is kept")
    ap.add_argument("--glare-levels", type=int, default=_ffi.GLARE_DEFAULT_LEVELS, metavar="L", help="with --glare: levels of the pyramid, 1..8; the glow is about 2^L pixels wide")
    ap.add_argument("--glare-spread", type=float, default=_ffi.GLARE_DEFAULT_SPREAD, metavar="S",
                    help="with --glare: the weight of each coarser level relative to the one below, in (0, 1]; 1 is the widest glow")
    ap.add_argument("--glare-threshold", type=float, default=0.0, metavar="T", help="with --glare: only the luminance above T glows (0: all of it)")
    ap.add_argument("--glare-out", default=None, metavar="FILE.pfm",
                    help="with --glare: also write the glared linear f32 image as a PFM (a plain render only, as --hdr-out, which stays the un-glared frame)")
    ap.add_argument("--pixel-filter", choices=("box", "tent", "gaussian", "mitchell", "blackman-harris"), default=None,
                    help="reconstruct every pixel from its own samples AND its neighbours', weighted by this filter at their sub-pixel distance "
                         "(rt_accum_track_filter: 16 B per pixel more), instead of the reference's box over the pixel; the image written is the "
                         "filtered one, and --checkpoint carries the plane in FILE.filter.npz, which --resume picks up.  Does not combine with "
                         "--denoise, --devices or --merge")
    ap.add_argument("--filter-radius", type=float, default=None, metavar="R",
                    help="with --pixel-filter: the radius in pixels, %g..%g (default: box 0.5, tent 1, gaussian 1.5, mitchell 2, blackman-harris 1.5)"
                         % (_ffi.FILTER_MIN_RADIUS, _ffi.FILTER_MAX_RADIUS))
    ap.add_argument("--filter-param", type=float, nargs="+", default=None, metavar="P",
                    help="with --pixel-filter gaussian: sigma (default 0.5); with mitchell: B C (default 1/3 1/3)")
    ap.add_argument("--features", action="store_true",
                    help="also keep the first-hit features of the accumulation — albedo, shading normal and depth of the primary hit, with their "
                         "second moments (rt_accum_track_features: 64 B per pixel more) —, recomputed by a kernel of its own; the image is "
                         "unchanged, and --checkpoint carries the records in FILE.features.npz, which --resume picks up.  Does not combine with "
                         "--devices and --merge (the library refuses features on shards and in a merge), nor with --denoise-guide halves, "
                         "--residual-target and --preview-every: the library would track both, but those three render through loops of "
                         "this program that read no records and write no FILE.features.npz, so the option would cost time for nothing")
    ap.add_argument("--feature-stride", type=int, default=None, metavar="K",
                    help="with --features: every K-th sample, by absolute index, takes a feature sample, %d..%d (default %d)"
                         % (_ffi.FEATURES_MIN_STRIDE, _ffi.FEATURES_MAX_STRIDE, DEFAULT_FEATURE_STRIDE))
    ap.add_argument("--feature-k", type=float, default=None, metavar="K",
                    help="with --denoise --denoise-guide features (which needs --features): the strength of the three feature distances of "
                         "rt_accum_denoise_features (default %g, the 2013 paper's; smaller keeps more feature edges)" % _ffi.FEATURE_GUIDE_DEFAULT_K)
    ap.add_argument("--demodulate", action="store_true",
                    help="with --denoise-guide features: filter the colour divided by the albedo and multiply the albedo back (keeps texture detail)")
    ap.add_argument("--albedo-out", default=None, metavar="FILE.pfm", help="with --features: write the mean albedo as a PFM")
    ap.add_argument("--normal-out", default=None, metavar="FILE.pfm", help="with --features: write the mean shading normal as a PFM")
    ap.add_argument("--depth-out", default=None, metavar="FILE.pfm", help="with --features: write the mean depth of the hits, in all three channels, as a PFM")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--devices", default=None, metavar="ID,ID,...",
                    help="render on these devices of the node at once (rt_multi_*): every device takes row-interleaved bands of the frame; the "
                         "progressive options (--noise-target, --adaptive-tolerance, --denoise, --buckets, --robust, --checkpoint, --resume) add "
                         "on every device and read the frame out of the joined accumulation on the first (rt_multi_accum_join), bit for bit "
                         "what --device renders.  A checkpoint is a whole-frame state: it resumes on any number of devices, or on one with --device")
    ap.add_argument("--copy-gather", action="store_true",
                    help="with --devices: device-to-device copies instead of RCCL (RT_MULTI_COPY_GATHER); an id may then be listed several times, "
                         "so --devices 0,0 runs two contexts on one GPU")
    a = ap.parse_args(argv)
    multi = a.devices is not None
    if multi:
        try:
            a.devices = [int(d) for d in a.devices.split(",")]
        except ValueError:
            ap.error("--devices takes a comma-separated list of device ids")
        if a.preview_every or a.merge or a.residual_target is not None:
            ap.error("--devices does not combine with --preview-every, --merge or --residual-target")
    elif a.copy_gather:
        ap.error("--copy-gather needs --devices")
    ny = a.ny
    aspect = a.nx / ny                                                        # main.rs:68
    file_name = a.out or output_file_name()

    t0 = time.perf_counter()                                                  # EZTimer, main.rs:70
    register_default_images()
    scene = Scene.build(a.scene, aspect)
    rend = _MultiAccum(a.devices, a.copy_gather) if multi else Renderer(a.device)
    rend.upload(scene)
    if a.aperture:
        rend.set_lens((a.aperture / 2.0, a.focus_dist))
    motion = scene.motion  # a scene's moving spheres are applied by themselves
    if motion.n_moving:
        if a.shutter:
            motion.shutter_open, motion.shutter_close = a.shutter
        rend.set_motion(motion)
    quads = scene.quads  # and so are its quads and triangles
    if quads.n:
        rend.set_quads(quads)
    if a.light_sampling:
        rend.set_lights(scene.lights)  # (a moving scene refuses it: RT_ERR_UNSUPPORTED)
    flags = _ffi.FLAG_RUSSIAN_ROULETTE if a.russian_roulette else 0
    # the display transform: set once on the context, it stands behind every 8-bit read-out of an accumulation below
    display = None
    if a.exposure is not None or a.auto_exposure or a.tone or a.srgb or a.dither:
        exposure = a.exposure if a.exposure is not None else {None: 1.0, "key": 0.18, "percentile": 0.8}[a.auto_exposure]
        display = make_display(exposure, auto=a.auto_exposure, percentile=a.percentile, curve=a.tone or "clamp", white=a.white,
                               transfer="srgb" if a.srgb else "gamma2", dither="bayer8" if a.dither else "none")
        if not display_check(display):
            ap.error("--exposure must be finite and > 0, --percentile in (0, 1], --white > 0")
        if multi or a.preview_every:
            ap.error("--exposure, --auto-exposure, --tone, --srgb and --dither do not combine with --devices or --preview-every "
                     "(rt_multi_* and the progress preview keep the reference quantisation)")
        rend.set_display(display)
    # the glare: set once on the context as well, in front of that display (or of the reference quantisation)
    glare = None
    if a.glare is not None:
        glare = make_glare(a.glare, a.glare_spread, a.glare_threshold, a.glare_levels if 0 <= a.glare_levels < 2 ** 32 else 0)
        if not glare_check(glare):
            ap.error("--glare takes 0..1, --glare-levels 1..%d, --glare-spread a value in (0, 1], --glare-threshold a finite value >= 0" % _ffi.GLARE_MAX_LEVELS)
        if multi or a.preview_every:
            ap.error("--glare does not combine with --devices or --preview-every (rt_multi_* and the progress preview keep the reference quantisation)")
        rend.set_glare(glare)
    elif a.glare_out:
        ap.error("--glare-out needs --glare")
    halves = a.residual_target is not None or (a.denoise and a.denoise_guide == "halves")
    a.filter = None
    if a.pixel_filter is None and (a.filter_radius is not None or a.filter_param is not None):
        ap.error("--filter-radius and --filter-param need --pixel-filter")
    if a.pixel_filter is not None:
        if a.denoise:
            ap.error("--pixel-filter does not combine with --denoise: the pixels of a filtered image are correlated, and the variance guides of "
                     "the denoisers do not describe it")
        if multi:
            ap.error("--pixel-filter does not combine with --devices: a row-interleaved shard has no neighbourhoods (rt_accum_track_filter)")
        if a.merge:
            ap.error("--pixel-filter does not combine with --merge: a merge of filter planes is not covered (rt_accum_merge)")
        if a.preview_every or a.robust is not None or a.residual_target is not None or a.hdr_out or a.glare_out:
            ap.error("--pixel-filter does not combine with --preview-every, --robust, --residual-target, --hdr-out or --glare-out")
        p = a.filter_param or []
        want = {"gaussian": 1, "mitchell": 2}.get(a.pixel_filter, 0)
        if p and len(p) != want:
            ap.error("--filter-param takes sigma with --pixel-filter gaussian, B C with mitchell, and nothing with the other filters")
        a.filter = make_pixel_filter(a.pixel_filter, a.filter_radius, sigma=p[0] if want == 1 and p else None, B=p[0] if want == 2 and p else None,
                                     C=p[1] if want == 2 and p else None)
        if not pixel_filter_check(a.filter):
            ap.error("--pixel-filter: --filter-radius takes %g..%g, sigma must be > 0, every value finite" % (_ffi.FILTER_MIN_RADIUS, _ffi.FILTER_MAX_RADIUS))
    if not a.features and (a.feature_stride is not None or a.albedo_out or a.normal_out or a.depth_out):
        ap.error("--feature-stride, --albedo-out, --normal-out and --depth-out need --features")
    if a.features:
        if multi or a.merge or halves or a.preview_every:
            ap.error("--features does not combine with --devices and --merge (rt_accum_track_features refuses shards, rt_accum_merge tracked "
                     "features), nor with --denoise-guide halves, --residual-target and --preview-every (their loops here read no records)")
        a.feature_stride = DEFAULT_FEATURE_STRIDE if a.feature_stride is None else a.feature_stride
        if not features_check(a.feature_stride):
            ap.error("--feature-stride takes %d..%d" % (_ffi.FEATURES_MIN_STRIDE, _ffi.FEATURES_MAX_STRIDE))
    a.feature_guide = None
    if a.denoise_guide == "features":
        if not (a.denoise and a.features) or a.robust is not None or a.denoise_levels is not None:
            ap.error("--denoise-guide features needs --denoise and --features, without --robust and --denoise-levels")
        a.feature_guide = make_feature_guide(k=_ffi.FEATURE_GUIDE_DEFAULT_K if a.feature_k is None else a.feature_k, demodulate=a.demodulate)
        if not feature_guide_check(a.feature_guide):
            ap.error("--feature-k must be finite and > 0")
    elif a.feature_k is not None or a.demodulate:
        ap.error("--feature-k and --demodulate need --denoise-guide features")
    if a.denoise_levels is not None:
        if not a.denoise or a.denoise_guide == "halves" or a.residual_target is not None:
            ap.error("--denoise-levels needs --denoise with --denoise-guide luminance or channels")
        if not 1 <= a.denoise_levels <= _ffi.DENOISE_MAX_LEVELS:
            ap.error("--denoise-levels takes 1..%d" % _ffi.DENOISE_MAX_LEVELS)
        if a.robust is not None:
            ap.error("--denoise-levels does not combine with --robust")
    a.robust_mode = None
    if a.robust is not None:
        kind, _, n = a.robust.partition(":")
        if kind not in ("gini", "median", "trim") or (kind == "trim") != bool(n) or (n and not n.isdigit()):
            ap.error("--robust takes gini, median or trim:N")
        a.robust_mode = (kind, int(n or 0))
    a.want_buckets = a.buckets is not None or a.robust_mode is not None  # (--buckets None with --robust: the resumed file's M, else the default)
    if a.want_buckets:
        if a.buckets is not None and not 3 <= a.buckets <= _ffi.BUCKETS_MAX:
            ap.error("--buckets takes 3..%d" % _ffi.BUCKETS_MAX)
        if halves or a.merge or a.preview_every:
            ap.error("--buckets and --robust do not combine with --denoise-guide halves, --residual-target, --merge or --preview-every")
        if a.robust_mode and a.denoise and a.denoise_guide != "luminance":
            ap.error("--denoise --robust filters with the luminance guide only")
    if a.firefly_map and not a.robust_mode:
        ap.error("--firefly-map needs --robust")
    if a.denoise_select is not None or a.select_map_out:
        if not (a.denoise and a.denoise_guide == "halves") or a.residual_target is not None or a.denoise_strength is not None:
            ap.error("--denoise-select needs --denoise --denoise-guide halves, without --residual-target and --denoise-strength")
        if a.denoise_select is None:
            ap.error("--select-map-out needs --denoise-select")
        try:
            a.select = make_select([float(k) for k in a.denoise_select.split(",")], a.denoise_radius, a.denoise_patch, a.select_error_radius, a.select_blend_radius)
        except ValueError as e:
            ap.error("--denoise-select: %s" % e)
        if not select_check(a.select):
            ap.error("--denoise-select takes 2..%d finite strengths > 0 in strictly increasing order, --select-error-radius and --select-blend-radius 0..%d"
                     % (_ffi.SELECT_MAX, _ffi.SELECT_MAX_WINDOW))
    if halves:
        if a.hdr_out or a.glare_out:
            ap.error("--hdr-out and --glare-out write the image of a plain render: they do not combine with the progressive options")
        if a.checkpoint or a.resume or a.merge:
            ap.error("--denoise-guide halves and --residual-target do not combine with --checkpoint, --resume or --merge")
        if a.first_sample is not None or a.adaptive_tolerance is not None or a.noise_target is not None or a.preview_every:
            ap.error("--denoise-guide halves and --residual-target do not combine with --first-sample, --adaptive-tolerance, --noise-target or --preview-every")
        if a.denoise_guide not in ("luminance", "halves") or (a.residual_target is not None and not a.residual_target >= 0.0):
            ap.error("--residual-target needs --denoise-guide halves (or none) and a value >= 0")
        if a.spp < 4:
            ap.error("the cross filter needs --spp >= 4: two samples per half")
        return render_halves(a, rend, scene, flags, file_name, t0)
    progressive = a.adaptive_tolerance is not None or a.noise_target is not None or a.denoise
    if (a.hdr_out or a.glare_out) and (progressive or halves or a.checkpoint or a.resume or a.merge or a.first_sample is not None or a.want_buckets):
        ap.error("--hdr-out and --glare-out write the image of a plain render: they do not combine with the progressive options")
    if a.checkpoint or a.resume or a.merge or a.first_sample is not None or a.want_buckets or a.filter is not None or a.features or (multi and progressive):
        if a.preview_every:
            ap.error("--checkpoint, --resume, --first-sample and --merge do not combine with --preview-every")
        if a.adaptive_tolerance is not None and a.noise_target is not None:
            ap.error("--adaptive-tolerance does not combine with --noise-target")
        if a.checkpoint_every < 1 or a.spp_step < 1:
            ap.error("--checkpoint-every and --spp-step must be >= 1")
        return render_with_state(a, rend, scene, flags, file_name, t0)
    if a.adaptive_tolerance is not None:
        if a.noise_target is not None or a.denoise or a.preview_every:
            ap.error("--adaptive-tolerance does not combine with --noise-target, --denoise or --preview-every")
        return render_adaptive(a, rend, scene, flags, file_name, t0)
    if a.noise_target is not None:
        return render_to_noise(a, rend, scene, flags, file_name, t0)
    if a.denoise:
        return render_denoised(a, rend, scene, flags, file_name, t0)
    params = make_params(a.nx, ny, a.spp, max_depth=a.max_depth, seed=a.seed, spp_slice=a.preview_every, flags=flags)
    if display is not None or glare is not None:  # through an accumulation: begin / add / read; its f32 image is rt_render's, bit for bit
        rend.accum_begin(scene.camera, params)
        st = rend.accum_add(a.spp)
        img, rgb8, _, _ = rend.accum_read(want_rgb8=True)
        rend.accum_end()
        print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)
        save_png(file_name, rgb8)
        if a.hdr_out:
            write_pfm(a.hdr_out, img)
        if a.glare_out:
            write_pfm(a.glare_out, rend.glare_image(a.nx, ny))
        notes = ""
        if glare is not None:
            g = rend.glare_info()
            notes += f"; glare: {g.levels} levels, the coarsest {g.coarse_nx}x{g.coarse_rows}"
        if display is not None:
            info = rend.display_info()
            notes += (f"; display: exposure {info.exposure:.4g}, {info.n_saturated} of {rgb8.size} values at 255, "
                      f"{info.n_non_finite} non-finite pixels")
        print(f"{file_name}: {a.nx}x{ny}, {a.spp} spp, {st.n_rays} rays, {st.n_rays / st.seconds_device / 1e6:.0f} Mray/s on the device{notes}", file=sys.stderr)
        return 0
    if a.preview_every:
        def progress(done, total, rgb8):
            print(f"{done}/{total}", file=sys.stderr)                          # main.rs:116-118
            save_png(file_name, rgb8)                                          # main.rs:119-123
        rend.set_progress(progress)
    img, rgb8, st = rend.render(scene.camera, params, want_rgb8=True)
    print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)        # drop(t), main.rs:126
    save_png(file_name, rgb8)                                                  # main.rs:127-128
    if a.hdr_out:
        write_pfm(a.hdr_out, img)
    print(f"{file_name}: {a.nx}x{ny}, {a.spp} spp, {st.n_rays} rays, {st.n_rays / st.seconds_device / 1e6:.0f} Mray/s on the device",
          file=sys.stderr)
    return 0


def render_to_noise(a, rend, scene, flags, file_name, t0):
    """--noise-target: samples in steps of --spp-step until the noise is reached or --spp are done.  With --preview-every the steps are
    taken here and the partial image of accum_read is saved after each; without, the library's rt_render_to_noise does the same."""
    params = make_params(a.nx, a.ny, a.spp, max_depth=a.max_depth, seed=a.seed, flags=flags)
    if a.preview_every or a.denoise:  # (rt_render_to_noise ends its accumulation: the filter needs it open)
        step = make_params(a.nx, a.ny, min(a.spp_step, a.spp), max_depth=a.max_depth, seed=a.seed, flags=flags)
        rend.accum_begin(scene.camera, step)
        if a.denoise and a.denoise_guide == "channels":
            rend.accum_track_channels()
        n_rays, seconds, done = 0, 0.0, 0
        while True:
            st = rend.accum_add(min(a.spp_step, a.spp - done))
            n_rays, seconds, done = n_rays + st.n_rays, seconds + st.seconds_device, done + st.n_paths // (a.nx * a.ny)
            _, rgb8, _, noise = rend.accum_read(want_rgb8=True)
            print(f"{noise.spp_done}/{a.spp} noise {noise.noise:.4g}", file=sys.stderr)
            if a.preview_every or not a.denoise:
                save_png(file_name, rgb8)
            if noise.noise <= a.noise_target or noise.spp_done >= a.spp:
                break
        if a.denoise:
            save_png(file_name, _denoised(a, rend))
        rend.accum_end()
    else:
        _, rgb8, _, noise, st = rend.render_to_noise(scene.camera, params, a.noise_target, a.spp_step, want_rgb8=True)
        n_rays, seconds = st.n_rays, st.seconds_device
        save_png(file_name, rgb8)
    print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)
    print(f"{file_name}: {a.nx}x{a.ny}, {noise.spp_done} of at most {a.spp} spp, noise {noise.noise:.4g} (target {a.noise_target:g}), "
          f"{n_rays} rays, {n_rays / seconds / 1e6:.0f} Mray/s on the device{', denoised' if a.denoise else ''}", file=sys.stderr)
    return 0


def render_adaptive(a, rend, scene, flags, file_name, t0):
    """--adaptive-tolerance: rt_render_adaptive in steps of --spp-step up to --spp; --counts-out saves the sample-count map."""
    params = make_params(a.nx, a.ny, a.spp, max_depth=a.max_depth, seed=a.seed, flags=flags)
    _, rgb8, _, counts, noise, info, st = rend.render_adaptive(scene.camera, params, a.adaptive_tolerance, a.spp_step, a.luminance_floor, a.min_spp,
                                                               want_rgb8=True)
    print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)
    save_png(file_name, rgb8)
    if a.counts_out:
        grey = np.minimum(counts.astype(np.float64) * (255.0 / max(a.spp, 1)), 255.0).astype(np.uint8)[::-1]  # (row 0 of the counts is the bottom row)
        save_png(a.counts_out, np.ascontiguousarray(np.repeat(grey[..., None], 3, axis=2)))
    print(f"{file_name}: {a.nx}x{a.ny}, {info.n_samples / max(counts.size, 1):.1f} spp on average ({info.spp_min}..{info.spp_max} of at most {a.spp}), "
          f"{info.n_active} pixels still active, noise {noise.noise:.4g}, {st.n_rays} rays, "
          f"{st.n_rays / max(st.seconds_device, 1e-9) / 1e6:.0f} Mray/s on the device", file=sys.stderr)
    return 0


def render_with_state(a, rend, scene, flags, file_name, t0):
    """--checkpoint / --resume / --first-sample / --merge: the adds are driven here in steps of --spp-step, as --denoise drives them, so
    that the state can be written between two of them.  The stopping rule is the command line's: --adaptive-tolerance (no pixel active,
    what rt_render_adaptive looks at), --noise-target, or plain --spp; --spp bounds the samples of the window either way, the resumed ones
    included, so an interrupted render and its resumption take exactly the steps of the uninterrupted one."""
    adaptive = a.adaptive_tolerance is not None
    state = AccumState.load(a.resume) if a.resume else None
    first = a.first_sample if a.first_sample is not None else (state.first_sample if state else 0)
    rend.accum_begin(scene.camera, make_params(a.nx, a.ny, min(a.spp_step, a.spp), max_depth=a.max_depth, seed=a.seed, flags=flags), first_sample=first)
    if a.denoise and a.denoise_guide == "channels":
        rend.accum_track_channels()
    n_buckets = 0  # M of the buckets the accumulation tracks, 0: none
    try:
        if state:
            rend.accum_import(state)
            # the buckets that were checkpointed beside the state go on with it, asked for or not; their M is the file's
            if os.path.exists(a.resume + ".buckets.npz"):
                try:
                    buckets = AccumBuckets.load(a.resume + ".buckets.npz")
                except (OSError, ValueError, KeyError) as e:
                    print(f"error: {a.resume}.buckets.npz: {e}", file=sys.stderr)
                    return 2
                if a.buckets is not None and a.buckets != buckets.M:
                    print(f"error: --buckets {a.buckets}, but {a.resume}.buckets.npz holds {buckets.M} buckets", file=sys.stderr)
                    return 2
                rend.accum_import_buckets(buckets)
                n_buckets = buckets.M
            elif a.want_buckets:
                print(f"error: --buckets / --robust with --resume need {a.resume}.buckets.npz, the buckets checkpointed beside the state", file=sys.stderr)
                return 2
        elif a.want_buckets:
            n_buckets = a.buckets if a.buckets is not None else DEFAULT_BUCKETS
            rend.accum_track_buckets(n_buckets)
        if state and a.filter is not None:  # the plane that was checkpointed beside the state goes on with it, under the same filter
            try:
                plane = AccumFilter.load(a.resume + ".filter.npz")
            except (OSError, ValueError, KeyError) as e:
                print(f"error: --pixel-filter with --resume needs {a.resume}.filter.npz, the plane checkpointed beside the state: {e}", file=sys.stderr)
                return 2
            if bytes(plane.filter) != bytes(a.filter):
                print(f"error: {a.resume}.filter.npz was summed under another filter than --pixel-filter, --filter-radius and --filter-param name", file=sys.stderr)
                return 2
            rend.accum_import_filter(plane)
        elif a.filter is not None:
            rend.accum_track_filter(a.filter)
        if state and a.features:  # likewise the feature records, under the same stride
            try:
                records = AccumFeatures.load(a.resume + ".features.npz")
            except (OSError, ValueError, KeyError) as e:
                print(f"error: --features with --resume needs {a.resume}.features.npz, the records checkpointed beside the state: {e}", file=sys.stderr)
                return 2
            if records.stride != a.feature_stride:
                print(f"error: {a.resume}.features.npz was summed under stride {records.stride}, not --feature-stride {a.feature_stride}", file=sys.stderr)
                return 2
            rend.accum_import_features(records)
        elif a.features:
            rend.accum_track_features(a.feature_stride)
        done, steps, n_rays, seconds = (state.done if state else 0), 0, 0, 0.0

        def finished():
            if done >= a.spp:
                return True
            if done == 0:
                return False
            if adaptive:
                return rend.accum_counts()[1].n_active == 0
            return a.noise_target is not None and rend.accum_read()[3].noise <= a.noise_target

        def save_state():
            if n_buckets:  # the buckets first: a state without its buckets resumes nowhere, buckets without a state are ignored
                rend.accum_export_buckets().save(a.checkpoint + ".buckets.npz")
            if a.filter is not None:  # likewise the filter plane
                rend.accum_export_filter().save(a.checkpoint + ".filter.npz")
            if a.features:  # and the feature records
                rend.accum_export_features().save(a.checkpoint + ".features.npz")
            rend.accum_export().save(a.checkpoint)

        while not finished():
            n = min(a.spp_step, a.spp - done)
            st = rend.accum_add_adaptive(n, a.adaptive_tolerance, a.luminance_floor, a.min_spp) if adaptive else rend.accum_add(n)
            done, steps, n_rays, seconds = done + n, steps + 1, n_rays + st.n_rays, seconds + st.seconds_device
            if a.checkpoint and steps % a.checkpoint_every == 0:
                save_state()
            print(f"{done}/{a.spp}", file=sys.stderr)
        for path in a.merge or ():
            rend.accum_merge(AccumState.load(path))
        if a.checkpoint and (a.merge or steps % a.checkpoint_every != 0 or steps == 0):
            save_state()  # (what was merged is part of it)
    except RtError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    _, rgb8, _, noise = rend.accum_read(want_rgb8=True)
    counts, info = rend.accum_counts()
    robust_line = ""
    if a.robust_mode:
        _, rinfo, trim, rgb8 = rend.accum_robust(*a.robust_mode, want_trim=True, want_rgb8=True)
        robust_line = (f"{file_name}: robust read-out ({a.robust}, {n_buckets} buckets): energy_removed {rinfo.energy_removed:.4g}, trimmed_fraction "
                       f"{rinfo.trimmed_fraction:.4g}, {rinfo.nonfinite_dropped} non-finite bucket means dropped (a biased estimate: the trim takes "
                       f"energy that belongs to the frame)")
        if a.firefly_map:
            worst = trim.max(axis=2).astype(np.uint32)  # the largest trim of the three channels; at most (M - 1) / 2
            grey = (worst * 255 // max((n_buckets - 1) // 2, 1)).astype(np.uint8)[::-1]  # (row 0 of the trims is the bottom row)
            save_png(a.firefly_map, np.ascontiguousarray(np.repeat(grey[..., None], 3, axis=2)))
    if a.denoise:
        rgb8 = _denoised(a, rend)
    if a.filter is not None:
        rgb8 = rend.accum_filtered(want_rgb8=True)[1]
    if a.features and (a.albedo_out or a.normal_out or a.depth_out):
        feat = rend.accum_features()
        if a.albedo_out:
            write_pfm(a.albedo_out, feat["albedo"])
        if a.normal_out:
            write_pfm(a.normal_out, feat["normal"])
        if a.depth_out:
            write_pfm(a.depth_out, np.repeat(feat["depth"][..., None], 3, axis=2))
    rend.accum_end()
    print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)
    save_png(file_name, rgb8)
    if robust_line:
        print(robust_line, file=sys.stderr)
    if a.counts_out:
        grey = np.minimum(counts.astype(np.float64) * (255.0 / max(a.spp, 1)), 255.0).astype(np.uint8)[::-1]  # (row 0 of the counts is the bottom row)
        save_png(a.counts_out, np.ascontiguousarray(np.repeat(grey[..., None], 3, axis=2)))
    print(f"{file_name}: {a.nx}x{a.ny}, samples {first}..{first + info.spp_max} ({info.n_samples / max(counts.size, 1):.1f} spp on average), "
          f"noise {noise.noise:.4g}, {n_rays} rays traced here"
          + (f", {n_rays / seconds / 1e6:.0f} Mray/s on the device" if seconds > 0 else "") + (", denoised" if a.denoise else ""), file=sys.stderr)
    return 0


def _denoised(a, rend):
    if a.robust_mode:
        return rend.accum_denoise_robust(*a.robust_mode, a.denoise_radius, a.denoise_patch, a.denoise_strength, want_rgb8=True)[1]
    if a.denoise_levels is not None:
        return rend.accum_denoise_multiscale(a.denoise_levels, a.denoise_guide, a.denoise_radius, a.denoise_patch, a.denoise_strength, want_rgb8=True)[1]
    if a.denoise_guide == "features":
        return rend.accum_denoise_features(a.feature_guide, a.denoise_radius, a.denoise_patch, a.denoise_strength, want_rgb8=True)[1]
    if a.denoise_guide == "channels":
        return rend.accum_denoise_channels(a.denoise_radius, a.denoise_patch, a.denoise_strength, want_rgb8=True)[1]
    return rend.accum_denoise(a.denoise_radius, a.denoise_patch, a.denoise_strength, want_rgb8=True)[1]


def render_halves(a, rend, scene, flags, file_name, t0):
    """--denoise --denoise-guide halves: one add of --spp samples and the cross filter; --residual-target: Renderer.render_to_residual."""
    params = make_params(a.nx, a.ny, a.spp, max_depth=a.max_depth, seed=a.seed, flags=flags)
    if a.residual_target is not None:
        _, rgb8, _, res, done = rend.render_to_residual(scene.camera, params, a.residual_target, a.spp_step, a.denoise_radius, a.denoise_patch,
                                                        a.denoise_strength, want_rgb8=True)
    else:
        rend.accum_begin(scene.camera, params)
        rend.accum_track_halves()
        rend.accum_add(a.spp)
        if a.denoise_select is not None:
            _, rgb8, index, est, info = rend.accum_denoise_select(a.select, want_rgb8=True)
            rend.accum_end()
            print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)
            save_png(file_name, rgb8)
            ks = list(a.select.strength)[:a.select.n_strengths]
            if a.select_map_out:
                with open(a.select_map_out, "wb") as f:  # (np.savez would append .npz to a name)
                    np.savez(f, index=index[::-1], est=est[::-1], strengths=np.asarray(ks, np.float32))
            print(f"{file_name}: {a.nx}x{a.ny}, {a.spp} spp, cross-filtered at the strength chosen per pixel from " + ", ".join("%g" % k for k in ks) +
                  f": frame-wide best {ks[info.best]:g}; estimated luminance MSE of a half filter " + ", ".join("%.4g" % e for e in list(info.est_mse)[:len(ks)]) +
                  "; pixels per candidate " + ", ".join(str(n) for n in list(info.chosen)[:len(ks)]) + f"; {info.usable} usable pixels", file=sys.stderr)
            return 0
        _, rgb8, _, res = rend.accum_denoise_halves(a.denoise_radius, a.denoise_patch, a.denoise_strength, want_rgb8=True)
        rend.accum_end()
        done = a.spp
    print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)
    save_png(file_name, rgb8)
    print(f"{file_name}: {a.nx}x{a.ny}, {done} of at most {a.spp} spp, cross-filtered, residual noise {res.residual_noise:.4g} (a lower bound of "
          f"the filtered frame's relative error)" + (f", target {a.residual_target:g}" if a.residual_target is not None else ""), file=sys.stderr)
    return 0


def render_denoised(a, rend, scene, flags, file_name, t0):
    """--denoise without --noise-target: begin, one add of --spp samples, the filter, end."""
    rend.accum_begin(scene.camera, make_params(a.nx, a.ny, a.spp, max_depth=a.max_depth, seed=a.seed, flags=flags))
    if a.denoise_guide == "channels":
        rend.accum_track_channels()
    st = rend.accum_add(a.spp)
    noise = rend.accum_read()[3]
    rgb8 = _denoised(a, rend)
    rend.accum_end()
    print(f"elapsed {time.perf_counter() - t0:.3f} s", file=sys.stderr)
    save_png(file_name, rgb8)
    print(f"{file_name}: {a.nx}x{a.ny}, {a.spp} spp, noise {noise.noise:.4g} before the filter, denoised, {st.n_rays} rays, "
          f"{st.n_rays / st.seconds_device / 1e6:.0f} Mray/s on the device", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
