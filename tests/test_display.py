"""The display transform on the GPU (rt_set_display, rt_display_info, rt_debug_display) against tests/display_ref.py.

The pixel stage — every curve x transfer x dither under a manual exposure — bit for bit through rt_debug_display, under the sRGB transfer
outside the reference's ambiguous values, where either of the two levels is right.  The identity configuration against no display on the
designed imported states.  The statistics: the lit count, the percentile's bin and its exposure bit for bit, the key exposure within one
f32 ulp, the same bits on a second run.  Every read-out of the accumulation family under a display, with everything but out_rgb8
unchanged in every bit.  The errors of the header.

Every test that sets a display on the session's Renderer clears it in a `finally`."""
import ctypes as C
import itertools

import numpy as np
import pytest

import designed_states as ds
import display_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
CURVES = (("clamp", ref.CLAMP), ("reinhard", ref.REINHARD), ("aces", ref.ACES))
TRANSFERS = (("gamma2", ref.GAMMA2), ("srgb", ref.SRGB))
DITHERS = (("none", ref.NONE), ("bayer8", ref.BAYER8))
WHITE = 3.0


def _held(got, want, info, what):
    """rgb8 against the reference: equal outside the ambiguous mask, either neighbouring level inside it; the mask within its cap."""
    assert got.shape == want.shape and got.dtype == np.uint8
    a = info["ambiguous"]
    if a is None:
        bad = got != want
    else:
        share = float(a.mean())
        print(what, "ambiguous share", share)
        assert share <= ref.AMBIGUOUS_CAP, (what, share)
        bad = np.where(a, (got != info["level_lo"]) & (got != info["level_hi"]), got != want)
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        assert False, (what, int(bad.sum()), "values differ, first at", first, int(got[first]), int(want[first]))


def _saturated_held(got_info, got_rgb8, info, what):
    assert got_info.n_non_finite == info["n_non_finite"], (what, got_info.n_non_finite, info["n_non_finite"])
    assert got_info.n_saturated == int((got_rgb8 == 255).sum()), what  # what was written
    if info["ambiguous"] is None or not (info["ambiguous"] & (info["level_hi"] == 255)).any():
        assert got_info.n_saturated == info["n_saturated"], (what, got_info.n_saturated, info["n_saturated"])


@pytest.mark.parametrize("nx,rows", ref.FRAMES)
def test_pixel_stage_against_the_reference(rt, renderer, nx, rows):
    for plane, e, name in ((ref.designed_plane(nx, rows), 1.0, "designed"), (ref.log_uniform_plane(nx, rows), 0.37, "log-uniform")):
        for (cn, c), (tn, t), (dn, d) in itertools.product(CURVES, TRANSFERS, DITHERS):
            what = (nx, rows, name, cn, tn, dn)
            disp = rt.make_display(e, curve=cn, white=WHITE, transfer=tn, dither=dn)
            got, ginfo = renderer.debug_display(plane, disp)
            want, info = ref.display(plane, disp)
            _held(got, want, info, what)
            _saturated_held(ginfo, got, info, what)
            assert ginfo.exposure == F32(e) and ginfo.n_lit == 0 and ginfo.log_average == 0 and ginfo.percentile_luminance == 0, what


def test_srgb_on_either_side_of_every_level_boundary_is_exact(rt, renderer):
    t = ref.srgb_boundary_values()
    img = np.repeat(t.reshape(1, -1, 1), 3, axis=2)
    disp = rt.make_display(transfer="srgb")
    want, info = ref.display(img, disp)
    assert not info["ambiguous"].any()
    got, _ = renderer.debug_display(img, disp)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


def _import_state(rt, r, nx, rows, done):
    scene = rt.Scene.build("test_sphere", nx / rows)
    r.upload(scene)
    prm = rt.make_params(nx, rows, 1, max_depth=8, seed=77)
    st = ds.state(nx, rows, done)
    s = rt.AccumState(st["nx"], st["rows"], st["first_sample"], st["done"], st["planes"], rt.accum_frame_id(scene.camera, prm), sum=st["sum"],
                      moments=st["moments"], counts=st["counts"], converged=st["converged"], channel_moments=st["channel_moments"])
    r.accum_begin(scene.camera, prm)
    r.accum_import(s)


@pytest.mark.parametrize("done", ds.UNIFORM_DONE)
def test_identity_display_is_no_display(rt, ctx, done):
    nx, rows = 40, 20
    try:
        _import_state(rt, ctx, nx, rows, done)
        img0, rgb0, _, _ = ctx.accum_read(want_rgb8=True)
        ctx.set_display(rt.make_display(1.0, curve="clamp", transfer="gamma2", dither="none"))
        img1, rgb1, _, _ = ctx.accum_read(want_rgb8=True)
        assert np.array_equal(rgb0, rgb1), int((rgb0 != rgb1).sum())
        assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
        info = ctx.display_info()
        assert info.exposure == 1 and info.n_saturated == int((rgb1 == 255).sum()) and info.n_non_finite == int((~np.isfinite(img1)).any(axis=-1).sum()) > 0
        ctx.accum_end()
    finally:
        ctx.set_display(None)


def _constant(nx, rows):
    return np.full((rows, nx, 3), 0.3, F32)


def _one_lit(nx, rows):
    img = np.zeros((rows, nx, 3), F32)
    img.reshape(-1, 3)[(nx * rows * 2) // 3] = [0.0, 5.0, 0.25]
    return img


def _black(nx, rows):
    img = np.zeros((rows, nx, 3), F32)
    img.reshape(-1, 3)[0] = [-1.0, 0.0, 0.0]
    return img


STAT_PLANES = (("constant", _constant), ("one lit pixel", _one_lit), ("black", _black), ("random", ref.statistics_plane))


@pytest.mark.parametrize("nx,rows", ref.FRAMES)
def test_percentile_exposure_is_exact(rt, renderer, nx, rows):
    for (name, make), q in itertools.product(STAT_PLANES, (2.0 ** -20, 0.5, 0.99, 1.0)):
        img = make(nx, rows)
        disp = rt.make_display(0.5, auto="percentile", percentile=q, curve="reinhard", white=WHITE, dither="bayer8")
        got, ginfo = renderer.debug_display(img, disp)
        s = ref.statistics(img, disp)
        what = (nx, rows, name, q)
        assert ginfo.n_lit == s["n_lit"], (what, ginfo.n_lit, s["n_lit"])
        assert F32(ginfo.percentile_luminance).view(np.uint32) == F32(s["percentile_luminance"]).view(np.uint32), (what, ginfo.percentile_luminance, s["percentile_luminance"])
        assert F32(ginfo.exposure).view(np.uint32) == F32(s["exposure"]).view(np.uint32), (what, ginfo.exposure, s["exposure"])
        assert ginfo.log_average == 0
        if name == "black":
            assert ginfo.n_lit == 0 and ginfo.exposure == 1 and ginfo.percentile_luminance == 0
        want, info = ref.display(img, disp, e=ginfo.exposure)  # the pixel stage under the reported e
        _held(got, want, info, what)
        _saturated_held(ginfo, got, info, what)
        again, ainfo = renderer.debug_display(img, disp)
        assert np.array_equal(again, got) and bytes(ainfo) == bytes(ginfo), what


@pytest.mark.parametrize("nx,rows", ref.FRAMES)
def test_key_exposure_within_one_ulp(rt, renderer, nx, rows):
    """n_lit exact; e within one f32 ulp of the numpy value (the logarithms, the tree and the exponential keep the f64
    quotient within 1e-12 of numpy's, relatively: the two f32 roundings are neighbours at the most); the same bits on a second run."""
    for name, make in STAT_PLANES:
        img = make(nx, rows)
        disp = rt.make_display(0.18, auto="key", curve="aces", dither="none")
        got, ginfo = renderer.debug_display(img, disp)
        s = ref.statistics(img, disp)
        what = (nx, rows, name)
        print(what, "e", ginfo.exposure, "numpy", s["exposure"], "log average", ginfo.log_average, s["log_average"], "n_lit", ginfo.n_lit)
        assert ginfo.n_lit == s["n_lit"], (what, ginfo.n_lit, s["n_lit"])
        e, w = F32(ginfo.exposure), F32(s["exposure"])
        assert e == w or e == np.nextafter(w, F32(np.inf)) or e == np.nextafter(w, F32(-np.inf)), (what, e, w)
        assert ginfo.percentile_luminance == 0
        if s["n_lit"]:
            assert abs(ginfo.log_average / s["log_average"] - 1) <= 1e-12, (what, ginfo.log_average, s["log_average"])
        else:
            assert ginfo.exposure == 1 and ginfo.log_average == 0
        want, info = ref.display(img, disp, e=ginfo.exposure)
        _held(got, want, info, what)
        _saturated_held(ginfo, got, info, what)
        again, ainfo = renderer.debug_display(img, disp)
        assert np.array_equal(again, got) and bytes(ainfo) == bytes(ginfo), what


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _noise_bytes(n):
    return bytes(n)


def test_every_read_out_under_a_display(rt, ctx):
    """64 x 48, 8 spp of an emitter scene with channels, halves and buckets tracked, under ACES + sRGB + Bayer + key: the seven calls, each
    against the reference on the f32 image of the same call and against the same call without a display."""
    nx, ny = 64, 48
    scene = rt.Scene.build("simple_light_scene", nx / ny)
    prm = rt.make_params(nx, ny, 8, max_depth=12, seed=5)
    disp = rt.make_display(0.18, auto="key", curve="aces", transfer="srgb", dither="bayer8")
    calls = {
        "read": lambda r: (lambda o: (o[0], o[1], [o[2], _noise_bytes(o[3])]))(r.accum_read(want_rgb8=True, want_sem=True)),
        "denoise": lambda r: (lambda o: (o[0], o[1], []))(r.accum_denoise(radius=2, want_rgb8=True)),
        "channels": lambda r: (lambda o: (o[0], o[1], []))(r.accum_denoise_channels(radius=2, want_rgb8=True)),
        "halves": lambda r: (lambda o: (o[0], o[1], [o[2], bytes(o[3])]))(r.accum_denoise_halves(radius=2, want_rgb8=True, want_err=True)),
        "denoise robust": lambda r: (lambda o: (o[0], o[1], []))(r.accum_denoise_robust(radius=2, want_rgb8=True)),
        "multiscale": lambda r: (lambda o: (o[0], o[1], []))(r.accum_denoise_multiscale(levels=2, radius=2, want_rgb8=True)),
        "read robust": lambda r: (lambda o: (o[0], o[3], [o[2], bytes(o[1])]))(r.accum_robust(want_trim=True, want_rgb8=True)),
    }
    try:
        ctx.upload(scene)
        ctx.accum_begin(scene.camera, prm)
        ctx.accum_track_channels(), ctx.accum_track_halves(), ctx.accum_track_buckets(4)
        ctx.accum_add(8)
        plain = {k: f(ctx) for k, f in calls.items()}
        ctx.set_display(disp)  # does not end the accumulation
        for k, f in calls.items():
            img, rgb8, rest = f(ctx)
            img0, rgb0, rest0 = plain[k]
            assert np.array_equal(_bits(img), _bits(img0)), (k, "out_rgb_f32 changed")
            for a, b in zip(rest, rest0):
                assert (a == b) if isinstance(a, bytes) else np.array_equal(_bits(a), _bits(b)), (k, "an output beside out_rgb8 changed")
            info = ctx.display_info()
            s = ref.statistics(img, disp)
            assert info.n_lit == s["n_lit"] > 0, (k, info.n_lit, s["n_lit"])
            e, w = F32(info.exposure), F32(s["exposure"])
            assert e == w or e == np.nextafter(w, F32(np.inf)) or e == np.nextafter(w, F32(-np.inf)), (k, e, w)
            want, rinfo = ref.display(img, disp, e=info.exposure)
            _held(rgb8, want, rinfo, k)
            _saturated_held(info, rgb8, rinfo, k)
            assert not np.array_equal(rgb8, rgb0), (k, "the display changed nothing")
        # rt_render keeps the reference quantisation; rt_scene_upload keeps the display (and ends the accumulation, as ever)
        prm1 = rt.make_params(nx, ny, 2, max_depth=12, seed=5)
        _, r8, _ = ctx.render(scene.camera, prm1, want_rgb8=True)
        ctx.set_display(None)
        _, r8_plain, _ = ctx.render(scene.camera, prm1, want_rgb8=True)
        assert np.array_equal(r8, r8_plain)
        # a further add continues bit for bit
        ctx.accum_add(3)
        after = ctx.accum_read(want_rgb8=True)
        ctx.accum_end()
        ctx.accum_begin(scene.camera, prm)
        ctx.accum_track_channels(), ctx.accum_track_halves(), ctx.accum_track_buckets(4)
        ctx.accum_add(8), ctx.accum_add(3)
        straight = ctx.accum_read(want_rgb8=True)
        assert np.array_equal(_bits(after[0]), _bits(straight[0])) and np.array_equal(after[1], straight[1]) and bytes(after[3]) == bytes(straight[3])
        ctx.set_display(disp)
        ctx.upload(scene)
        ctx.accum_begin(scene.camera, prm)
        ctx.accum_add(2)
        img, rgb8, _, _ = ctx.accum_read(want_rgb8=True)
        want, rinfo = ref.display(img, disp, e=ctx.display_info().exposure)
        _held(rgb8, want, rinfo, "after rt_scene_upload")
        # no f32 pointer from the caller: the same rgb8
        out = np.zeros((ny, nx, 3), np.uint8)
        ctx._call("rt_accum_read", None, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None)
        assert np.array_equal(out, rgb8)
        ctx.accum_end()
    finally:
        ctx.set_display(None)


def test_errors(rt):
    r = rt.Renderer(0)
    try:
        with pytest.raises(rt.RtError, match="rt_display_info"):
            r.display_info()
        img = ref.log_uniform_plane(7, 5)
        r.debug_display(img, rt.make_display())  # the test hook leaves rt_display_info alone
        with pytest.raises(rt.RtError, match="rt_display_info"):
            r.display_info()
        scene = rt.Scene.build("test_sphere", 7 / 5)
        r.upload(scene)
        r.accum_begin(scene.camera, rt.make_params(7, 5, 1, max_depth=4))
        r.accum_add(1)
        r.accum_read(want_rgb8=True)  # no display: still none
        with pytest.raises(rt.RtError, match="rt_display_info"):
            r.display_info()
        good = rt.make_display(2.0, curve="aces", transfer="srgb")
        r.set_display(good)
        img, rgb8, _, _ = r.accum_read(want_rgb8=True)
        assert r.display_info().exposure == 2
        for bad in (dict(exposure=0.0), dict(exposure=float("nan")), dict(auto="percentile", percentile=0.0), dict(curve="reinhard", white=0.0), dict(curve=3),
                    dict(transfer=2), dict(dither=2), dict(auto=3)):
            with pytest.raises(rt.RtError, match="rt_set_display"):
                r.set_display(rt.make_display(**bad))
        d = rt.make_display()
        d.reserved = 1
        with pytest.raises(rt.RtError, match="rt_set_display"):
            r.set_display(d)
        again = r.accum_read(want_rgb8=True)[1]  # the previous display is still in force
        assert np.array_equal(again, rgb8)
        want, info = ref.display(img, good)
        _held(again, want, info, "the display before the refused ones")
        with pytest.raises(rt.RtError, match="rt_debug_display"):
            r.debug_display(img, d)
        r.accum_end()
    finally:
        r.close()


def test_render_py_display_flags_and_hdr_out(rt, renderer, tmp_path):
    """render.py with the display flags renders through an accumulation: the PFM of --hdr-out is rt_render's f32 image bit for bit, and the
    PNG is the display transform of it."""
    import os
    import subprocess
    import sys
    from PIL import Image
    from ray_tracing_in_one_weekend_amd import images
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    png, pfm = str(tmp_path / "frame.png"), str(tmp_path / "frame.pfm")
    c = subprocess.run([sys.executable, "-m", "ray_tracing_in_one_weekend_amd.render", "--scene", "simple_light_scene", "--nx", "64", "--ny", "48", "--spp", "4",
                        "--auto-exposure", "key", "--tone", "aces", "--srgb", "--dither", "--out", png, "--hdr-out", pfm], cwd=root, capture_output=True,
                       text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    assert "display: exposure" in c.stderr
    scene = rt.Scene.build("simple_light_scene", 64 / 48)
    renderer.upload(scene)
    img, _, _ = renderer.render(scene.camera, rt.make_params(64, 48, 4))
    hdr = images.read_pfm(pfm)
    assert np.array_equal(hdr.view(np.uint32), img.view(np.uint32))
    disp = rt.make_display(0.18, auto="key", curve="aces", transfer="srgb", dither="bayer8")
    got = np.asarray(Image.open(png).convert("RGB"), np.uint8)
    s = ref.statistics(img, disp)
    for e in (s["exposure"], np.nextafter(F32(s["exposure"]), F32(np.inf)), np.nextafter(F32(s["exposure"]), F32(-np.inf))):
        want, info = ref.display(img, disp, e=e)
        a = info["ambiguous"]
        if not np.where(a, (got != info["level_lo"]) & (got != info["level_hi"]), got != want).any():
            break
    else:
        assert False, "the PNG is not the display transform of the PFM under the key exposure or either of its f32 neighbours"
