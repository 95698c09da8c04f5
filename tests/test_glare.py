"""The glare on the GPU (rt_set_glare, rt_glare_info, rt_glare_image, rt_debug_glare) against tests/glare_ref.py.

The kernels through rt_debug_glare: `out` bit for bit, NaN positions and payloads included, with the plain and with the fused down chain,
on every frame, plane and parameter set of the issue; out_rgb8 against display_ref.display of the reference's `out` under the reference
quantisation and under {KEY, ACES, SRGB, BAYER8}, there outside display_ref's ambiguous values.  Then the product calls on one small
accumulation: every read-out of the display's list under a glare, everything but out_rgb8 unchanged in every bit, the errors of the
header, and render.py.

Every test that sets a glare, a display or a chain on a Renderer clears it in a `finally`."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref
import display_ref
import glare_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMETERS = tuple(itertools.product((1, 3, 8), (0.5, 1.0), (0.0, 0.25, 1.0), (0.0, 1.0)))  # levels x spread x amount x threshold
CHAINS = ("plain", "fused")


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


_REFERENCE = {}


def _reference(nx, rows, name, plane, prm):
    """glare_ref.glare of a plane under one parameter set, computed once for both chains."""
    key = (nx, rows, name, prm)
    if key not in _REFERENCE:
        L, sp, a, t = prm
        _REFERENCE[key] = ref.glare(plane, ref.make(a, sp, t, L))
    return _REFERENCE[key]


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got, F32).view(np.uint32), np.ascontiguousarray(want, F32).view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(int(i) for i in bad[0])
        assert False, (what, len(bad), "values differ, first at", first, float(got[first]), float(want[first]))


def _held(got, want, info, what):
    """rgb8 against display_ref: equal outside the ambiguous mask, either neighbouring level inside it; the mask within its cap."""
    a = info["ambiguous"]
    if a is None:
        bad = got != want
    else:
        assert float(a.mean()) <= display_ref.AMBIGUOUS_CAP, (what, float(a.mean()))
        bad = np.where(a, (got != info["level_lo"]) & (got != info["level_hi"]), got != want)
    assert not bad.any(), (what, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("nx,rows", ref.FRAMES)
def test_out_is_the_reference_bit_for_bit(rt, ctx, nx, rows, chain):
    try:
        ctx.debug_glare_chain(chain)
        for (name, make), prm in itertools.product(ref.PLANES, PARAMETERS):
            plane = make(nx, rows)
            want, winfo = _reference(nx, rows, name, plane, prm)
            L, sp, a, t = prm
            got, _, info = ctx.debug_glare(plane, rt.make_glare(a, sp, t, L), want_rgb8=False)
            what = (nx, rows, name, chain, prm)
            _same_bits(got, want, what)
            assert (info.levels, info.coarse_nx, info.coarse_rows, info.reserved) == (winfo["levels"], winfo["coarse_nx"], winfo["coarse_rows"], 0), what
    finally:
        ctx.debug_glare_chain("auto")


@pytest.mark.parametrize("nx,rows", ref.FRAMES)
def test_rgb8_is_the_display_of_the_glared_reference(rt, ctx, nx, rows):
    disp = rt.make_display(0.18, auto="key", curve="aces", transfer="srgb", dither="bayer8")
    for (name, make), prm in itertools.product(ref.PLANES, ((3, 0.5, 0.25, 0.0), (8, 1.0, 1.0, 1.0))):
        plane = make(nx, rows)
        want, _ = _reference(nx, rows, name, plane, prm)
        L, sp, a, t = prm
        g = rt.make_glare(a, sp, t, L)
        what = (nx, rows, name, prm)
        got, rgb8, _ = ctx.debug_glare(plane, g)  # no display: the reference quantisation, the display of the identity configuration
        _same_bits(got, want, what)
        assert np.array_equal(rgb8, denoise_ref.finalize_rgb8(want)), what
        assert np.array_equal(rgb8, display_ref.display(want, display_ref.make())[0]), what
        _, rgb8_identity, _ = ctx.debug_glare(plane, g, rt.make_display())
        assert np.array_equal(rgb8_identity, rgb8), what
        _, rgb8_d, _ = ctx.debug_glare(plane, g, disp)
        s = display_ref.statistics(want, disp)
        for e in (s["exposure"], np.nextafter(F32(s["exposure"]), F32(np.inf)), np.nextafter(F32(s["exposure"]), F32(-np.inf))):
            w8, info = display_ref.display(want, disp, e=e)  # (the key exposure is held within one f32 ulp: tests/test_display.py)
            a_ = info["ambiguous"]
            if not np.where(a_, (rgb8_d != info["level_lo"]) & (rgb8_d != info["level_hi"]), rgb8_d != w8).any():
                assert float(a_.mean()) <= display_ref.AMBIGUOUS_CAP, (what, float(a_.mean()))
                break
        else:
            assert False, (what, "out_rgb8 is not the display of the glared reference under the key exposure or either of its f32 neighbours")


def test_the_debug_hook_leaves_the_context_alone_and_names_its_refusals(rt):
    r = rt.Renderer(0)
    try:
        img = ref.random_plane(7, 13)
        r.debug_glare(img, rt.make_glare())
        with pytest.raises(rt.RtError, match="rt_glare_info"):
            r.glare_info()
        with pytest.raises(rt.RtError, match="rt_glare_image"):
            r.glare_image(7, 13)
        with pytest.raises(rt.RtError, match="rt_display_info"):
            r.display_info()
        for bad in (dict(amount=1.5), dict(amount=float("nan")), dict(spread=0.0), dict(threshold=-1.0), dict(threshold=float("inf")), dict(levels=0),
                    dict(levels=9)):
            with pytest.raises(rt.RtError, match="rt_debug_glare"):
                r.debug_glare(img, rt.make_glare(**bad))
            with pytest.raises(rt.RtError, match="rt_set_glare"):
                r.set_glare(rt.make_glare(**bad))
        with pytest.raises(rt.RtError, match="rt_debug_glare"):
            r.debug_glare(img, rt.make_glare(), rt.make_display(exposure=0.0))
        with pytest.raises(rt.RtError, match="rt_debug_glare_chain"):
            r.debug_glare_chain(3)
    finally:
        r.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_every_read_out_under_a_glare(rt, ctx):
    """64 x 48, 8 spp of an emitter scene with channels, halves and buckets tracked (the frame of tests/test_display.py): the seven calls
    under a glare, without and with a display behind it, each against the references on the f32 image of the same call and against the
    same call without a glare."""
    nx, ny = 64, 48
    scene = rt.Scene.build("simple_light_scene", nx / ny)
    prm = rt.make_params(nx, ny, 8, max_depth=12, seed=5)
    glare, rg = rt.make_glare(0.25, 0.7, 0.0, 4), ref.make(0.25, 0.7, 0.0, 4)
    disp = rt.make_display(1.5, curve="aces", transfer="gamma2", dither="bayer8")
    calls = {
        "read": lambda r: (lambda o: (o[0], o[1], [o[2], bytes(o[3])]))(r.accum_read(want_rgb8=True, want_sem=True)),
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
        state0 = ctx.accum_export()
        plain = {k: f(ctx) for k, f in calls.items()}
        with pytest.raises(rt.RtError, match="rt_glare_info"):
            ctx.glare_info()
        ctx.set_glare(glare)  # does not end the accumulation
        for with_display in (False, True):
            ctx.set_display(disp if with_display else None)
            for k, f in calls.items():
                img, rgb8, rest = f(ctx)
                img0, rgb0, rest0 = plain[k]
                assert np.array_equal(_bits(img), _bits(img0)), (k, "out_rgb_f32 changed")
                for a, b in zip(rest, rest0):
                    assert (a == b) if isinstance(a, bytes) else np.array_equal(_bits(a), _bits(b)), (k, "an output beside out_rgb8 changed")
                want, winfo = ref.glare(img, rg)
                _same_bits(ctx.glare_image(nx, ny), want, (k, "rt_glare_image"))
                info = ctx.glare_info()
                assert (info.levels, info.coarse_nx, info.coarse_rows) == (winfo["levels"], winfo["coarse_nx"], winfo["coarse_rows"]) == (4, 4, 3), k
                if with_display:
                    w8, dinfo = display_ref.display(want, disp)
                    _held(rgb8, w8, dinfo, k)
                    assert ctx.display_info().n_saturated == int((rgb8 == 255).sum())
                else:
                    assert np.array_equal(rgb8, denoise_ref.finalize_rgb8(want)), k
                assert not np.array_equal(rgb8, rgb0), (k, "the glare changed nothing")
        ctx.set_display(None)
        state1 = ctx.accum_export()
        for name in ("sum", "moments", "counts", "converged", "channel_moments"):
            a, b = getattr(state0, name, None), getattr(state1, name, None)
            assert (a is None) == (b is None) and (a is None or np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))), name
        # no f32 pointer from the caller: the same rgb8
        _, rgb8, _, _ = ctx.accum_read(want_rgb8=True)
        out = np.zeros((ny, nx, 3), np.uint8)
        ctx._call("rt_accum_read", None, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None)
        assert np.array_equal(out, rgb8)
        # amount 0 is no glare; an invalid glare leaves the one before in force; NULL restores the previous bytes
        ctx.set_glare(rt.make_glare(0.0, 0.7, 0.0, 4))
        assert np.array_equal(ctx.accum_read(want_rgb8=True)[1], plain["read"][1])
        ctx.set_glare(glare)
        with pytest.raises(rt.RtError, match="rt_set_glare"):
            ctx.set_glare(rt.make_glare(amount=2.0))
        assert np.array_equal(ctx.accum_read(want_rgb8=True)[1], rgb8)
        # rt_render keeps the reference quantisation; rt_scene_upload keeps the glare (and ends the accumulation, as ever)
        prm1 = rt.make_params(nx, ny, 2, max_depth=12, seed=5)
        _, r8, _ = ctx.render(scene.camera, prm1, want_rgb8=True)
        ctx.upload(scene)
        ctx.accum_begin(scene.camera, prm)
        ctx.accum_add(8)
        assert np.array_equal(ctx.accum_read(want_rgb8=True)[1], rgb8), "after rt_scene_upload"
        ctx.set_glare(None)
        assert np.array_equal(ctx.accum_read(want_rgb8=True)[1], plain["read"][1])
        _, r8_plain, _ = ctx.render(scene.camera, prm1, want_rgb8=True)
        assert np.array_equal(r8, r8_plain)
    finally:
        ctx.set_glare(None), ctx.set_display(None)


def test_a_shard_refuses_rgb8_under_a_glare_and_nothing_else(rt):
    r = rt.Renderer(0)
    try:
        nx, ny = 32, 24
        scene = rt.Scene.build("test_sphere", nx / ny)
        r.upload(scene)
        prm = rt.make_params(nx, ny, 2, max_depth=4, seed=3, shard_count=2, shard_id=1, shard_band=4)
        r.accum_begin(scene.camera, prm)
        r.accum_add(2)
        img0, rgb0, sem0, _ = r.accum_read(want_rgb8=True, want_sem=True)
        r.set_glare(rt.make_glare())
        with pytest.raises(rt.RtError, match=r"rt_accum_read failed \(-5\).*no neighbourhoods"):  # RT_ERR_STATE, and the reason
            r.accum_read(want_rgb8=True)
        img1, none8, sem1, _ = r.accum_read(want_rgb8=False, want_sem=True)  # no out_rgb8: unaffected
        assert none8 is None and np.array_equal(_bits(img0), _bits(img1)) and np.array_equal(_bits(sem0), _bits(sem1))
        r.set_glare(None)
        assert np.array_equal(r.accum_read(want_rgb8=True)[1], rgb0)
        r.accum_end()
    finally:
        r.close()


def test_render_py_glare_flags_and_glare_out(rt, renderer, tmp_path):
    """render.py --glare .. --glare-out: the PNG and the PFM are what the library calls give — the PFM the reference's `out` of
    rt_render's f32 image, the PNG its reference quantisation; --hdr-out stays the un-glared frame."""
    from PIL import Image
    from ray_tracing_in_one_weekend_amd import images
    png, pfm, hdr = str(tmp_path / "frame.png"), str(tmp_path / "glare.pfm"), str(tmp_path / "frame.pfm")
    c = subprocess.run([sys.executable, "-m", "ray_tracing_in_one_weekend_amd.render", "--scene", "simple_light_scene", "--nx", "64", "--ny", "48", "--spp", "4",
                        "--glare", "0.2", "--glare-levels", "3", "--glare-spread", "0.5", "--glare-threshold", "0.5", "--out", png, "--glare-out", pfm,
                        "--hdr-out", hdr], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    assert "glare:" in c.stderr
    scene = rt.Scene.build("simple_light_scene", 64 / 48)
    renderer.upload(scene)
    img, _, _ = renderer.render(scene.camera, rt.make_params(64, 48, 4))
    assert np.array_equal(images.read_pfm(hdr).view(np.uint32), img.view(np.uint32))
    want, _ = ref.glare(img, ref.make(0.2, 0.5, 0.5, 3))
    _same_bits(images.read_pfm(pfm), want, "--glare-out")
    assert np.array_equal(np.asarray(Image.open(png).convert("RGB"), np.uint8), denoise_ref.finalize_rgb8(want))
