"""The selected strength on the GPU (rt_accum_denoise_select, rt_debug_denoise_select) against tests/select_ref.py, bit for bit: out, the
index map, est, out_j and E_j of every candidate and every field of RtSelectInfo, through the hook on designed inputs of every size at which
the tiles, halos and the tree take another path, and through the product call on imported states.  Held to the code that was there before:
out_j is rt_accum_denoise_halves at k_j, and with T = 0 every pixel of the result is that call's at the chosen strength.  out_rgb8 and
the display and glare behind it; nothing else an accumulation returns moves; the errors; the joined context of an RtMulti; and the error
of rendered frames against converged ones."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import accum_state_ref
import denoise_ref
import glare_ref
import halves_ref
import select_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
KS = ref.FOUR_STRENGTHS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), "values differ")


def _held(got, want, what):
    """The same bits where the reference is a number, a NaN where it is one."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.where(np.isnan(want), ~np.isnan(got), _bits(got) != _bits(want)) if got.dtype.kind == "f" else got != want
    assert not bad.any(), (what, int(bad.sum()), "values differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]))


def _raises(rt, code, fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-%d\)" % code):
        fn(*a, **kw)


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.set_glare(None), r.set_display(None)
    r.close()


_scenes = {}


def _scene(rt, name, aspect):
    if (name, aspect) not in _scenes:
        _scenes[name, aspect] = rt.Scene.build(name, aspect)
    return _scenes[name, aspect]


def _is_the_reference(got, want, what):
    """(img, index, est, info) of either call against the dict of select_ref.finish."""
    img, index, est, info = got
    _held(img, want["out"], (what, "out"))
    _same(index, want["index"], (what, "index"))
    _held(est, want["est"], (what, "est"))
    assert ref.info_matches(info, want["info"]), (what, info.as_dict(), want["info"])


# ---- 1. the hook against the reference ----------------------------------------------------------------------------------------------------------
def _hook(rt, r, ins, sel, first, done, counts, probe=None):
    return r.debug_denoise_select([ins[0][0], ins[1][0]], [(ins[0][1], ins[0][2]), (ins[1][1], ins[1][2])], sel, first, done, counts, probe)


def _hook_is_the_reference(rt, r, halves, first, done, counts, strengths, radius, patch, windows, what, Ks=None):
    """Every (S, T) of `windows` and every K of `Ks` over one set of candidates; the probes of every candidate once."""
    ins, nh = ref.state_inputs(halves, first, done if counts is None else counts)
    cands = ref.candidates(ins, nh, strengths, radius, patch)
    want = None
    for K in Ks or (len(strengths),):
        for S, T in windows:
            want = ref.finish(cands, S, T, K)
            sel = rt.make_select(strengths[:K], radius, patch, S, T)
            _is_the_reference(_hook(rt, r, ins, sel, first, done, counts), want, (what, K, S, T))
    K = len(strengths)
    for j in range(K):
        got = _hook(rt, r, ins, sel, first, done, counts, probe=j)
        _held(got[4], cands[0][j], (what, "out_j", j)), _held(got[5], cands[1][j], (what, "E_j", j))
    return want


@pytest.mark.parametrize("nx,rows", [(1, 1), (1, 7), (7, 1), (3, 2), (70, 19)])
def test_hook_on_frames_smaller_than_a_window_and_wider_than_a_tile(rt, ctx, nx, rows):
    want = _hook_is_the_reference(rt, ctx, halves_ref.plain_halves(nx, rows), 3, 16, None, KS, 5, 1, [(2, 1), (4, 4)], (nx, rows))
    assert want["info"]["usable"] == nx * rows


def test_hook_on_the_synthetic_halves(rt, ctx):
    halves, first, done, _ = ref.synthetic_halves()
    want = _hook_is_the_reference(rt, ctx, halves, first, done, None, KS, 5, 1, [(2, 1)], "synthetic")
    assert min(want["info"]["chosen"]) >= 0.05 * 64 * 48  # every candidate is in play (tests/test_select_host.py)


@pytest.mark.parametrize("counts", [False, True])
@pytest.mark.parametrize("patch", [0, 1, 2, 3])
@pytest.mark.parametrize("radius", [1, 5, 10])
def test_hook_on_37_x_21(rt, ctx, radius, patch, counts):
    """The kernel halves (a v = 0 block with exact ties, a NaN and a +inf pixel) or, with counts, the adaptive state with pixels of 0 .. 3
    samples: S, T in {0, 1, 4} and K in {2, 3, 4}."""
    if counts:
        halves, first, done, cnt, _ = ref.adaptive_state(7)
    else:
        (halves, first, done, _), cnt = ref.kernel_halves(), None
    windows = list(itertools.product((0, 1, 4), (0, 1, 4)))
    want = _hook_is_the_reference(rt, ctx, halves, first, done, cnt, KS, radius, patch, windows, (radius, patch, counts), Ks=(2, 3, 4))
    assert not want["usable"].all()


def test_hook_more_than_256_partial_sums(rt, ctx):
    want = _hook_is_the_reference(rt, ctx, halves_ref.extremes_halves(), 0, 16, None, (0.45, 1.0), 1, 0, [(2, 1)], "257 x 256")
    assert want["info"]["usable"] == 257 * 256 and all(np.isfinite(want["info"]["est_mse"]))


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("patch", [0, 1, 2, 3])
def test_plain_and_fused_chains_agree_in_every_bit(rt, ctx, patch, K):
    """k_denoise_multi<F, K> against 2 K launches of k_denoise<F>: every output and every probe, on the kernel halves (NaN, inf, v = 0),
    on the adaptive state with counts, at R 5 and at the largest window, and on a frame of several tiles with a partial one."""
    r = ctx
    cases = [(ref.kernel_halves()[0], 0, 16, None, 5), (ref.adaptive_state(7)[0], 7, 8, ref.adaptive_state(7)[3], 10), (halves_ref.plain_halves(70, 19), 3, 16, None, 2)]
    try:
        for halves, first, done, cnt, radius in cases:
            ins, _ = ref.state_inputs(halves, first, done if cnt is None else cnt)
            sel = rt.make_select(KS[:K], radius, patch, 2, 1)
            runs = {}
            for chain in ("plain", "fused"):
                r.debug_select_chain(chain)
                runs[chain] = [_hook(rt, r, ins, sel, first, done, cnt, probe=j) for j in range(K)]
            for j, (a, b) in enumerate(zip(runs["plain"], runs["fused"])):
                for x, y, k in zip(a[:3] + a[4:], b[:3] + b[4:], ("out", "index", "est", "out_j", "E_j")):
                    _same(x, y, (radius, patch, K, j, k))
                assert bytes(a[3]) == bytes(b[3]), (radius, patch, K, "info")
    finally:
        r.debug_select_chain("auto")
    with pytest.raises(rt.RtError, match="rt_debug_select_chain"):
        r.debug_select_chain(3)


# ---- 2. the product call on imported states -----------------------------------------------------------------------------------------------------
def _import_designed(rt, r, halves, first, done, counts=None, conv=None):
    """test_sphere at the frame's aspect, an accumulation with the state (sum = the sum of the halves) and the halves imported."""
    rows, nx = halves[0][1].shape
    scene = _scene(rt, "test_sphere", nx / rows)
    r.set_option("pixel_order", 0)
    r.upload(scene)
    prm = rt.make_params(nx, rows, 1, max_depth=8, seed=77)
    fid = rt.accum_frame_id(scene.camera, prm)
    with np.errstate(all="ignore"):
        total = (halves[0][0] + halves[1][0]).astype(np.float32)
        mom = np.stack([halves[0][1] + halves[1][1], halves[0][2] + halves[1][2]], -1)
    planes = accum_state_ref.COUNTS if counts is not None else 0
    st = rt.AccumState(nx, rows, first, done, planes, fid, sum=total, moments=mom, counts=counts, converged=conv)
    hs = rt.AccumHalves(nx, rows, first, done, fid, sum=np.stack([halves[0][0], halves[1][0]]),
                        moments=np.stack([np.stack([h[1], h[2]], -1) for h in halves]))
    assert st.check() and hs.check()
    r.accum_begin(scene.camera, prm, first_sample=first)
    r.accum_import(st)
    r.accum_import_halves(hs)
    return st, hs


def _product(r, sel, want_rgb8=True):
    img, rgb8, index, est, info = r.accum_denoise_select(sel, want_rgb8=want_rgb8)
    return (img, index, est, info), rgb8


STATES = {"synthetic": (ref.synthetic_halves, dict()), "kernel ties": (ref.kernel_halves, dict(radius=1, patch=1, S=1)),
          "adaptive 4": (lambda: ref.adaptive_state(4), dict()), "adaptive 7": (lambda: ref.adaptive_state(7), dict(T=0)),
          "blind": (ref.blind_state, dict()), "257 x 256": (lambda: (halves_ref.extremes_halves(), 0, 16, None), dict(strengths=(0.45, 1.0), radius=1, patch=0))}


@pytest.mark.parametrize("name", list(STATES))
def test_product_call_on_imported_states(rt, ctx, name):
    """Also: out_j IS rt_accum_denoise_halves at k_j, and with T = 0 pixel p of the result is pixel p of that call at k_{s(p)}, in every bit;
    the exported state and halves are what went in."""
    r = ctx
    make, kw = STATES[name]
    halves, first, done, cnt, conv = (make() + (None,))[:5]
    st, hs = _import_designed(rt, r, halves, first, done, cnt, conv)
    want = ref.select(halves, first, done if cnt is None else cnt, **kw)
    p = dict(dict(strengths=KS, radius=5, patch=1, S=2, T=1), **kw)
    sel = rt.make_select(p["strengths"], p["radius"], p["patch"], p["S"], p["T"])
    r.launched_variants(reset=True)
    got, rgb8 = _product(r, sel)
    assert not any(r.launched_variants(reset=True).values())
    print(f"{name}: {got[3].as_dict()}")
    _is_the_reference(got, want, name)
    _same(rgb8, want["rgb8"], (name, "rgb8"))
    # held to the cross filter that was there before
    single = [r.accum_denoise_halves(p["radius"], p["patch"], k)[0] for k in p["strengths"]]
    for j, img in enumerate(single):
        _held(img, want["outs"][j], (name, "rt_accum_denoise_halves at k_j against the reference's out_j", j))
    ins, _ = ref.state_inputs(halves, first, done if cnt is None else cnt)
    for j, img in enumerate(single):
        _same(_hook(rt, r, ins, sel, first, done, cnt, probe=j)[4], img, (name, "the probe's out_j against rt_accum_denoise_halves at k_j", j))
    sel0 = rt.make_select(p["strengths"], p["radius"], p["patch"], p["S"], 0)
    (img0, index0, _, _), _ = _product(r, sel0, False)
    picked = np.choose(index0[..., None], single)
    _same(img0, picked, (name, "T = 0: every pixel is rt_accum_denoise_halves at the chosen strength"))
    _same(index0, want["index"], (name, "the choice does not depend on T"))
    back, back_h = r.accum_export(), r.accum_export_halves()  # read, not changed
    _same(back.sum, st.sum, name), _same(back.moments, st.moments, name), _same(back_h.sum, hs.sum, name), _same(back_h.moments, hs.moments, name)
    r.accum_end()


# ---- 3. out_rgb8 through a display and a glare ----------------------------------------------------------------------------------------------------
def test_rgb8_goes_through_the_display_and_the_glare(rt, ctx):
    """out_rgb8 is the context's presentation of the f32 image the same call returns, as rt_accum_denoise_halves's is: the reference
    quantisation, the display (held to rt_debug_display over that image, which tests/test_display.py holds to its reference), the glare
    in front of it (rt_glare_image against tests/glare_ref.py, rt_debug_glare for the bytes).  The other outputs do not move."""
    r = ctx
    halves, first, done, _ = ref.synthetic_halves()
    _import_designed(rt, r, halves, first, done)
    glare, rg = rt.make_glare(0.25, 0.7, 0.0, 4), glare_ref.make(0.25, 0.7, 0.0, 4)
    disp = rt.make_display(1.5, curve="aces", transfer="gamma2", dither="bayer8")
    try:
        plain, plain8 = _product(r, None)
        img = plain[0]
        _same(plain8, denoise_ref.finalize_rgb8(img), "the reference quantisation")
        seen = [plain8]
        for what, g, d in (("display", None, disp), ("glare and display", glare, disp), ("glare", glare, None)):
            r.set_glare(g), r.set_display(d)
            got, rgb8 = _product(r, None)
            for a, b, k in zip(got[:3], plain[:3], ("out", "index", "est")):
                _held(a, b, (what, k, "moved"))
            assert bytes(got[3]) == bytes(plain[3]), what
            if g is not None:
                _same(r.glare_image(64, 48), glare_ref.glare(img, rg)[0], (what, "rt_glare_image behind the selection"))
                _same(rgb8, r.debug_glare(img, g, d)[1], (what, "rgb8"))
            else:
                _same(rgb8, r.debug_display(img, d)[0], (what, "rgb8"))
            h_img, h8, _, _ = r.accum_denoise_halves(want_rgb8=True)  # the same presentation as the cross filter's
            _same(h8, r.debug_glare(h_img, g, d)[1] if g is not None else r.debug_display(h_img, d)[0], (what, "rt_accum_denoise_halves's rgb8"))
            assert not any(np.array_equal(rgb8, x) for x in seen), (what, "changed nothing")
            seen.append(rgb8)
    finally:
        r.set_glare(None), r.set_display(None)
        r.accum_end()


# ---- 4. nothing else moves --------------------------------------------------------------------------------------------------------------------
def _everything(r):
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    st, hs = r.accum_export(), r.accum_export_halves()
    dh = r.accum_denoise_halves(want_rgb8=True, want_err=True)
    out = [("f32", img), ("rgb8", rgb8), ("sem", sem), ("noise", bytes(noise)), ("denoise halves", dh[0]), ("denoise halves rgb8", dh[1]),
           ("denoise halves err", dh[2]), ("residual", bytes(dh[3])), ("state sum", st.sum), ("state moments", st.moments), ("state counts", st.counts),
           ("state converged", st.converged), ("state scalars", repr((st.first_sample, st.done, st.planes, st.frame_id)).encode()),
           ("halves sum", hs.sum), ("halves moments", hs.moments)]
    for h in range(2):
        half = r.accum_half(h, want_sem=True)
        out += [(f"half {h}", half[0]), (f"half {h} sem", half[1])]
    return out


def _unchanged(now, kept, what):
    assert [k for k, _ in now] == [k for k, _ in kept]
    for (k, a), (_, b) in zip(now, kept):
        assert a == b if isinstance(a, bytes) else np.array_equal(_bits(a), _bits(b)), (what, k)


NX, NY = 20, 18


def _rendered(rt, r, n, adaptive=False, **shard):
    scene = _scene(rt, "test_sphere", NX / NY)
    r.set_option("pixel_order", 0)
    r.upload(scene)
    prm = rt.make_params(NX, NY, 4, seed=SEED, spp_slice=2, max_depth=50, **shard)
    r.accum_begin(scene.camera, prm, first_sample=7)
    r.accum_track_halves()
    for k in n:
        r.accum_add_adaptive(k, 0.3, 0.01, 3) if adaptive else r.accum_add(k)
    return scene, prm


@pytest.mark.parametrize("adaptive", [False, True])
def test_nothing_else_moves(rt, ctx, adaptive):
    r = ctx
    _rendered(rt, r, (3, 2, 4), adaptive)
    kept = _everything(r)
    r.launched_variants(reset=True)
    img, rgb8, index, est, info = r.accum_denoise_select(want_rgb8=True)
    assert not any(r.launched_variants(reset=True).values())  # no kernel of a ledger family
    assert np.isfinite(img).all() and info.usable > 0 and sum(info.chosen) == NX * NY
    _unchanged(_everything(r), kept, "after rt_accum_denoise_select")
    r.accum_add_adaptive(1, 0.3, 0.01, 3) if adaptive else r.accum_add(1)  # and the accumulation goes on
    r.accum_end()


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(rt, ctx):
    r, f = ctx, rt._ffi
    fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    img, rgb8 = np.full((NY, NX, 3), 7.0, np.float32), np.full((NY, NX, 3), 9, np.uint8)
    index, est, info = np.full((NY, NX), 5, np.uint8), np.full((NY, NX), 3.0, np.float32), f.RtSelectInfo()
    info.best, info.usable, info.est_mse[0] = 77, 78, 79.0

    def call(sel=None):
        return r._lib.rt_accum_denoise_select(r._ctx, C.byref(sel) if sel is not None else None, img.ctypes.data_as(fp), rgb8.ctypes.data_as(u8p),
                                              index.ctypes.data_as(u8p), est.ctypes.data_as(fp), C.byref(info))

    def untouched(what):
        assert (img == 7.0).all() and (rgb8 == 9).all() and (index == 5).all() and (est == 3.0).all(), what
        assert (info.best, info.usable, info.est_mse[0]) == (77, 78, 79.0), what

    r.accum_end()
    assert call() == -f.ERR_STATE  # no accumulation
    scene, prm = _rendered(rt, r, ())
    r.accum_begin(scene.camera, prm)
    r.accum_add(4)
    assert call() == -f.ERR_STATE  # no tracking
    untouched("no accumulation, no tracking")
    _rendered(rt, r, (3,))
    assert call() == -f.ERR_STATE  # three samples: a half holds one
    untouched("three samples")
    r.accum_add(1)
    kept = _everything(r)
    bads = [dict(strengths=[0.5]), dict(strengths=[0.7, 0.7]), dict(strengths=[1.0, 0.5]), dict(strengths=[0.0, 1.0]), dict(strengths=[0.5, float("nan")]),
            dict(strengths=[0.5, float("inf")]), dict(radius=0), dict(radius=f.DENOISE_MAX_RADIUS + 1), dict(patch=f.DENOISE_MAX_PATCH + 1),
            dict(error_radius=f.SELECT_MAX_WINDOW + 1), dict(blend_radius=f.SELECT_MAX_WINDOW + 1)]
    for bad in bads:
        assert call(rt.make_select(**bad)) == -f.ERR_INVALID, bad
    sel = rt.make_select()
    sel.reserved = 1
    assert call(sel) == -f.ERR_INVALID
    sel = rt.make_select()
    sel.n_strengths = 5
    assert call(sel) == -f.ERR_INVALID
    untouched("invalid parameters")
    _unchanged(_everything(r), kept, "after the refusals")
    assert r._lib.rt_accum_denoise_select(r._ctx, None, None, None, None, None, None) == 0  # every output may be NULL
    assert call() == 0 and (index < 4).all() and info.best < 4 and info.usable > 0  # and the same call succeeds
    want = r.accum_denoise_select(rt.make_select(), want_rgb8=True)  # NULL is the defaults written out
    _same(img, want[0], "NULL against the explicit defaults"), _same(rgb8, want[1], "rgb8"), _same(index, want[2], "index"), _held(est, want[3], "est")
    assert bytes(info) == bytes(want[4])
    r.accum_end()
    # a sharded frame
    img[:], rgb8[:], index[:], est[:] = 7.0, 9, 5, 3.0
    info.best, info.usable, info.est_mse[0] = 77, 78, 79.0
    _rendered(rt, r, (4,), shard_count=2, shard_band=4, shard_id=1)
    assert call() == -f.ERR_UNSUPPORTED
    untouched("a sharded frame")
    r.accum_end()
    # the hook's refusals
    ins, _ = ref.state_inputs(halves_ref.plain_halves(3, 2), 0, 16)
    _raises(rt, f.ERR_INVALID, _hook, rt, r, ins, rt.make_select(strengths=[0.5, 1.0]), 0, 16, None, 2)  # probe_candidate >= K
    _raises(rt, f.ERR_INVALID, _hook, rt, r, ins, rt.make_select(radius=0), 0, 16, None)
    assert r._lib.rt_debug_denoise_select(r._ctx, 3, 2, None, None, None, None, None, 0, 16, None, None, None, None, None, 0, None, None) == -f.ERR_INVALID


# ---- 6. the joined context of an RtMulti ----------------------------------------------------------------------------------------------------------
def test_joined_context_equals_the_single_one(rt, ctx):
    nx, ny = 24, 27
    scene = _scene(rt, "sphere_scene", nx / ny)
    prm = lambda band: rt.make_params(nx, ny, 4, max_depth=8, seed=SEED, spp_slice=3, shard_band=band)
    r = ctx
    r.set_option("pixel_order", 0)
    r.upload(scene)
    r.accum_begin(scene.camera, prm(0), first_sample=7)
    r.accum_track_halves()
    r.accum_add(4), r.accum_add(2)
    want = r.accum_denoise_select(want_rgb8=True)
    r.accum_end()
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.accum_begin(scene.camera, prm(8), first_sample=7, halves=True)
        m.accum_add(4), m.accum_add(2)
        j = m.accum_join()
        got = j.accum_denoise_select(want_rgb8=True)
        assert not any(j.launched_variants().values())
        m.accum_end()
    finally:
        m.close()
    for a, b, k in zip(got[:4], want[:4], ("out", "rgb8", "index", "est")):
        _held(a, b, ("joined", k))
    assert bytes(got[4]) == bytes(want[4]) and want[4].usable == nx * ny


def test_render_py_select_flags_and_map_out(rt, ctx, tmp_path):
    """render.py --denoise --denoise-guide halves --denoise-select .. --select-map-out: the PNG and the maps are what the library call gives."""
    from PIL import Image
    png, maps = str(tmp_path / "frame.png"), str(tmp_path / "maps.npz")
    c = subprocess.run([sys.executable, "-m", "ray_tracing_in_one_weekend_amd.render", "--scene", "test_sphere", "--nx", "40", "--ny", "30", "--spp", "8", "--denoise",
                        "--denoise-guide", "halves", "--denoise-select", "0.45,1.0", "--select-error-radius", "1", "--select-blend-radius", "2", "--denoise-radius", "3",
                        "--out", png, "--select-map-out", maps], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    assert "frame-wide best" in c.stderr
    r = ctx
    scene = rt.Scene.build("test_sphere", 40 / 30)
    r.set_option("pixel_order", 0)
    r.upload(scene)
    r.accum_begin(scene.camera, rt.make_params(40, 30, 8))
    r.accum_track_halves()
    r.accum_add(8)
    _, rgb8, index, est, _ = r.accum_denoise_select(rt.make_select((0.45, 1.0), 3, 1, 1, 2), want_rgb8=True)
    r.accum_end()
    assert np.array_equal(np.asarray(Image.open(png).convert("RGB"), np.uint8), rgb8)
    with np.load(maps) as z:
        _same(z["index"], index[::-1], "index map"), _held(z["est"], est[::-1], "est map")
        assert [float(k) for k in z["strengths"]] == [float(np.float32(0.45)), 1.0]
    bad = subprocess.run([sys.executable, "-m", "ray_tracing_in_one_weekend_amd.render", "--scene", "test_sphere", "--nx", "8", "--ny", "6", "--spp", "8", "--denoise",
                          "--denoise-guide", "halves", "--denoise-select", "1.0,0.45", "--out", png], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--denoise-select" in bad.stderr


# ---- 7. rendered frames -----------------------------------------------------------------------------------------------------------------------
# cornell_box 64 x 64, depth 8, 16 spp, against rt_render at 4 096 spp with another seed (the two bit-reproducible frames of
# tests/test_halves.py), R 5, F 1.  Measured on an MI355X, RMSE of the linear radiance:
#   with Scene.lights: 16 spp 0.17207; rt_accum_denoise_halves at 0.45 / 0.7 / 1.0 / 1.4: 0.09132 / 0.07848 / 0.07084 / 0.07490;
#                      selected from all four with S 2, T 1: 0.07703; with the defaults (0.7, 1.0, 1.4; S 0, T 1): 0.07078
#   without          : 16 spp 0.25412; 0.10343 / 0.09295 / 0.09252 / 0.09701; from all four 0.09476; with the defaults 0.08995
# The defaults are the one choice of scripts/select_defaults.py that is more than 5 % better than (four candidates, S 2, T 1) on both frames.
# MEASURED ratio = RMSE(selected at the defaults) / RMSE(16 spp), rounded up in the fourth digit (the frames are bit-reproducible);
# best = RtSelectInfo.best at the defaults, an index into (0.7, 1.0, 1.4): the truly best candidate with the lights, the second best
# (0.5 % behind in RMSE) without.
MEASURED = {"lights": dict(ratio=0.4114, best=1), "no_lights": dict(ratio=0.3540, best=0)}
_truth = {}


def _lum_mse(a, b):
    d = halves_ref.lum32(a).astype(np.float64) - halves_ref.lum32(b).astype(np.float64)
    return float(np.mean(d * d))


@pytest.mark.parametrize("which", ["lights", "no_lights"])
def test_rendered_frames(rt, ctx, which):
    r = ctx
    scene = _scene(rt, "cornell_box", 1.0)
    r.set_option("pixel_order", 0)
    r.upload(scene)
    if which == "lights":
        r.set_lights(scene.lights)
    try:
        if which not in _truth:
            _truth[which] = r.render(scene.camera, rt.make_params(64, 64, 4096, max_depth=8, seed=SEED + 1))[0]
        truth = _truth[which]
        r.accum_begin(scene.camera, rt.make_params(64, 64, 16, max_depth=8, seed=SEED))
        r.accum_track_halves()
        r.accum_add(16)
        e_noisy = denoise_ref.rmse(r.accum_read()[0], truth)
        img, _, index, est, info = r.accum_denoise_select()
        e_sel = denoise_ref.rmse(img, truth)
        img4, _, _, _, info4 = r.accum_denoise_select(rt.make_select(KS, 5, 1, 2, 1))
        e_single = [denoise_ref.rmse(r.accum_denoise_halves(strength=k)[0], truth) for k in KS]
        hs = r.accum_export_halves()
        halves = [(hs.sum[h], hs.moments[h][..., 0], hs.moments[h][..., 1]) for h in range(2)]
        ins, _ = ref.state_inputs(halves, 0, 16)
        half_mse = [0.5 * sum(_lum_mse(r.debug_denoise(ins[h][0], ins[1 - h][1], ins[1 - h][2], 5, 1, k), truth) for h in range(2)) for k in KS]
        r.accum_end()
    finally:
        r.set_lights(None)
    print(f"{which}: RMSE 16 spp {e_noisy:.5f}; selected at the defaults {e_sel:.5f} (ratio {e_sel / e_noisy:.7f}), best {info.best}, chosen {list(info.chosen)}; "
          f"selected from {KS} with S 2, T 1: {denoise_ref.rmse(img4, truth):.5f}; rt_accum_denoise_halves at {KS}: " + " / ".join(f"{e:.5f}" for e in e_single))
    print(f"{which}: est_mse of {KS} " + " / ".join(f"{e:.6f}" for e in info4.est_mse) + "; true luminance MSE of the half filters " + " / ".join(f"{e:.6f}" for e in half_mse) +
          f"; est_mse_selected {info4.est_mse_selected:.6f}; best {info4.best}, truly best half filter {int(np.argmin(half_mse))}, truly best combined {int(np.argmin(e_single))}; "
          f"chosen {list(info4.chosen)}, usable {info4.usable}")
    assert np.isfinite(img).all() and info.usable == 64 * 64 == info4.usable
    assert list(info.est_mse)[:3] == list(info4.est_mse)[1:]  # a candidate's figure does not depend on the others
    assert e_sel / e_noisy <= MEASURED[which]["ratio"]
    assert info.best == MEASURED[which]["best"]
