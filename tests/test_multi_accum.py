"""Progressive accumulation across the contexts of a MultiRenderer (rt_multi_accum_*), on one GPU through MultiRenderer([0] * n,
copy_gather=True).  Everything is bit for bit: the join of imported designed planes against the planes themselves
(tests/multi_accum_ref.py), and everything the joined context returns against ONE Renderer over the frame after the same adds.

Geometries, the smallest at which the row and tile arithmetic takes another path: 24 x 27 / band 8 / n 2 (a shard of 11 rows: tiles and a
tail inside the shard, the frame tiles and a 3-row tail); 16 x 11 / 8 / 3 (a partial band and a shard with no row); 7 x 3 / 1 / 2
(alternating rows, no tiles); 1 x 1 / n 2 (one pixel, one shard empty); 24 x 13 / n 1 (a single shard).

The adaptive settings are those of tests/test_halves.py (tolerance 0.3, floor 0.01, min_samples 3)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import multi_accum_ref as mref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(24, 27, 8, 2), (16, 11, 8, 3), (7, 3, 1, 2), (1, 1, 0, 2), (24, 13, 0, 1)]
SEED, FIRST = 1234, 7
TOL, FLOOR, MIN = 0.3, 0.01, 3
UNIFORM, ADAPTIVE = (4, 2), (4, 4)  # the first add gives each half two samples: every filter runs after every add
ALL = dict(channels=True, halves=True, buckets=3)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), "values differ")


def _all_same(got, want, what):
    assert [k for k, _ in got] == [k for k, _ in want], what
    for (k, a), (_, b) in zip(got, want):
        if isinstance(a, (bytes, tuple)):
            assert a == b, (what, k, a, b)
        else:
            _same(a, b, (what, k))


def _raises(rt, code, fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-%d\)" % code):
        fn(*a, **kw)


_multis, _scenes = {}, {}


@pytest.fixture(scope="module")
def multi(rt):
    """MultiRenderer([0] * n, copy_gather=True), one per n for the whole module."""
    def get(n):
        if n not in _multis:
            _multis[n] = rt.MultiRenderer([0] * n, copy_gather=True)
        return _multis[n]
    yield get
    for m in _multis.values():
        m.close()
    _multis.clear()


@pytest.fixture(scope="module")
def single(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


def _scene(rt, name, nx, ny):
    if (name, nx, ny) not in _scenes:
        _scenes[name, nx, ny] = rt.Scene.build(name, nx / ny)
    return _scenes[name, nx, ny]


def _params(rt, nx, ny, band, spp=4, **kw):
    return rt.make_params(nx, ny, spp, **{"max_depth": 8, "seed": SEED, "spp_slice": 3, "shard_band": band, **kw})


def _snapshots(r, tracked):
    """The exported state, halves and buckets of the open accumulation of `r` as (name, array or tuple of scalars)."""
    st = r.accum_export()
    out = [("state scalars", (st.nx, st.rows, st.first_sample, st.done, st.planes, st.frame_id)), ("state sum", st.sum), ("state moments", st.moments),
           ("state counts", st.counts), ("state converged", st.converged)]
    if tracked:
        hs, bs = r.accum_export_halves(), r.accum_export_buckets()
        out += [("state channel moments", st.channel_moments), ("halves scalars", (hs.nx, hs.rows, hs.first_sample, hs.done, hs.frame_id)), ("halves sum", hs.sum),
                ("halves moments", hs.moments), ("buckets scalars", (bs.nx, bs.rows, bs.first_sample, bs.done, bs.M, bs.frame_id)), ("buckets sum", bs.sum)]
    return out


def _everything(r, tracked):
    """Everything an accumulation returns: the snapshots, the image, rgb8, sem and the three frame figures, counts and RtAdaptiveInfo, and
    with tracking the channel sem, both half images, the robust read-out with its info and all five filters (else the two that need none)."""
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    counts, info = r.accum_counts()
    out = _snapshots(r, tracked) + [("f32", img), ("rgb8", rgb8), ("sem", sem), ("noise", bytes(noise)), ("counts", counts), ("info", bytes(info))]
    dn = r.accum_denoise(want_rgb8=True)
    out += [("denoise", dn[0]), ("denoise rgb8", dn[1]), ("denoise multiscale", r.accum_denoise_multiscale(levels=2)[0])]
    if tracked:
        out += [("channel sem", r.accum_channel_sem()), ("denoise channels", r.accum_denoise_channels()[0]),
                ("denoise multiscale channels", r.accum_denoise_multiscale(levels=2, guide="channels")[0])]
        dh = r.accum_denoise_halves(want_rgb8=True, want_err=True)
        out += [("denoise halves", dh[0]), ("denoise halves rgb8", dh[1]), ("denoise halves err", dh[2]), ("residual", bytes(dh[3]))]
        for h in range(2):
            half = r.accum_half(h, want_sem=True)
            out += [("half %d" % h, half[0]), ("half %d sem" % h, half[1])]
        rb = r.accum_robust("gini", want_trim=True, want_rgb8=True)
        out += [("robust", rb[0]), ("robust info", bytes(rb[1])), ("robust trim", rb[2]), ("robust rgb8", rb[3]),
                ("denoise robust", r.accum_denoise_robust("median")[0])]
    return out


def _begin_single(r, scene, prm, tracked, first=FIRST):
    r.accum_begin(scene.camera, prm, first_sample=first)
    if tracked:
        r.accum_track_channels(), r.accum_track_halves(), r.accum_track_buckets(3)


def _adds(r):
    for n in UNIFORM:
        yield ("uniform", n), r.accum_add(n)
    for n in ADAPTIVE:
        yield ("adaptive", n), r.accum_add_adaptive(n, TOL, FLOOR, MIN)


# ---- 1. round trip on designed bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,band,n", GEOMETRIES)
def test_import_join_export_is_the_identity_on_designed_bits(rt, multi, nx, ny, band, n):
    """A whole-frame snapshot of designed bits — counts and flags, channel moments, halves, 3 and 16 buckets, every value distinct, NaNs
    with payloads, both infinities, -0.0 — imported over n shards, joined and exported from the joined context: every plane the input as
    bytes, every scalar field the whole frame's."""
    m = multi(n)
    scene = _scene(rt, "test_sphere", nx, ny)
    m.upload(scene)
    prm = _params(rt, nx, ny, band)
    whole_prm = _params(rt, nx, ny, 0)
    fid = rt.accum_frame_id(scene.camera, whole_prm)
    for M in (3, 16):
        w = mref.designed(nx, ny, first_sample=5, done=9, M=M, seed=M, frame_id=fid)
        state = rt.AccumState(nx, ny, 5, 9, w["planes"], fid, w["sum"], w["moments"], w["counts"], w["converged"], w["channel_moments"])
        halves = rt.AccumHalves(nx, ny, 5, 9, fid, w["halves"]["sum"], w["halves"]["moments"])
        buckets = rt.AccumBuckets(nx, ny, M, 5, 9, fid, w["buckets"])
        assert state.check() and halves.check() and buckets.check()
        m.accum_begin(scene.camera, prm, first_sample=5)
        m.accum_import(state, halves, buckets)
        j = m.accum_join()
        st, hs, bs = j.accum_export(), j.accum_export_halves(), j.accum_export_buckets()
        assert (st.nx, st.rows, st.first_sample, st.done, st.planes, st.frame_id) == (nx, ny, 5, 9, w["planes"], fid)
        assert (hs.nx, hs.rows, hs.first_sample, hs.done, hs.frame_id) == (nx, ny, 5, 9, fid)
        assert (bs.nx, bs.rows, bs.first_sample, bs.done, bs.M, bs.frame_id) == (nx, ny, 5, 9, M, fid)
        for name in ("sum", "moments", "counts", "converged", "channel_moments"):
            assert getattr(st, name).tobytes() == w[name].tobytes(), (M, name)
        assert hs.sum.tobytes() == w["halves"]["sum"].tobytes() and hs.moments.tobytes() == w["halves"]["moments"].tobytes(), M
        assert bs.sum.tobytes() == w["buckets"].tobytes(), M
        assert not any(j.launched_variants().values())
        m.accum_end()


# ---- 2. equal to one context ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("scene_name", ["sphere_scene", "cornell_box"])  # tiles by default; a general scene: rows by default
@pytest.mark.parametrize("nx,ny,band,n", GEOMETRIES[:2])
def test_joined_context_is_one_context(rt, multi, single, nx, ny, band, n, scene_name, tracked):
    """The same uniform and then adaptive adds on a Renderer and on the MultiRenderer, first_sample 7; after EVERY add the joined context
    returns what the Renderer returns: every exported plane, image, rgb8, sem, the frame figures, counts and RtAdaptiveInfo, channel sem,
    all five filters, both half images and the robust read-out with its info.  The ledger of the joined context stays empty."""
    m = multi(n)
    scene = _scene(rt, scene_name, nx, ny)
    m.upload(scene), single.upload(scene)
    assert bool(single.scene_info()["general_kernels"]) == (scene_name == "cornell_box")
    _begin_single(single, scene, _params(rt, nx, ny, 0), tracked)
    m.accum_begin(scene.camera, _params(rt, nx, ny, band), first_sample=FIRST, **(ALL if tracked else {}))
    for (step, st1), (_, stn) in zip(_adds(single), _adds(m)):
        assert (st1.n_paths, st1.n_rays, list(st1.rays_per_depth)) == (stn.n_paths, stn.n_rays, list(stn.rays_per_depth)), step
        j = m.accum_join()
        assert not any(j.launched_variants().values()), step
        _all_same(_everything(j, tracked), _everything(single, tracked), (step, n))
        assert not any(j.launched_variants().values()), step
    conv = single.accum_export().converged
    print(f"{scene_name} {nx}x{ny}: {int(conv.sum())} of {conv.size} pixels converged")
    assert 0 < conv.sum() < conv.size  # some pixels stopped and some went on: else the adaptive adds show nothing
    single.accum_end(), m.accum_end()


# ---- 3. independence of n and band ----------------------------------------------------------------------------------------------------------
def test_joined_planes_do_not_depend_on_n_and_band(rt, multi):
    nx, ny = 24, 27
    scene = _scene(rt, "sphere_scene", nx, ny)
    want = None
    for n in (1, 2, 3):
        m = multi(n)
        m.upload(scene)
        for band in (1, 4, 8):
            m.accum_begin(scene.camera, _params(rt, nx, ny, band), first_sample=FIRST, **ALL)
            m.accum_add(6), m.accum_add_adaptive(4, TOL, FLOOR, MIN)
            got = _snapshots(m.accum_join(), True)
            m.accum_end()
            if want is None:
                want = got
            _all_same(got, want, (n, band))
    assert 0 < dict(want)["state converged"].sum() < nx * ny


# ---- 4. resume ---------------------------------------------------------------------------------------------------------------------------------
def test_resume_on_another_number_of_devices_and_on_one_context(rt, multi, single):
    nx, ny, band = 24, 27, 8
    scene = _scene(rt, "sphere_scene", nx, ny)
    for r in (multi(2), multi(3), single):
        r.upload(scene)
    prm = _params(rt, nx, ny, band)
    m = multi(2)
    m.accum_begin(scene.camera, prm, first_sample=FIRST, **ALL)
    m.accum_add(4), m.accum_add(2)
    j = m.accum_join()
    state, halves, buckets = j.accum_export(), j.accum_export_halves(), j.accum_export_buckets()
    assert (state.done, state.rows, halves.done, buckets.M) == (6, ny, 6, 3) and state.frame_id == rt.accum_frame_id(scene.camera, _params(rt, nx, ny, 0))

    def go_on(r):
        r.accum_add_adaptive(4, TOL, FLOOR, MIN), r.accum_add_adaptive(4, TOL, FLOOR, MIN)
    go_on(m)
    uninterrupted = _everything(m.accum_join(), True)
    m.accum_end()
    # three devices, another band
    m3 = multi(3)
    m3.accum_begin(scene.camera, _params(rt, nx, ny, 4), first_sample=FIRST)
    m3.accum_import(state, halves, buckets)
    got = m3.accum_join().accum_export()  # right after the import: the state that went in
    assert (got.done, got.planes, got.frame_id) == (state.done, state.planes, state.frame_id)
    for name in ("sum", "moments", "channel_moments"):
        _same(getattr(got, name), getattr(state, name), ("right after the import", name))
    go_on(m3)
    _all_same(_everything(m3.accum_join(), True), uninterrupted, "resumed on three devices")
    m3.accum_end()
    # one context, through the single-context imports
    single.accum_begin(scene.camera, _params(rt, nx, ny, 0), first_sample=FIRST)
    single.accum_import(state), single.accum_import_halves(halves), single.accum_import_buckets(buckets)
    go_on(single)
    _all_same(_everything(single, True), uninterrupted, "resumed on one context")
    # and the run that never stopped, on one context
    _begin_single(single, scene, _params(rt, nx, ny, 0), True)
    single.accum_add(4), single.accum_add(2)
    go_on(single)
    _all_same(_everything(single, True), uninterrupted, "one context, uninterrupted")
    single.accum_end()


# ---- 5. the mirror and the refusals ---------------------------------------------------------------------------------------------------------
def test_the_joined_context_is_a_mirror(rt, multi, single):
    nx, ny, band = 16, 11, 8
    f = rt._ffi
    scene = _scene(rt, "sphere_scene", nx, ny)
    m = multi(3)
    m.upload(scene), single.upload(scene)
    prm, whole = _params(rt, nx, ny, band), _params(rt, nx, ny, 0)
    _begin_single(single, scene, whole, True)
    m.accum_begin(scene.camera, prm, first_sample=FIRST, **ALL)
    single.accum_add(4), m.accum_add(4)
    j = m.accum_join()
    assert m.accum_join()._ctx.value == j._ctx.value  # the same context for the life of the MultiRenderer
    state, halves, buckets = j.accum_export(), j.accum_export_halves(), j.accum_export_buckets()
    before = _everything(j, True)
    for call in (lambda: j.accum_begin(scene.camera, whole), lambda: j.accum_add(2), lambda: j.accum_add_adaptive(2, TOL, FLOOR, MIN),
                 lambda: j.accum_import(state), lambda: j.accum_import_halves(halves), lambda: j.accum_import_buckets(buckets),
                 lambda: j.accum_merge(state), j.accum_track_channels, j.accum_track_halves, lambda: j.accum_track_buckets(3), j.accum_end):
        with pytest.raises(rt.RtError, match=r"\(-%d\).*mirror" % f.ERR_STATE):
            call()
    _all_same(_everything(j, True), before, "after the refused calls")
    # rt_multi_render between two adds leaves the accumulation alone (and renders the frame of one context)
    img = m.render(scene.camera, _params(rt, nx, ny, band, spp=3))[0]
    _same(img, single.render(scene.camera, _params(rt, nx, ny, 0, spp=3))[0], "rt_multi_render in between")
    single.accum_add_adaptive(3, TOL, FLOOR, MIN), m.accum_add_adaptive(3, TOL, FLOOR, MIN)
    _all_same(_everything(m.accum_join(), True), _everything(single, True), "after the refusals and a render")
    # refused arguments change nothing
    _raises(rt, f.ERR_INVALID, m.accum_add_adaptive, 2, -1.0, FLOOR, MIN)
    _raises(rt, f.ERR_INVALID, m.accum_add_adaptive, 0, TOL, FLOOR, MIN)
    _raises(rt, f.ERR_STATE, m.accum_add, 2)  # a uniform add behind an adaptive one, as on one context
    _raises(rt, f.ERR_UNSUPPORTED, m.accum_import, state)  # rt_accum_import on shards that track halves, as on one context
    _all_same(_everything(m.accum_join(), True), _everything(single, True), "after the refused adds")
    m.accum_end(), single.accum_end()
    # after the end: the joined context reads nothing, join and import are refused, end is not
    _raises(rt, f.ERR_STATE, j.accum_read)
    _raises(rt, f.ERR_STATE, m.accum_join)
    _raises(rt, f.ERR_STATE, m.accum_import, state)
    _raises(rt, f.ERR_STATE, m.accum_add, 1)
    m.accum_end()
    # begin: an unknown track bit and M out of range, before any device is touched
    lib, cam = m._lib, scene.camera
    import ctypes as C
    for track, M in ((8, 0), (f.MULTI_TRACK_BUCKETS, 2), (f.MULTI_TRACK_BUCKETS, 17), (f.MULTI_TRACK_BUCKETS | 16, 3)):
        assert lib.rt_multi_accum_begin(m._m, C.byref(cam), C.byref(prm), 0, track, M) == -f.ERR_INVALID
        _raises(rt, f.ERR_STATE, m.accum_join)  # nothing was begun
    assert lib.rt_multi_accum_begin(m._m, C.byref(cam), C.byref(prm), 0, f.MULTI_TRACK_CHANNELS, 99) == 0  # (M is not looked at without the bit)
    # an import that does not fit the frame is refused whole; a state of another frame, halves of another window
    fresh = rt.AccumState(nx, ny, FIRST, 4, 0, state.frame_id ^ 1, state.sum, state.moments)
    _raises(rt, f.ERR_INVALID, m.accum_import, fresh)
    m.accum_begin(scene.camera, prm, first_sample=FIRST)
    _raises(rt, f.ERR_INVALID, m.accum_import, state, rt.AccumHalves(nx, ny, FIRST, 5, state.frame_id, halves.sum, halves.moments))
    m.accum_import(state, halves, buckets)  # (the refusals left the fresh accumulation as it was)
    _all_same(_everything(m.accum_join(), True), before, "imported after the refusals")
    m.accum_end()


def test_calls_before_begin_are_refused(rt):
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        for call in (lambda: m.accum_add(1), lambda: m.accum_add_adaptive(1, TOL, FLOOR, MIN), m.accum_join):
            _raises(rt, rt._ffi.ERR_STATE, call)
        m.accum_end()
    finally:
        m.close()


# ---- 7. render.py ----------------------------------------------------------------------------------------------------------------------------
def _render_py(*args):
    cmd = [sys.executable, "-m", "ray_tracing_in_one_weekend_amd.render", "--scene", "sphere_scene", "--nx", "24", "--ny", "27", "--max-depth", "8", "--seed", "7",
           "--spp-step", "4", "--adaptive-tolerance", TOL, "--min-spp", MIN, "--denoise", *args]
    p = subprocess.run([str(a) for a in cmd], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p


def test_render_py_on_devices(rt, tmp_path):
    """--devices 0,0 --copy-gather writes the PNG bytes and the checkpoint planes of --device 0; its checkpoint, stopped early, resumed on
    --devices 0,0,0 ends on the image of the uninterrupted run."""
    one, two, part, resumed = (tmp_path / n for n in ("one.png", "two.png", "part.png", "resumed.png"))
    ck1, ck2, ckp = (tmp_path / n for n in ("one.npz", "two.npz", "part.npz"))
    _render_py("--spp", 12, "--device", 0, "--checkpoint", ck1, "--out", one)
    _render_py("--spp", 12, "--devices", "0,0", "--copy-gather", "--checkpoint", ck2, "--out", two)
    assert open(two, "rb").read() == open(one, "rb").read()
    a, b = rt.AccumState.load(str(ck1)), rt.AccumState.load(str(ck2))
    assert (a.nx, a.rows, a.first_sample, a.done, a.planes, a.frame_id) == (b.nx, b.rows, b.first_sample, b.done, b.planes, b.frame_id)
    assert a.planes & rt._ffi.ACCUM_STATE_COUNTS and 0 < a.converged.sum() < a.converged.size
    for name in ("sum", "moments", "counts", "converged"):
        _same(getattr(a, name), getattr(b, name), ("checkpoint", name))
    _render_py("--spp", 8, "--devices", "0,0", "--copy-gather", "--checkpoint", ckp, "--out", part)
    assert rt.AccumState.load(str(ckp)).done == 8 and open(part, "rb").read() != open(one, "rb").read()
    p = _render_py("--spp", 12, "--devices", "0,0,0", "--copy-gather", "--resume", ckp, "--out", resumed)
    assert "12/12" in p.stderr and "8/12" not in p.stderr
    assert open(resumed, "rb").read() == open(one, "rb").read()
    _render_py("--spp", 12, "--device", 0, "--resume", ckp, "--out", resumed)  # and on one context with plain --resume
    assert open(resumed, "rb").read() == open(one, "rb").read()
