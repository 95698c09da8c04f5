"""The pixel reconstruction filters on the GPU (rt_accum_track_filter, rt_accum_read_filtered, rt_accum_export_filter, rt_accum_import_filter,
rt_debug_filter_add): the plane and the read-out of rendered accumulations against tests/filter_ref.py over their single-sample frames,
bit for bit; the box identity; the footprint of designed radiance; slice and add invariance; adaptive adds; the fallback of the read-out;
resume; everything else an accumulation returns unchanged with tracking on; the errors of the header; and the presentation of out_rgb8."""
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_ref as ref
from helpers import STATS_COUNTERS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 1234
NX, NY = 24, 13
f32 = np.float32
# nx, ny (tests/frame_cases.py says why these): a single pixel; row-major under a chunk, no tiles; tiles plus a 3-row tail; tiles plus a
# tail where a chunk straddles samples
SHAPES = {"1x1": (1, 1), "7x3": (7, 3), "16x11": (16, 11), "24x13": (NX, NY)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = _bits(a) != _bits(b)
    assert not bad.any(), (what, int(bad.sum()), "values differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]))


def _held(got, want, what):
    """The same bits where the reference is a number, a NaN where it is one."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.where(np.isnan(want), ~np.isnan(got), _bits(got) != _bits(want))
    assert not bad.any(), (what, int(bad.sum()), "values differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]))


def _raises(rt, code, fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-%d\)" % code):
        fn(*a, **kw)


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.set_option("pixel_order", 0)
    r.set_display(None), r.set_glare(None)
    r.close()


@pytest.fixture(scope="module")
def ctx2(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


_scenes, _single = {}, {}


def _setup(rt, r, shape="24x13", po=0, **more):
    nx, ny = SHAPES[shape]
    if shape not in _scenes:
        _scenes[shape] = rt.Scene.build("test_sphere", nx / ny)
    r.set_option("pixel_order", po)
    r.upload(_scenes[shape])
    return _scenes[shape], lambda spp, **kw: rt.make_params(nx, ny, spp, **{"seed": SEED, "spp_slice": 2, "max_depth": 50, **more, **kw})


def _singles(r, scene, prm, shape, lo, hi):
    """x[i], lo <= i < hi: the frame of the sample with the absolute index i, from a one-sample accumulation each (sum = 0 + x_i); computed
    once and never changed."""
    have = _single.setdefault(shape, {})
    for i in range(lo, hi):
        if i not in have:
            r.accum_begin(scene.camera, prm(1), first_sample=i)
            r.accum_add(1)
            img = r.accum_export().sum
            img.setflags(write=False)
            have[i] = img
    r.accum_end()
    return [have[i] for i in range(lo, hi)]


def _reference(rt, flt, x, first, shape="24x13", plane=None, i0=None, active=None):
    nx, ny = SHAPES[shape]
    table, D = rt.pixel_filter_table(flt)
    plane = ref.new_plane(nx, ny) if plane is None else plane
    return ref.add_samples(plane, x, first if i0 is None else i0, SEED, table, flt.radius, D, active)


def _plane_is(rt, r, flt, want, first, n, what, acc_sum=None, counts=None):
    """The exported plane and the read-out against the reference plane `want`."""
    got = r.accum_export_filter()
    assert (got.nx, got.rows, got.first_sample, got.done) == (want.shape[1], want.shape[0], first, n) and got.check(), what
    assert bytes(got.filter) == bytes(flt), what
    _held(got.plane, want, (what, "plane"))
    acc_sum = r.accum_export().sum if acc_sum is None else acc_sum
    c, W = ref.read_out(want, acc_sum, n if counts is None else counts)
    img, _, w = r.accum_filtered(want_weight=True)
    _held(img, c, (what, "filtered image"))
    _held(w, W, (what, "weight"))
    return got


# ---- 1. the defining property -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("first", [0, 7])
def test_plane_is_the_in_order_gather_of_the_header(rt, ctx, first, kind):
    r = ctx
    flt = rt.make_pixel_filter(kind)
    for shape, orders in (("24x13", (1, 2)), ("16x11", (2,)), ("7x3", (0,)), ("1x1", (0,))):
        for po in orders:
            scene, prm = _setup(rt, r, shape, po)
            x = _singles(r, scene, prm, shape, first, first + 5)
            r.accum_begin(scene.camera, prm(3), first_sample=first)
            r.accum_track_filter(flt)
            r.accum_add(3)
            _plane_is(rt, r, flt, _reference(rt, flt, x[:3], first, shape), first, 3, (kind, first, shape, po, "after 3"))
            r.accum_add(2)
            want = _reference(rt, flt, x, first, shape)
            _plane_is(rt, r, flt, want, first, 5, (kind, first, shape, po, "after 3 + 2"))
            assert (want[..., 3] != 0).all() and (want[..., :3] != 0).any()
    r.accum_end()


# ---- 2. the box identity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("po", [1, 2])
def test_box_of_radius_half_is_the_accumulation_itself(rt, ctx, po):
    r = ctx
    scene, prm = _setup(rt, r, po=po)
    r.accum_begin(scene.camera, prm(3), first_sample=7)
    r.accum_track_filter(rt.make_pixel_filter("box"))
    r.accum_add(3), r.accum_add(2)
    st, snap = r.accum_export(), r.accum_export_filter()
    _same(snap.plane[..., :3], st.sum, "plane.rgb is the exported sum")
    _same(snap.plane[..., 3], np.full((NY, NX), 5, f32), "W is (float)n")
    img, rgb8, _, _ = r.accum_read(want_rgb8=True)
    fimg, frgb8, w = r.accum_filtered(want_rgb8=True, want_weight=True)
    _same(fimg, img, "filtered f32 is accum_read's"), _same(frgb8, rgb8, "filtered rgb8 is accum_read's"), _same(w, snap.plane[..., 3], "weight")
    assert rgb8.any()
    r.accum_end()


# ---- 3. the footprint of designed radiance ----------------------------------------------------------------------------------------------
IMPULSES = ((12, 6), (0, 0), (23, 5))  # (i, j): interior, a corner, an edge; further apart than any two footprints reach


@pytest.mark.parametrize("kind", ref.KINDS)
def test_footprint_of_an_impulse(rt, ctx, kind):
    """One pixel of radiance 1, all others 0: the plane holds exactly table[kx] * table[ky] at each neighbour whose support holds the sample,
    with the jitter of that (pixel, i0), and 0 elsewhere — written out here per neighbour, without filter_ref.add_samples.  An x / y swap, a
    sign error of the offset or a halo that wraps lands on other pixels or other table entries."""
    r = ctx
    scene, prm = _setup(rt, r, po=2)
    flt = rt.make_pixel_filter(kind)
    table, D = rt.pixel_filter_table(flt)
    i0 = 3
    r.accum_begin(scene.camera, prm(2), first_sample=0)
    r.accum_track_filter(flt)
    rad = np.zeros((1, NY, NX, 3), f32)
    for i, j in IMPULSES:
        rad[0, j, i] = 1.0
    r.debug_filter_add(i0, rad)
    jx, jy = ref.jitter(SEED, NX, NY, i0)
    want = np.zeros((NY, NX, 4), f32)
    hits = 0
    for i, j in IMPULSES:
        for dy in range(-D, D + 1):
            for dx in range(-D, D + 1):  # the target p = q - (dx, dy) sees q at (dx, dy)
                pi, pj = i - dx, j - dy
                if not (0 <= pi < NX and 0 <= pj < NY):
                    continue
                w, ok = ref.weights(jx[j, i], jy[j, i], dx, dy, table, flt.radius)
                if ok:
                    want[pj, pi] = w
                    hits += 1
    got = r.accum_export_filter()
    assert (got.first_sample, got.done) == (0, 0)  # the hook leaves `done`, and below the sums, alone
    # away from the impulses sum.w still collects the weights of the zero-radiance samples: rgb is the footprint, w is checked by the reference
    _same(got.plane[..., :3], want[..., :3], (kind, "rgb of the footprint"))
    full = _reference(rt, flt, list(rad), 0, i0=i0)
    _same(got.plane, full, (kind, "the whole plane against the reference"))
    assert hits >= len(IMPULSES) and (want[..., 0] != 0).sum() >= 3
    assert not r.accum_export().sum.any()
    r.accum_end()


@pytest.mark.parametrize("kind", ref.KINDS)
def test_a_nan_sample_poisons_its_neighbourhood_and_nothing_else(rt, ctx, kind):
    r = ctx
    scene, prm = _setup(rt, r, po=1)
    flt = rt.make_pixel_filter(kind)
    table, D = rt.pixel_filter_table(flt)
    i0, (qi, qj) = 2 ** 32 - 2, (12, 6)
    rad = np.full((2, NY, NX, 3), 0.5, f32)
    rad[1, qj, qi, 1] = np.nan
    rad[0, 2, 3] = 1e30
    r.accum_begin(scene.camera, prm(2), first_sample=0)
    r.accum_track_filter(flt)
    r.debug_filter_add(i0, rad)  # the samples 2^32 - 2 and 2^32 - 1
    got = r.accum_export_filter().plane
    want = _reference(rt, flt, list(rad), 0, i0=i0)
    _held(got, want, (kind, "plane"))
    jx, jy = ref.jitter(SEED, NX, NY, i0 + 1)
    poisoned = np.zeros((NY, NX), bool)
    for dy in range(-D, D + 1):
        for dx in range(-D, D + 1):
            if ref.weights(jx[qj, qi], jy[qj, qi], dx, dy, table, flt.radius)[1]:
                poisoned[qj - dy, qi - dx] = True
    assert poisoned[qj, qi] and np.array_equal(np.isnan(got[..., 1]), poisoned) and not np.isnan(got[..., (0, 2, 3)]).any()
    near = np.zeros((NY, NX), bool)
    near[qj - D:qj + D + 1, qi - D:qi + D + 1] = True
    assert not (poisoned & ~near).any()
    if float(flt.radius) == D + 0.5:  # the support reaches every sample of the (2D + 1)^2 neighbourhood: exactly that is poisoned
        assert np.array_equal(poisoned, near) and poisoned.sum() == (2 * D + 1) ** 2
    assert np.isfinite(got[2, 3, 0]) and got[2, 3, 0] > 1e29
    r.accum_end()


# ---- 4. slice and add invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mitchell", "gaussian"])
def test_plane_does_not_depend_on_slices_or_adds(rt, ctx, kind):
    r = ctx
    flt = rt.make_pixel_filter(kind)
    scene, prm = _setup(rt, r, po=2)
    x = _singles(r, scene, prm, "24x13", 7, 12)
    want = _reference(rt, flt, x, 7)
    for adds, spp_slice in (((5,), 1), ((5,), 2), ((5,), 5), ((2, 3), 2), ((1, 1, 1, 1, 1), 2), ((2, 3), 1)):
        r.accum_begin(scene.camera, prm(max(adds), spp_slice=spp_slice), first_sample=7)
        r.accum_track_filter(flt)
        for n in adds:
            r.accum_add(n)
        _same(r.accum_export_filter().plane, want, (kind, adds, spp_slice))
    r.accum_end()


# ---- 5. adaptive adds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("po", [1, 2])
def test_adaptive_adds_skip_converged_sources_and_keep_feeding_converged_targets(rt, ctx, ctx2, po):
    """A chosen set of pixels is made to converge by giving them moments without variance (S1 = S2 = 2 after two samples) under a tolerance of
    0, which stops a pixel only where V = 0.  They stop being sources; as targets they keep receiving from their active neighbours."""
    r = ctx
    first = 7
    flt = rt.make_pixel_filter("mitchell")
    scene, prm = _setup(rt, r, po=po)
    x = _singles(r, scene, prm, "24x13", first, first + 7)
    chosen = np.zeros((NY, NX), bool)
    chosen[3:9, 5:15] = True  # a block with an interior further than D from any active pixel
    chosen[0, 0] = chosen[12, 23] = chosen[10, 8] = chosen[11, 16] = True
    r.accum_begin(scene.camera, prm(3), first_sample=first)
    r.accum_track_filter(flt)
    r.accum_add(2)
    for p in np.flatnonzero(chosen):
        r.debug_accum_set_moments(int(p), 2.0, 2.0)
    before = r.accum_export_filter().plane
    r.accum_add_adaptive(3, 0.0, 0.01, 2)
    counts = r.accum_counts()[0]
    assert np.array_equal(counts == 2, chosen) and (counts[~chosen] == 5).all(), np.unique(counts, return_counts=True)
    want = _reference(rt, flt, x[:2], first)
    _same(before, want, "the plane before the adaptive add")
    want = _reference(rt, flt, x[2:5], first, plane=want, i0=first + 2, active=~chosen)
    st = r.accum_export()
    _plane_is(rt, r, flt, want, first, 5, (po, "after one adaptive add"), st.sum, counts)
    r.accum_add_adaptive(2, 0.0, 0.01, 2)
    counts = r.accum_counts()[0]
    assert np.array_equal(counts == 2, chosen) and (counts[~chosen] == 7).all()
    want = _reference(rt, flt, x[5:7], first, plane=want, i0=first + 5, active=~chosen)
    st = r.accum_export()
    snap = _plane_is(rt, r, flt, want, first, 7, (po, "after two adaptive adds"), st.sum, counts)
    changed = (_bits(snap.plane) != _bits(before)).any(-1)
    assert changed[3, 5] and changed[0, 0] and changed[8, 14]  # converged, with active neighbours
    assert not changed[5:7, 8:12].any()                        # converged, further than D = 2 from every active pixel
    assert changed[~chosen].all()
    # the fallback of the read-out takes the pixel's own count: a converged and an active pixel without a positive weight sum
    snap.plane[5, 9, 3], snap.plane[1, 20, 3] = 0.0, -1.0
    r2 = ctx2
    _setup(rt, r2, po=po)
    r2.accum_begin(scene.camera, prm(3), first_sample=first)
    r2.accum_import(st), r2.accum_import_filter(snap)
    c, W = ref.read_out(snap.plane, st.sum, counts)
    img, _, w = r2.accum_filtered(want_weight=True)
    _same(img, c, "read-out with counts"), _same(w, W, "weights with counts")
    box = r2.accum_read()[0]
    _same(img[5, 9], box[5, 9], "converged pixel falls back to its box mean of 2 samples")
    _same(img[1, 20], box[1, 20], "active pixel falls back to its box mean of 7 samples")
    r.accum_end(), r2.accum_end()


# ---- 6. the fallback ----------------------------------------------------------------------------------------------------------------------
def test_read_out_falls_back_to_the_box_mean_without_a_positive_weight(rt, ctx, ctx2):
    r, r2 = ctx, ctx2
    flt = rt.make_pixel_filter("tent")
    scene, prm = _setup(rt, r, po=2)
    r.accum_begin(scene.camera, prm(3), first_sample=0)
    r.accum_track_filter(flt)
    r.accum_add(3)
    st, snap = r.accum_export(), r.accum_export_filter()
    designed = {(2, 3): 0.0, (6, 12): -0.25, (11, 20): np.nan, (9, 9): -0.0}
    for (j, i), w in designed.items():
        snap.plane[j, i, 3] = w
    _setup(rt, r2, po=2)
    r2.accum_begin(scene.camera, prm(3), first_sample=0)
    r2.accum_import(st), r2.accum_import_filter(snap)
    img, rgb8, w = r2.accum_filtered(want_rgb8=True, want_weight=True)
    box, box8, _, _ = r2.accum_read(want_rgb8=True)
    c, W = ref.read_out(snap.plane, st.sum, 3)
    _same(img, c, "read-out"), _held(w, W, "weights")
    mask = np.zeros((NY, NX), bool)
    for j, i in designed:
        mask[j, i] = True
    _same(img[mask], box[mask], "the designed pixels read the box mean")
    with np.errstate(invalid="ignore", divide="ignore"):
        quotient = (snap.plane[..., :3] / snap.plane[..., 3:]).astype(f32)
    _same(img[~mask], quotient[~mask], "all others the quotient")
    assert (img[~mask] != box[~mask]).any()
    _same(rgb8[::-1][mask], box8[::-1][mask], "rgb8 of the designed pixels")
    # no sample yet: W = 0 everywhere, the sums are zeros
    r2.accum_begin(scene.camera, prm(3), first_sample=0)
    r2.accum_track_filter(flt)
    img, _, w = r2.accum_filtered(want_weight=True)
    assert not img.any() and not w.any() and not np.isnan(img).any()
    r.accum_end(), r2.accum_end()


# ---- 7. checkpoint and resume -----------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_for_bit(rt, ctx, ctx2, tmp_path):
    r, r2 = ctx, ctx2
    first = 7
    flt = rt.make_pixel_filter("mitchell")
    scene, prm = _setup(rt, r, po=2)
    x = _singles(r, scene, prm, "24x13", first, first + 5)
    r.accum_begin(scene.camera, prm(3), first_sample=first)
    r.accum_track_filter(flt)
    r.accum_add(3)
    st, snap = r.accum_export(), r.accum_export_filter()
    st.save(str(tmp_path / "state.npz")), snap.save(str(tmp_path / "filter.npz"))
    st2, snap2 = rt.AccumState.load(str(tmp_path / "state.npz")), rt.AccumFilter.load(str(tmp_path / "filter.npz"))
    _same(snap2.plane, snap.plane, "the file")
    assert bytes(snap2.filter) == bytes(flt)
    r.accum_add(2)
    whole = r.accum_export_filter()
    whole_read = r.accum_filtered(want_rgb8=True, want_weight=True)
    _setup(rt, r2, po=1)  # the other pixel order: the snapshot is in image order
    for track_first in (False, True):
        r2.accum_begin(scene.camera, prm(3), first_sample=first)
        if track_first:
            r2.accum_track_filter(flt)
            _raises(rt, rt._ffi.ERR_UNSUPPORTED, r2.accum_import, st2)  # the state comes first
            r2.accum_begin(scene.camera, prm(3), first_sample=first)
        r2.accum_import(st2)
        r2.accum_import_filter(snap2)
        _same(r2.accum_export_filter().plane, snap.plane, "right after the import")
        r2.accum_add(2)
        got = r2.accum_export_filter()
        _same(got.plane, whole.plane, "the resumed plane")
        _same(got.plane, _reference(rt, flt, x, first), "the resumed plane against the reference")
        for a, b, what in zip(r2.accum_filtered(want_rgb8=True, want_weight=True), whole_read, ("f32", "rgb8", "weight")):
            _same(a, b, ("the resumed read-out", what))
        assert (got.first_sample, got.done, got.frame_id) == (first, 5, whole.frame_id) and bytes(got.filter) == bytes(flt)
    # a fresh accumulation that tracks the same filter takes a snapshot of its own window; one that tracks another filter refuses it
    inv = rt._ffi.ERR_INVALID
    r2.accum_begin(scene.camera, prm(3), first_sample=first)
    r2.accum_track_filter(flt)
    empty = r2.accum_export_filter()
    assert empty.done == 0 and not empty.plane.any()
    r2.accum_import_filter(empty)
    r2.accum_begin(scene.camera, prm(3), first_sample=first)
    r2.accum_track_filter(rt.make_pixel_filter("gaussian"))
    _raises(rt, inv, r2.accum_import_filter, empty)
    other_radius = rt.AccumFilter(NX, NY, first, 0, empty.frame_id, filter=rt.make_pixel_filter("gaussian", 2.0))
    _raises(rt, inv, r2.accum_import_filter, other_radius)
    assert bytes(r2.accum_export_filter().filter) == bytes(rt.make_pixel_filter("gaussian"))
    # the header mismatches, each against an accumulation that holds the state
    def fresh():
        r2.accum_begin(scene.camera, prm(3), first_sample=first)
        r2.accum_import(st2)
    for field, value in (("done", 2), ("first_sample", first + 1), ("frame_id", snap2.frame_id ^ 1), ("nx", NX + 1), ("rows", NY - 1)):
        fresh()
        bad = rt.AccumFilter.load(str(tmp_path / "filter.npz"))
        if field in ("nx", "rows"):
            bad = rt.AccumFilter(NX + (field == "nx"), NY - (field == "rows"), first, 3, snap2.frame_id, filter=flt)
        else:
            setattr(bad, field, value)
        _raises(rt, inv, r2.accum_import_filter, bad)
        _raises(rt, rt._ffi.ERR_STATE, r2.accum_filtered)  # the refusal turned nothing on
    fresh()
    bad = rt.AccumFilter.load(str(tmp_path / "filter.npz"))
    bad.radius_bits = int(f32(0.25).view(np.uint32))
    _raises(rt, inv, r2.accum_import_filter, bad)
    fresh()
    r2.accum_add(1)
    _raises(rt, rt._ffi.ERR_STATE, r2.accum_import_filter, snap2)  # samples were added since
    r.accum_end(), r2.accum_end()


# ---- 8. nothing else moves --------------------------------------------------------------------------------------------------------------
def _everything(r):
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    counts, info = r.accum_counts()
    st, hs, bs = r.accum_export(), r.accum_export_halves(), r.accum_export_buckets()
    return [("f32", img), ("rgb8", rgb8), ("sem", sem), ("noise", bytes(noise)), ("counts", counts), ("info", bytes(info)),
            ("denoise", r.accum_denoise()[0]), ("denoise channels", r.accum_denoise_channels()[0]), ("denoise halves", r.accum_denoise_halves()[0]),
            ("state sum", st.sum), ("state moments", st.moments), ("state channel moments", st.channel_moments), ("state counts", st.counts),
            ("state converged", st.converged), ("state scalars", repr((st.first_sample, st.done, st.planes, st.frame_id)).encode()),
            ("halves sum", hs.sum), ("halves moments", hs.moments), ("buckets", bs.sum)]


@pytest.mark.parametrize("adaptive", [False, True])
def test_nothing_else_moves(rt, ctx, adaptive):
    r = ctx
    scene, prm = _setup(rt, r, po=2)
    runs = []
    for track in (False, True):
        r.accum_begin(scene.camera, prm(4), first_sample=7)
        r.accum_track_channels(), r.accum_track_halves(), r.accum_track_buckets(4)
        if track:
            r.accum_track_filter(rt.make_pixel_filter("mitchell", 3.0))
        stats = [r.accum_add(4), r.accum_add(3)]
        if adaptive:
            _, _, sem, noise = r.accum_read(want_sem=True)
            tol = float(np.median(sem[sem > 0])) / max(noise.mean_luminance, 1e-3)
            stats += [r.accum_add_adaptive(2, tol, 0.01, 4), r.accum_add_adaptive(3, tol, 0.01, 4)]
        got = _everything(r)
        got += [("stats %d %s" % (k, c), repr(getattr(s, c)).encode()) for k, s in enumerate(stats) for c in STATS_COUNTERS]
        got += [("rays per depth %d" % k, bytes(s.rays_per_depth)) for k, s in enumerate(stats)]
        runs.append(got)
    if adaptive:
        counts = dict(runs[0])["counts"]
        assert len(np.unique(counts)) > 1, "the adaptive adds stopped some pixels and not others"
    assert [k for k, _ in runs[0]] == [k for k, _ in runs[1]]
    for (what, a), (_, b) in zip(*runs):
        if isinstance(a, bytes):
            assert a == b, what
        else:
            _held(a, b, what)
    r.accum_end()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(rt, ctx):
    r = ctx
    f = rt._ffi
    flt = rt.make_pixel_filter("tent")
    scene, prm = _setup(rt, r)
    r.accum_end()
    _raises(rt, f.ERR_STATE, r.accum_track_filter, flt)  # no accumulation
    _raises(rt, f.ERR_STATE, r.accum_filtered)
    _raises(rt, f.ERR_STATE, r.accum_export_filter)
    # a sharded accumulation
    r.accum_begin(scene.camera, prm(2, shard_count=2, shard_band=4, shard_id=1))
    _raises(rt, f.ERR_STATE, r.accum_track_filter, flt)
    _raises(rt, f.ERR_STATE, r.accum_import_filter, rt.AccumFilter(NX, r.shard_rows(prm(2, shard_count=2, shard_band=4, shard_id=1)), filter=flt))
    r.accum_add(1)  # ... goes on untracked
    _raises(rt, f.ERR_STATE, r.accum_filtered)
    # a read, an export and the hook without tracking
    r.accum_begin(scene.camera, prm(2))
    _raises(rt, f.ERR_STATE, r.accum_filtered)
    _raises(rt, f.ERR_STATE, r.accum_export_filter)
    _raises(rt, f.ERR_STATE, r.debug_filter_add, 0, np.zeros((1, NY, NX, 3), f32))
    # a bad filter
    for bad in (rt.make_pixel_filter("tent", 0.25), rt.make_pixel_filter("tent", 3.5), rt.make_pixel_filter("gaussian", sigma=0.0),
                rt.make_pixel_filter(5), rt.make_pixel_filter("mitchell", B=float("nan")), rt.make_pixel_filter("box", float("inf")), None):
        _raises(rt, f.ERR_INVALID, r.accum_track_filter, bad)
    _raises(rt, f.ERR_STATE, r.accum_filtered)  # none of them turned tracking on
    # tracking after the first sample
    r.accum_add(1)
    _raises(rt, f.ERR_STATE, r.accum_track_filter, flt)
    r.accum_begin(scene.camera, prm(2))
    r.accum_add_adaptive(2, 0.1, 0.01, 2)
    _raises(rt, f.ERR_STATE, r.accum_track_filter, flt)
    # a second call: the same filter is fine, another one is not; a merge is not covered
    r.accum_begin(scene.camera, prm(2))
    r.accum_track_filter(flt), r.accum_track_filter(flt)
    _raises(rt, f.ERR_STATE, r.accum_track_filter, rt.make_pixel_filter("tent", 1.5))
    r.accum_add(2)
    st = r.accum_export()
    kept = r.accum_export_filter().plane
    r.accum_track_filter(flt)  # still the same filter: nothing changes, nothing is cleared
    st.first_sample = 2
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_merge, st)
    _raises(rt, f.ERR_INVALID, r.debug_filter_add, 0, np.zeros((0, NY, NX, 3), f32))
    _same(r.accum_export_filter().plane, kept, "the plane after the refusals")
    r.accum_end()
    _raises(rt, f.ERR_STATE, r.accum_filtered)  # tracking ended with the accumulation
    r.accum_begin(scene.camera, prm(2))
    _raises(rt, f.ERR_STATE, r.accum_filtered)
    r.accum_end()


# ---- 10. presentation -------------------------------------------------------------------------------------------------------------------
def test_rgb8_goes_through_the_glare_and_the_display(rt, ctx):
    r = ctx
    scene, prm = _setup(rt, r, po=2)
    r.accum_begin(scene.camera, prm(4), first_sample=0)
    r.accum_track_filter(rt.make_pixel_filter("gaussian"))
    r.accum_add(4)
    plain, plain8, _ = r.accum_filtered(want_rgb8=True)
    display = rt.make_display(exposure=0.18, auto="key", curve="aces", transfer="srgb", dither="bayer8")
    glare = rt.make_glare(amount=0.3, spread=0.8, levels=3)
    try:
        r.set_display(display)
        img, rgb8, _ = r.accum_filtered(want_rgb8=True)
        _same(img, plain, "f32 under a display")
        _same(rgb8, r.debug_display(img, display)[0], "rgb8 under a display")
        r.set_glare(glare)
        img, rgb8, _ = r.accum_filtered(want_rgb8=True)
        _same(img, plain, "f32 under a glare and a display")
        _same(rgb8, r.debug_glare(img, glare, display)[1], "rgb8 under a glare and a display")
        assert (rgb8 != plain8).any()
        r.set_display(None)
        _same(r.accum_filtered(want_rgb8=True)[1], r.debug_glare(img, glare, None)[1], "rgb8 under a glare")
    finally:
        r.set_display(None), r.set_glare(None)
    _same(r.accum_filtered(want_rgb8=True)[1], plain8, "rgb8 without either")
    r.accum_end()


# ---- 11. render.py ----------------------------------------------------------------------------------------------------------------------
def _render_py(*args):
    cmd = [sys.executable, "-m", "ray_tracing_in_one_weekend_amd.render", "--scene", "test_sphere", "--nx", "40", "--ny", "20", "--max-depth", "8",
           "--seed", "7", *[str(a) for a in args]]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_render_py_writes_the_filtered_image_and_resumes_it(rt, ctx, tmp_path):
    whole, part, resumed, box, ck = (tmp_path / n for n in ("whole.png", "part.png", "resumed.png", "box.png", "ck.npz"))
    flt = ("--pixel-filter", "mitchell", "--filter-radius", 1.5, "--filter-param", 0.25, 0.5)
    p = _render_py("--spp", 6, "--spp-step", 4, *flt, "--out", whole)
    assert p.returncode == 0, p.stderr[-2000:]
    p = _render_py("--spp", 4, "--spp-step", 4, *flt, "--checkpoint", ck, "--out", part)
    assert p.returncode == 0, p.stderr[-2000:]
    snap = rt.AccumFilter.load(str(ck) + ".filter.npz")
    assert (snap.first_sample, snap.done) == (0, 4) and snap.check() and bytes(snap.filter) == bytes(rt.make_pixel_filter("mitchell", 1.5, B=0.25, C=0.5))
    p = _render_py("--spp", 6, "--spp-step", 4, *flt, "--resume", ck, "--out", resumed)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(resumed, "rb").read() == open(whole, "rb").read() != open(part, "rb").read()
    # the image is accum_filtered's rgb8 of the same accumulation
    from PIL import Image
    scene = rt.Scene.build("test_sphere", 40 / 20)
    ctx.set_option("pixel_order", 0)
    ctx.upload(scene)
    ctx.accum_begin(scene.camera, rt.make_params(40, 20, 4, max_depth=8, seed=7))
    ctx.accum_track_filter(snap.filter)
    ctx.accum_add(4), ctx.accum_add(2)
    _same(np.asarray(Image.open(whole).convert("RGB")), ctx.accum_filtered(want_rgb8=True)[1], "the PNG")
    ctx.accum_end()
    p = _render_py("--spp", 6, "--spp-step", 4, "--pixel-filter", "tent", "--resume", ck, "--out", box)  # another filter than the checkpoint's
    assert p.returncode == 2 and "another filter" in p.stderr
    for more, word in ((("--denoise",), "--denoise"), (("--devices", "0,0", "--copy-gather"), "--devices"), (("--merge", ck), "--merge")):
        p = _render_py("--spp", 6, "--pixel-filter", "tent", *more, "--out", box)
        assert p.returncode == 2 and word in p.stderr and "--pixel-filter does not combine" in p.stderr, p.stderr[-2000:]
    p = _render_py("--spp", 6, "--pixel-filter", "gaussian", "--filter-radius", 3.5, "--out", box)
    assert p.returncode == 2 and "--filter-radius" in p.stderr
    assert not os.path.exists(box)
