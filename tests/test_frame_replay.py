"""Whole frames under rt_set_lens, rt_set_motion, rt_set_quads and rt_set_lights against tests/frame_replay.py — a frame as the in-order
sum of its paths, each path followed bounce by bounce through the single-kernel list walk — at the geometries of tests/frame_cases.py:
a single pixel, row-major frames under a chunk, tiles plus a tail, a chunk that straddles samples, shards with a tail, a partial band
and no row.  Every path through the renderer is walked against the replay, bit for bit, ray counts per depth included: slices, the debug
options, the list walk, shards, several contexts; and the accumulation entry points are fed by the replay's per-sample frames x[s],
never by frames the device delivered.  No comparison here has a tolerance.

The conditions that make a case worth its time are asserted on the replay alone: enough paths survive, they end in every way the scene
offers, and the set under test takes part in the bounces."""
import numpy as np
import pytest

import adaptive_ref
import denoise_channels_ref as ch_ref
import denoise_ref
import frame_cases as fc
import frame_replay
import noise_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
BRUTE = frame_replay.FLAG_BRUTE_FORCE
FLOOR, MIN, STEP = 0.01, 2, 2
OPTIONS = [("primary_lists", 1), ("grid", 1), ("pixel_order", 1), ("pixel_order", 2), ("materialise_primaries", 1), ("chains", 1),
           ("queue_shards", 1), ("queue_shards", 3), ("queue_shards", 64), ("isect_workgroups", 1)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = _bits(a) != _bits(b)
    assert not diff.any(), (what, "%d values differ, the first at %r" % (int(diff.sum()), tuple(int(v[0]) for v in np.nonzero(diff))))


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


_scenes, _frames = {}, {}


class Setup:
    def __init__(self, rt, case):
        self.rt, self.case = rt, case
        self.set, self.geom = fc.SETS[case[0]], fc.GEOMETRIES[case[1]]
        key = (self.set["scene"], self.geom["nx"], self.geom["ny"])
        if key not in _scenes:
            aspect = self.geom["nx"] / self.geom["ny"]
            _scenes[key] = fc.sphere_scene(rt, aspect) if self.set["scene"] == "spheres" else (fc.general_scene(rt, aspect),)
        self.scene = _scenes[key][0]
        self.lens = self.set.get("lens")
        self.shutter = fc.SHUTTER if self.set.get("motion") else None
        self.movers = _scenes[key][1] if self.set.get("motion") else np.zeros(0, np.uint32)

    def apply(self, r):
        """upload and sets, on a Renderer or a MultiRenderer"""
        r.upload(self.scene)
        r.set_lens(self.lens)
        if self.set.get("motion"):
            _, movers, c1, _ = _scenes[(self.set["scene"], self.geom["nx"], self.geom["ny"])]
            r.set_motion(self.rt.make_motion(movers, c1, fc.SHUTTER))
        if self.set.get("quads"):
            assert self.scene.quads.n
            r.set_quads(self.scene.quads)
        if self.set.get("lights"):
            if self.set["scene"] == "spheres":
                r.set_lights(self.rt.make_lights(*_scenes[(self.set["scene"], self.geom["nx"], self.geom["ny"])][3]))
            else:
                assert self.scene.lights.n == 2
                r.set_lights(self.scene.lights)

    def params(self, spp=fc.SPP, **kw):
        return fc.params(self.rt, self.case[1], spp, **kw)

    def shards(self):
        """[(shard id or None for an unsharded geometry, its image rows)]"""
        g = self.geom
        if "count" not in g:
            return [(None, np.arange(g["ny"]))]
        return [(k, frame_replay.shard_image_rows(g["ny"], g["band"], g["count"], k)) for k in range(g["count"])]

    def named(self):
        """the frame the geometry is named for: the whole one, or its named shard"""
        k = self.geom.get("shard")
        return (k, dict(self.shards())[k])


def _prepare(rt, r, case):
    """the context set up for the case, and the replay of its frame (made once, never changed)"""
    su = Setup(rt, case)
    su.apply(r)
    if case not in _frames:
        spp = fc.SPP_ADAPTIVE if case in fc.ADAPTIVE_CASES else fc.SPP
        _frames[case] = frame_replay.replay(r, su.scene, su.params(spp), su.lens, su.shutter)
    return su, _frames[case]


def _check_frame(got, fr, rows, what, spp=fc.SPP):
    img, _, st = got
    _same(img, fr.image(rows, spp), (what, "image"))
    want = fr.rays_per_depth(rows, slice(0, spp))
    have = list(st.rays_per_depth)
    assert have[:len(want)] == want and not any(have[len(want):]) and st.n_rays == sum(want), (what, "rays per depth", have[:len(want)], want)


def _conditions(su, fr):
    """on the replay alone; percentages only where the frame has the paths to carry them"""
    n = fr.last.size
    ends = fr.ends()
    alive2 = (fr.last >= 2).mean()
    rate = None
    if su.case[0] != "none":
        a = su.scene.arrays()
        n_static = len(a["sph_mat"]) + len(a["rect_mat"]) + len(a["med_mat"])
        mat_type = fc.material_type_of_hit(su.scene, bool(su.set.get("quads")))
        took = total = 0
        for depth, b in enumerate(fr.bounces):
            if depth == 0:
                continue
            hit = b["hit"]
            part = np.isin(hit, su.movers) | (bool(su.set.get("quads")) & (hit >= n_static))
            if su.set.get("lights"):
                part |= (hit >= 0) & fc.takes_light_branch(b["keys"], depth, mat_type[np.maximum(hit, 0)])
            took, total = took + int(part.sum()), total + len(hit)
        rate = took / max(total, 1)
    print("%s: %d paths, alive at depth 2 %.3f, ends %r, the set takes part in %r of the bounces past depth 0" % (fc.case_id(su.case), n, alive2, ends, rate))
    if n < 500:
        return
    assert alive2 >= 0.30, (su.case, alive2)
    assert ends["dropped"] == 0 and all(ends[k] > 0 for k in ("sky", "emitter", "absorbed", "depth limit")), (su.case, ends)
    if su.set.get("motion") or su.set.get("quads") or su.set.get("lights"):
        assert rate >= 0.05, (su.case, rate)


# ---- 1. every path through the renderer is the replay ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_every_path_through_the_renderer_is_the_replay(rt, ctx, case):
    r = ctx
    su, fr = _prepare(rt, r, case)
    _conditions(su, fr)
    cam = su.scene.camera
    info = r.scene_info()
    if su.set["scene"] == "spheres":
        assert info["grid"] == 1 and info["general_kernels"] == 0 and info["tree_in_lds"] == 1
    else:
        assert info["general_kernels"] == 1 and info["n_planar"] == (su.scene.quads.n if su.set.get("quads") else 0)
    # the whole frame, whatever shards the geometry names
    whole = rt.make_params(su.geom["nx"], su.geom["ny"], fc.SPP, max_depth=fc.MAX_DEPTH, seed=fc.SEED)
    _check_frame(r.render(cam, whole), fr, None, (case, "whole"))
    if su.set["scene"] == "spheres":
        assert r.render_parts()["primary_lists_overflow"] >= 0, (case, "the frame had no candidate lists")
    # the frame the geometry is named for, through every path
    sid, rows = su.named()
    kw = {} if sid is None else dict(shard_id=sid)
    for spp_slice in (2, 0):  # slices of 2, 2, 1; the library's own choice
        _check_frame(r.render(cam, su.params(spp_slice=spp_slice, **kw)), fr, rows, (case, "spp_slice", spp_slice))
    _check_frame(r.render(cam, su.params(flags=BRUTE, **kw)), fr, rows, (case, "list walk"))
    _check_frame(r.render(cam, su.params(flags=BRUTE, spp_slice=2, **kw)), fr, rows, (case, "list walk, sliced"))
    for opt, val in OPTIONS:
        r.set_option(opt, val)
        try:
            _check_frame(r.render(cam, su.params(spp_slice=2 if opt == "pixel_order" else 0, **kw)), fr, rows, (case, opt, val))
        finally:
            r.set_option(opt, 0)
    # shards, de-interleaved by the restated rows; ray counts summed
    if sid is not None:
        full = np.zeros((su.geom["ny"], su.geom["nx"], 3), F32)
        rays = np.zeros(64, np.uint64)
        for k, krows in su.shards():
            img, _, st = r.render(cam, su.params(shard_id=k, spp_slice=2))
            assert img.shape[0] == len(krows) == r.shard_rows(su.params(shard_id=k))
            _check_frame((img, None, st), fr, krows, (case, "shard", k))
            full[krows] = img
            rays += np.array(list(st.rays_per_depth), np.uint64)
        assert any(len(krows) == 0 for _, krows in su.shards()) == (case[1] == "16x11/4x4")
        _same(full, fr.image(None, fc.SPP), (case, "shards de-interleaved"))
        want = fr.rays_per_depth(None, slice(0, fc.SPP))
        assert [int(x) for x in rays[:len(want)]] == want, (case, "ray counts summed over the shards")


@pytest.mark.parametrize("case", fc.MULTI_CASES, ids=fc.case_id)
def test_three_contexts_gather_the_replay(rt, ctx, case):
    su, fr = _prepare(rt, ctx, case)
    m = rt.MultiRenderer([0, 0, 0], copy_gather=True)
    try:
        su.apply(m)
        _check_frame(m.render(su.scene.camera, su.params()), fr, None, (case, "three contexts"))
    finally:
        m.close()


def test_the_fused_depth_0_ran_without_overflow_for_every_sphere_set(rt, ctx):
    """primary_lists_overflow == 0: every pixel had a candidate list, so k_shade<GEN> found every depth-0 hit from the lists."""
    for name, st in fc.SETS.items():
        if st["scene"] != "spheres":
            continue
        seen = {}
        for case in fc.CASES:
            if case[0] == name:
                su = Setup(rt, case)
                su.apply(ctx)
                ctx.render(su.scene.camera, su.params())
                seen[case[1]] = ctx.render_parts()["primary_lists_overflow"]
        print(name, seen)
        assert all(v >= 0 for v in seen.values()) and 0 in seen.values(), (name, seen)


# ---- 2. accumulations, fed by the replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", [False, True], ids=["plain", "channels"])
@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_accumulation_in_steps_is_the_replay(rt, ctx, case, track):
    r = ctx
    su, fr = _prepare(rt, r, case)
    sid, rows = su.named()
    x = fr.frames(rows, fc.SPP)
    r.accum_begin(su.scene.camera, su.params(2, **({} if sid is None else dict(shard_id=sid))))
    if track:
        r.accum_track_channels()
    done = 0
    for n in (2, 1, 2):
        st = r.accum_add(n)
        done += n
        total, s1, s2, _ = noise_ref.accumulate(x[:done])
        img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
        _same(img, fr.image(rows, done), (case, done, "image"))
        _same(img, (total / F32(done)).astype(F32), (case, done, "noise_ref's sum"))
        _same(rgb8, denoise_ref.finalize_rgb8(fr.image(rows, done)), (case, done, "rgb8"))
        _same(sem, noise_ref.sem(s1, s2, done), (case, done, "sem"))
        want = fr.rays_per_depth(rows, slice(done - n, done))
        assert list(st.rays_per_depth)[:len(want)] == want and noise.spp_done == done, (case, done, "rays of the add")
        if track:
            c1, c2 = ch_ref.accumulate_channels(x[:done])
            _same(r.accum_channel_sem(), ch_ref.channel_sem(c1, c2, done), (case, done, "channel sem"))
    r.accum_end()


def _tolerance(x):
    """test_adaptive._tolerance for decisions at 2 and 4 of 6 samples: the median, over the pixels with any variance, of the relative
    standard error after 4 samples — the last decision — from the reference alone"""
    rel = adaptive_ref.relative_error(x, 4, FLOOR)
    rel = rel[np.isfinite(rel) & (rel > 0)]
    return float(np.quantile(rel, 0.5)) if rel.size else 0.05


@pytest.mark.parametrize("case", fc.ADAPTIVE_CASES, ids=fc.case_id)
def test_render_adaptive_is_the_replay(rt, ctx, case):
    r = ctx
    su, fr = _prepare(rt, r, case)
    sid, rows = su.named()
    x = fr.frames(rows, fc.SPP_ADAPTIVE)
    tol = _tolerance(x)
    rp = adaptive_ref.Replay(x)
    while rp.issued < fc.SPP_ADAPTIVE:
        if rp.adaptive(min(STEP, fc.SPP_ADAPTIVE - rp.issued), tol, FLOOR, MIN) == 0:
            break
    early, full = (rp.cnt < fc.SPP_ADAPTIVE).mean(), (rp.cnt == fc.SPP_ADAPTIVE).mean()
    print(fc.case_id(case), "tolerance", tol, "counts", np.unique(rp.cnt, return_counts=True))
    assert early >= 0.10 and full >= 0.10, (case, tol, early, full)  # coverage, from the reference alone
    p = su.params(fc.SPP_ADAPTIVE, **({} if sid is None else dict(shard_id=sid)))
    for opts in ({}, {"pixel_order": 1}, {"pixel_order": 2}, {"queue_shards": 3}):
        for o, v in opts.items():
            r.set_option(o, v)
        try:
            img, rgb8, sem, counts, noise, info, st = r.render_adaptive(su.scene.camera, p, tol, STEP, FLOOR, MIN, want_rgb8=True, want_sem=True)
        finally:
            for o in opts:
                r.set_option(o, 0)
        assert np.array_equal(counts, rp.cnt), (case, opts, "counts", int((counts != rp.cnt).sum()))
        _same(img, rp.image(), (case, opts, "image"))
        _same(sem, rp.sem(), (case, opts, "sem"))
        _same(rgb8, denoise_ref.finalize_rgb8(rp.image()), (case, opts, "rgb8"))
        assert (info.n_active, info.n_samples, info.spp_min, info.spp_max) == rp.info(), (case, opts, "info")
        assert st.n_paths == sum(rp.traced) == st.rays_per_depth[0], (case, opts, st.n_paths, rp.traced)
        # the rays of the samples every pixel took: per depth, from the replay's paths
        took = np.arange(fc.SPP_ADAPTIVE)[:, None, None] < rp.cnt[None]
        last = fr.last[:, rows][took]
        want = [int((last >= k).sum()) for k in range(fc.MAX_DEPTH + 1)]
        assert list(st.rays_per_depth)[:len(want)] == want, (case, opts, "rays per depth")


def test_the_filters_on_a_frame_from_the_replay(rt, ctx):
    r = ctx
    case = fc.DENOISE_CASE
    su, fr = _prepare(rt, r, case)
    x = fr.frames(None, fc.SPP)
    total, s1, s2, n = noise_ref.accumulate(x)
    ybar, var = noise_ref.pixel_figures(s1, s2, n)
    c = (total / F32(n)).astype(F32)
    var_rgb = ch_ref.channel_variance(*ch_ref.accumulate_channels(x), n).astype(F32)
    k = rt._ffi.DENOISE_DEFAULT_STRENGTH
    by_luminance, _ = denoise_ref.denoise(c, ybar.astype(F32), var.astype(F32), 5, 1, k)
    by_channels, _ = ch_ref.denoise(c, var_rgb, 5, 1, k)
    assert (by_luminance != c).any(axis=-1).mean() >= 0.10 and (by_channels != c).any(axis=-1).mean() >= 0.10  # coverage
    r.accum_begin(su.scene.camera, su.params(fc.SPP, spp_slice=2))
    r.accum_track_channels()
    r.accum_add(fc.SPP)
    img, rgb8 = r.accum_denoise(want_rgb8=True)
    _same(img, by_luminance, "rt_accum_denoise"), _same(rgb8, denoise_ref.finalize_rgb8(by_luminance), "rt_accum_denoise, rgb8")
    img, rgb8 = r.accum_denoise_channels(want_rgb8=True)
    _same(img, by_channels, "rt_accum_denoise_channels"), _same(rgb8, denoise_ref.finalize_rgb8(by_channels), "rt_accum_denoise_channels, rgb8")
    r.accum_end()
