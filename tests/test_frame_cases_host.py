"""The geometries of tests/frame_cases.py and the GPU-free pieces of tests/frame_replay.py, without a GPU: the numpy restatement of the rows
of a shard against rt_shard_rows / rt_shard_row_to_image_row (host functions of the GPU library), the pixel order and the dealing of chunks
against their defining properties, every named geometry against the property it is named for, and the replay's row selection, sample order
and division on synthetic per-sample frames."""
import numpy as np
import pytest

import adaptive_ref
import frame_cases as fc
import frame_replay

F32 = np.float32


@pytest.fixture(scope="module")
def lib(rt):
    return rt._ffi.load_gpu_library()  # dlopen and symbol binding only


def test_restated_shard_rows_are_the_librarys(lib):
    n = 0
    for ny in (1, 2, 7, 8, 11, 27, 64, 135):
        for band in (0, 1, 3, 4, 8, 16):
            for count in (0, 1, 2, 3, 4, 8, 11):
                for sid in range(max(count, 1) + 1):
                    want = lib.rt_shard_rows(ny, band, count, sid)
                    assert fc.shard_rows(ny, band, count, sid) == want, (ny, band, count, sid)
                    if sid >= max(count, 1):  # no such shard: no rows when the frame is sharded (an unsharded frame has one shard, 0)
                        assert want == (0 if count > 1 else ny)
                        continue
                    rows = frame_replay.shard_image_rows(ny, band, count, sid)
                    assert len(rows) == want, (ny, band, count, sid)
                    got = [lib.rt_shard_row_to_image_row(lj, band, count, sid) for lj in range(want)]
                    assert got == list(rows) == [frame_replay.local_row_to_image_row(lj, band, count, sid) for lj in range(want)], (ny, band, count, sid)
                    n += 1
    assert n > 1000
    # the shards of a frame partition its rows
    for ny, band, count in ((27, 8, 2), (11, 4, 4), (13, 8, 3)):
        rows = np.concatenate([frame_replay.shard_image_rows(ny, band, count, k) for k in range(count)])
        assert sorted(rows.tolist()) == list(range(ny))


def test_restated_pixel_order_is_a_bijection_with_a_row_major_tail():
    for nx, rows in ((8, 8), (16, 11), (24, 13), (24, 11), (32, 5), (7, 3), (16, 3), (1, 1), (40, 17)):
        for general, po in ((False, 0), (True, 0), (True, 2), (False, 1)):
            tpr, tp = fc.pixel_order(po, general, nx, rows)
            tiles = nx % 8 == 0 and rows >= 8 and (po == 2 or (po == 0 and not general))
            assert (tpr > 0) == tiles and tp == (nx * (rows // 8) * 8 if tiles else 0), (nx, rows, general, po)
            where = np.array([[fc.local_of_pixel(nx, tpr, tp, i, lj) for i in range(nx)] for lj in range(rows)])
            assert sorted(where.ravel().tolist()) == list(range(nx * rows))
            tail = where[(rows // 8) * 8 if tiles else 0:]
            assert np.array_equal(tail.ravel(), np.arange(tail.size) + (tp if tiles else 0))  # row-major behind the tiles
            if tiles:  # 64 consecutive slots are one 8 x 8 block
                for t in range(tp // 64):
                    lj, i = np.nonzero((where >= 64 * t) & (where < 64 * t + 64))
                    assert lj.max() - lj.min() == 7 and i.max() - i.min() == 7 and lj.min() % 8 == 0 and i.min() % 8 == 0


def test_restated_dealing_fills_every_shard_within_its_capacity():
    for nq in (1, 3, 8, 64, 2048):
        for n in (5, 105, 256, 257, 880, 1560, 3240):
            cap = fc.shard_cap(nq, n)
            q, pos = fc.deal(nq, np.arange(n))
            assert pos.max() < cap and cap % 256 == 0 and cap >= 256
            assert len(set(zip(q.tolist(), pos.tolist()))) == n  # no two paths share a place
            assert cap * nq >= n and (cap - 256) * nq < -(-n // 256) * 256  # no smaller multiple of 256 holds the chunks
            for s in range(min(nq, 4)):  # a shard's places are filled from the front, but for its last chunk
                mine = np.sort(pos[q == s])
                full = mine[:len(mine) // 256 * 256] if len(mine) % 256 else mine
                assert np.array_equal(full, np.arange(len(full)))


def test_every_geometry_has_the_property_it_is_named_for():
    P = {g: fc.properties(g) for g in fc.GEOMETRIES}
    one = lambda g, k=0: P[g]["shards"][k]
    assert one("1x1")["npix"] == 1
    s = one("7x3")
    assert s["tiles_per_row"] == 0 and s["npix"] < 256 and fc.GEOMETRIES["7x3"]["nx"] % 8 != 0
    s = one("32x5")
    assert fc.GEOMETRIES["32x5"]["nx"] % 8 == 0 and s["rows"] < 8 and s["tiles_per_row"] == 0
    s = one("16x11")
    assert s["tiles_per_row"] > 0 and s["rows"] % 8 == 3 == s["tail_rows"] and s["npix"] < 256
    s = one("24x13")
    assert s["tiles_per_row"] > 0 and s["rows"] % 8 != 0 and s["npix"] == 312 and s["npix"] > 256 and s["npix"] % 256 != 0 and s["chunk_straddles_samples"]
    s = one("24x27/8x2", 1)
    assert fc.GEOMETRIES["24x27/8x2"]["shard"] == 1 and s["rows"] == 11 and s["tiles_per_row"] > 0 and s["tail_rows"] == 3 and not P["24x27/8x2"]["empty"]
    assert one("24x27/8x2", 0)["rows"] == 16 and one("24x27/8x2", 0)["tail_rows"] == 0
    s = one("16x11/4x4", 2)
    assert fc.GEOMETRIES["16x11/4x4"]["shard"] == 2 and s["rows"] == 3 and s["partial_band"] == 3 and P["16x11/4x4"]["empty"] == [3]
    assert [P["16x11/4x4"]["shards"][k]["rows"] for k in range(3)] == [4, 4, 3]
    # general scenes keep the rows unless RT_OPT_PIXEL_ORDER 2 asks for tiles: both orders are rendered for every case
    assert fc.properties("24x13", general=True)["shards"][0]["tiles_per_row"] == 0
    assert fc.properties("24x13", general=True, po=2)["shards"][0]["tiles_per_row"] == 3
    # no case is larger than about 3 300 paths
    for _, g in fc.CASES:
        assert fc.GEOMETRIES[g]["nx"] * fc.GEOMETRIES[g]["ny"] * fc.SPP <= 3300
    for s_, g in fc.ADAPTIVE_CASES:
        rows = max(v["rows"] for v in P[g]["shards"].values()) if "shard" not in fc.GEOMETRIES[g] else one(g, fc.GEOMETRIES[g]["shard"])["rows"]
        assert rows * fc.GEOMETRIES[g]["nx"] * fc.SPP_ADAPTIVE <= 3300


def test_the_case_lists_cover_what_they_promise():
    for s in fc.SETS:
        have = {g for s_, g in fc.CASES if s_ == s}
        assert set(fc.EVERY_SET_GETS) <= have, s
    for g in fc.GEOMETRIES:
        have = {s for s, g_ in fc.CASES if g_ == g}
        assert {"none", "lens"} <= have and any(fc.SETS[s]["scene"] == "general" for s in have), g
    assert {s for s, _ in fc.MULTI_CASES} == set(fc.SETS) and set(fc.MULTI_CASES) <= set(fc.CASES)
    assert set(fc.ADAPTIVE_CASES) <= set(fc.CASES) and {g for _, g in fc.ADAPTIVE_CASES} == set(fc.TAILED)
    assert {s for s, _ in fc.ADAPTIVE_CASES} >= {"lens", "motion"} and fc.DENOISE_CASE in fc.CASES
    assert not any(fc.SETS[s].get("motion") and (fc.SETS[s].get("quads") or fc.SETS[s].get("lights")) for s in fc.SETS)


def test_the_scenes_are_what_the_cases_say(rt):
    """host code only: the sphere scene gets a grid with two large spheres, the general scene has wrappers, a medium, rectangles, planar
    primitives of both kinds and two emitters for Scene.lights; no mover is an emitter or leaves the layer"""
    for geom in ("1x1", "32x5", "24x27/8x2"):
        g = fc.GEOMETRIES[geom]
        scene, movers, c1, lights = fc.sphere_scene(rt, g["nx"] / g["ny"])
        grid = rt.grid_build(scene)
        assert grid is not None and grid["large"] == [0, 1] and np.prod(grid["dims"]) >= 64
        assert scene.flat.n_spheres == 2 + fc.N_SMALL and scene.flat.n_rects == 0 and 16 <= len(movers) < fc.N_SMALL
        a = scene.arrays()
        assert (a["mat_type"][a["sph_mat"][movers]] != rt._ffi.MAT_EMISSION).all() and (c1[:, 1] - 0.3 > 0.1).all()
        assert len(lights[0]) == 2
        general = fc.general_scene(rt, g["nx"] / g["ny"])
        fs = general.flat
        assert fs.n_rects >= 14 and fs.n_xforms >= 2 and fs.n_media == 1 and general.lights.n == 2 == general.lights.n_found
        kinds = np.ctypeslib.as_array(general.quads.kind, shape=(general.quads.n,))
        assert (kinds == rt._ffi.PLANAR_TRIANGLE).sum() == 60 and (kinds == rt._ffi.PLANAR_QUAD).sum() == 3
        assert len(fc.material_type_of_hit(general, True)) == fs.n_spheres + fs.n_rects + fs.n_media + general.quads.n


def _synthetic(spp, ny, nx, seed=3):
    """per-sample values that make every order of summation and every misplaced row or sample visible: magnitudes over 2^-20 .. 2^20"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.5, 1.0, (spp, ny, nx, 3)) * 2.0 ** rng.integers(-20, 21, (spp, ny, nx, 1))).astype(F32)
    last = rng.integers(0, 5, (spp, ny, nx))
    return frame_replay.Frame(x, last, np.zeros((spp, ny, nx), np.int64), [], 4)


def test_the_replays_sums_rows_and_counts_on_synthetic_frames():
    fr = _synthetic(5, 11, 6)
    # sample order: ((((0 + x0) + x1) + x2) + x3) + x4, then one division — per element, against a scalar loop
    img = fr.image()
    for j, i, c in ((0, 0, 0), (10, 5, 2), (4, 3, 1)):
        t = F32(0)
        for s in range(5):
            t = F32(t + fr.x[s, j, i, c])
        assert img[j, i, c] == F32(t / F32(5))
    back = frame_replay.mean_in_order(fr.x[::-1])
    assert (back != img).any()  # (the values are such that the order shows)
    assert np.array_equal(fr.image(spp=3), frame_replay.mean_in_order(fr.x[:3])) and (fr.image(spp=3) != img).any()
    # rows of a shard, in its local order; a shard without rows
    rows = frame_replay.shard_image_rows(11, 4, 4, 2)
    assert rows.tolist() == [8, 9, 10] and np.array_equal(fr.image(rows), img[8:11])
    rows = frame_replay.shard_image_rows(11, 2, 2, 1)
    assert rows.tolist() == [2, 3, 6, 7, 10] and np.array_equal(fr.image(rows), img[rows])
    empty = frame_replay.shard_image_rows(11, 4, 4, 3)
    assert fr.image(empty).shape == (0, 6, 3) and fr.rays_per_depth(empty) == [0] * 5
    # ray counts: a path whose last ray is at depth k was traced at depths 0 .. k
    want = [int((fr.last >= k).sum()) for k in range(5)]
    assert fr.rays_per_depth() == want and want[0] == fr.last.size
    parts = [fr.rays_per_depth(frame_replay.shard_image_rows(11, 4, 4, k)) for k in range(4)]
    assert [sum(p[k] for p in parts) for k in range(5)] == want
    assert [a + b for a, b in zip(fr.rays_per_depth(samples=slice(0, 2)), fr.rays_per_depth(samples=slice(2, 5)))] == want
    # the per-sample frames are what adaptive_ref.Replay takes
    rp = adaptive_ref.Replay(fr.frames(rows))
    rp.uniform(5)
    assert np.array_equal(rp.image(), fr.image(rows)) and rp.cnt.shape == (5, 6)
    with pytest.raises(ValueError):
        fr.x[0, 0, 0, 0] = 1.0  # a replay is never changed


def test_near_one_is_the_interval_of_the_kernels():
    d = np.zeros((6, 3), F32)
    d[:, 0] = np.sqrt(np.array([0x3f7fffe0, 0x3f7fffdf, 0x3f800011, 0x3f800012, 0x3f800000, 0x7fc00000], np.uint32).view(F32).astype(np.float64)).astype(F32)
    l2 = (d[:, 0] * d[:, 0]).astype(F32).view(np.uint32)
    want = (l2 >= 0x3f7fffe0) & (l2 <= 0x3f800011)
    want[5] = False
    assert np.array_equal(frame_replay.near_one(d), want) and want[4] and not want[5]
