"""Motion blur on the host side (no GPU): MovingSphere flattens to its centre of time 0 plus a motion-table entry, moving_sphere_scene
is sphere_scene with its small diffuse spheres moving upwards, the shutter is validated, and the documented f32 semantics of c(tm)
stay within the 2 ulp of the coordinate magnitude that the GPU's bounds rely on."""
import numpy as np
import pytest

import motion_ref


def _motion_arrays(m):
    n = m.n_moving
    idx = np.array([m.sphere[k] for k in range(n)], dtype=np.uint32)
    c1 = np.array([m.center1[k] for k in range(3 * n)], dtype=np.float32).reshape(n, 3)
    return idx, c1


def _centres(scene):
    a = scene.arrays()
    return np.stack([a["sph_cx"], a["sph_cy"], a["sph_cz"]], axis=1).astype(np.float32)


def test_moving_sphere_flattens_to_c0_and_a_motion_entry(rt):
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    m = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.5, 0.5, 0.5)))
    s.sphere((0, -100.5, -1), 100.0, m, "ground")
    s.moving_sphere((0.25, 0.5, -1), (0.75, 1.5, -2), 0.5, m, "mover")
    s.sphere((2, 0, -1), 0.5, m, "still")
    s.set_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, 2.0, shutter=(0.25, 0.5))
    s.finish(use_bvh=False)
    mo = s.motion
    idx, c1 = _motion_arrays(mo)
    assert mo.n_moving == 1 and (mo.shutter_open, mo.shutter_close) == (0.25, 0.5)
    assert s.sphere_name(int(idx[0])) == "mover"
    assert np.array_equal(_centres(s)[idx[0]], np.array([0.25, 0.5, -1], np.float32))
    assert np.array_equal(c1[0], np.array([0.75, 1.5, -2], np.float32))
    assert s.flat.n_spheres == 3


def test_static_scene_has_no_motion_and_default_shutter(rt):
    s = rt.Scene.build("sphere_scene", 16 / 9)
    mo = s.motion
    assert mo.n_moving == 0 and (mo.shutter_open, mo.shutter_close) == (0.0, 1.0)


def test_moving_sphere_below_a_wrapper_is_refused(rt):
    f = rt._ffi
    s = rt.Scene.new()
    m = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.5, 0.5, 0.5)))
    h = s.moving_sphere((0, 0, 0), (0, 1, 0), 0.5, m, "mover")
    s.translate(h, (1, 0, 0))
    s.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0)
    with pytest.raises(rt.RtError, match="only bare spheres move"):
        s.finish(use_bvh=False)


@pytest.mark.parametrize("shutter", [(-0.1, 0.5), (0.6, 0.5), (0.0, 1.5), (float("nan"), 1.0)])
def test_shutter_validation(rt, shutter):
    s = rt.Scene.new()
    with pytest.raises(rt.RtError, match="shutter"):
        s.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, shutter=shutter)


def test_moving_sphere_scene_is_sphere_scene_with_bouncing_diffuse_spheres(rt):
    f = rt._ffi
    a, b = rt.Scene.build("sphere_scene", 16 / 9), rt.Scene.build("moving_sphere_scene", 16 / 9)
    assert a.flat.n_spheres == b.flat.n_spheres == 533
    ca, cb = _centres(a), _centres(b)
    ra, rb = a.arrays()["sph_r"], b.arrays()["sph_r"]
    by_name = {a.sphere_name(i): i for i in range(533)}
    idx, c1 = _motion_arrays(b.motion)
    assert len(idx) > 300 and np.all(np.diff(idx.astype(np.int64)) > 0)
    mat_type = b.arrays()["mat_type"]
    sph_mat = b.arrays()["sph_mat"]
    for i in range(533):  # every sphere stands where sphere_scene puts it, bit for bit
        j = by_name[b.sphere_name(i)]
        assert np.array_equal(ca[j].view(np.uint32), cb[i].view(np.uint32)) and ra[j] == rb[i]
    moving = set(int(i) for i in idx)
    for i in range(533):
        small_diffuse = rb[i] == np.float32(0.2) and mat_type[sph_mat[i]] == f.MAT_DIFFUSE
        assert (i in moving) == bool(small_diffuse), (i, b.sphere_name(i))
    d = c1 - cb[idx]
    assert np.all(d[:, 0] == 0) and np.all(d[:, 2] == 0) and np.all(d[:, 1] >= 0) and np.all(d[:, 1] < 0.5) and d[:, 1].max() > 0.4
    assert np.array_equal(np.array(list(a.camera.origin)), np.array(list(b.camera.origin)))


def test_f32_centre_is_within_2_ulp_of_the_exact_one():
    """The figure every bound of rt_set_motion relies on: |c(tm) - (c0 + tm (c1 - c0))| <= 2 ulp of the larger coordinate magnitude,
    where c1 - c0 is the f32 difference the library forms once (its bounds run from c0 to c0 + dc)."""
    rng = np.random.default_rng(5)
    n = 200000
    scale = 10.0 ** rng.uniform(-3, 6, size=(n, 1))
    c0 = (rng.uniform(-1, 1, size=(n, 3)) * scale).astype(np.float32)
    c1 = (c0 + rng.uniform(-1, 1, size=(n, 3)) * scale * 10.0 ** rng.uniform(-4, 0, size=(n, 1))).astype(np.float32)
    tm = rng.uniform(0, 1, size=n).astype(np.float32)
    tm[:1000] = 0.0
    tm[1000:2000] = 1.0
    got = motion_ref.center_at(c0, c1, tm).astype(np.float64)
    dc = (c1 - c0).astype(np.float32).astype(np.float64)
    exact = c0.astype(np.float64) + tm.astype(np.float64)[:, None] * dc
    mag = np.maximum(np.abs(c0.astype(np.float64)), np.abs(c0.astype(np.float64) + dc))
    ulp = np.spacing(mag.astype(np.float32)).astype(np.float64)
    worst = (np.abs(got - exact) / ulp).max()
    print("worst error of c(tm): %.3f ulp of the coordinate magnitude" % worst)
    assert worst <= 2.0
    # and the point stays inside the segment's box widened by 2^-22 of the magnitude (the slack rt_set_motion adds)
    lo = np.minimum(c0.astype(np.float64), c0.astype(np.float64) + dc) - mag * 2.0 ** -22
    hi = np.maximum(c0.astype(np.float64), c0.astype(np.float64) + dc) + mag * 2.0 ** -22
    assert np.all(got >= lo) and np.all(got <= hi)
