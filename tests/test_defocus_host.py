"""Thin-lens camera without a GPU: the new C-ABI symbols, RtLens as gcc and ctypes lay it out, the host mirror's thin-lens camera
against the pinhole one, and the numpy restatement of the lens rays (tests/lens_ref.py) that tests/test_defocus.py holds the kernels to."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lens_ref
from helpers import ctr_draw, path_keys, primary_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lens_symbols_are_exported_by_both_libraries(rt):
    f = rt._ffi
    gpu, host = f.load_gpu_library(), f.load_host_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", f.GPU_LIB_PATH], check=True, capture_output=True, text=True).stdout
    for n in ("rt_set_lens", "rt_multi_set_lens"):
        assert n in f.GPU_SYMBOLS and hasattr(gpu, n) and re.search(rf" T {n}$", nm, flags=re.M), n
    for n in ("rth_set_camera_lens", "rth_scene_lens"):
        assert n in f.HOST_SYMBOLS and hasattr(host, n), n
    assert gpu.rt_abi_version() == 11  # the lens only adds symbols
    assert gpu.rt_set_lens(None, None) == -1 and gpu.rt_multi_set_lens(None, None) == -1  # RT_ERR_INVALID, no context needed


def test_rtlens_layout_matches_the_c_compiler(rt, tmp_path):
    src = tmp_path / "lens.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   'sizeof(RtLens),offsetof(RtLens,lens_radius),offsetof(RtLens,focus_dist));return 0;}\n')
    exe = tmp_path / "lens"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    L = rt.RtLens
    assert got == [C.sizeof(L), L.lens_radius.offset, L.focus_dist.offset] == [8, 0, 4]


CAMERAS = [((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 16 / 9, 0.1, 10.0),  # the book's cover
           ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 20.0, 800.0),
           ((-2.5, 7.25, 1e4), (0.3, -1.0, 2.0), (0.2, 1.0, -0.1), 63.0, 0.75, 3.0e-3, 0.37)]


def _scene(rt, *cam, **lens):
    s = rt.Scene.new()
    s.sphere((0.0, 0.0, 0.0), 1.0, s.material(rt._ffi.MAT_DIFFUSE, tex0=s.constant_tex((0.5, 0.5, 0.5))))
    s.set_camera(*cam, **lens)
    return s.finish()


@pytest.mark.parametrize("cam", CAMERAS)
def test_thin_lens_camera_flattens_like_the_pinhole_one(rt, cam):
    """Camera::new_lens gives new_'s RtCamera bit for bit (rth_set_camera_lens against rth_set_camera), and the lens
    {aperture / 2, focus_dist}; a pinhole scene's lens is {0, 1}."""
    *pin, aperture, focus = cam
    a, b = _scene(rt, *pin), _scene(rt, *pin, aperture=aperture, focus_dist=focus)
    assert bytes(a.camera) == bytes(b.camera)
    assert (a.lens.lens_radius, a.lens.focus_dist) == (0.0, 1.0)
    assert b.lens.lens_radius == np.float32(aperture) / np.float32(2.0) and b.lens.focus_dist == np.float32(focus)
    c = _scene(rt, *pin, aperture=0.0, focus_dist=focus)  # a zero aperture through the lens entry point: still the pinhole camera
    assert bytes(c.camera) == bytes(a.camera) and c.lens.lens_radius == 0.0
    for bad in ({"aperture": -0.1, "focus_dist": 1.0}, {"aperture": 0.1, "focus_dist": 0.0}, {"aperture": float("nan"), "focus_dist": 1.0},
                {"aperture": 0.1, "focus_dist": float("inf")}):
        with pytest.raises(rt.RtError, match="rth_set_camera_lens"):
            rt.Scene.new().set_camera(*pin, **bad)


def test_named_scenes_have_a_pinhole_lens(rt):
    s = rt.Scene.build("sphere_scene", 16 / 9)
    assert (s.lens.lens_radius, s.lens.focus_dist) == (0.0, 1.0)


def test_disc_draws_follow_the_rejection_rule():
    """random_in_unit_disk as restated: every point lies inside the unit disc, trip t reads counters 2 + 2t and 3 + 2t (2..253 in all),
    the first accepted pair is taken, and about pi/4 of the trips accept."""
    n = 20000
    keys = path_keys(95, np.arange(n, dtype=np.uint64) * 7919, np.arange(n, dtype=np.uint64) % 256)
    k0, k1 = keys[:, 0], keys[:, 1]
    rx, ry, trips = lens_ref.disc_draws(k0, k1)
    r2 = (rx * rx).astype(np.float32) + (ry * ry).astype(np.float32)
    assert (r2 < 1.0).all() and (trips >= 1).all() and trips.max() <= lens_ref.LENS_TRIPS
    assert 2 * lens_ref.LENS_TRIPS + 1 == 253  # the last counter the loop can read
    assert abs(1.0 / trips.mean() - np.pi / 4) < 0.02
    # a table of paths: the accepted pair re-derived draw by draw; paths that needed several trips included
    rows = np.concatenate([np.flatnonzero(trips == t)[:3] for t in (1, 2, 3, 4, 5)])
    assert len(rows) >= 12
    for i in rows:
        ctr = 2
        while True:
            x = np.float32(((int(ctr_draw(k0[i], k1[i], ctr)) >> 8) - (1 << 23)) * 2.0 ** -23)
            y = np.float32(((int(ctr_draw(k0[i], k1[i], ctr + 1)) >> 8) - (1 << 23)) * 2.0 ** -23)
            if np.float32(x * x) + np.float32(y * y) < np.float32(1.0):
                break
            ctr += 2
        assert (x, y) == (rx[i], ry[i]) and ctr == 2 * trips[i], i


def test_lens_rays_reach_the_pinhole_point_of_the_plane_of_focus(rt):
    """Without a lens the restatement is helpers.primary_rays bit for bit; with one every origin lies on the lens disc and every ray
    passes (to float32 accuracy) through origin + focus_dist * dir, where the pinhole ray of the same sample meets the plane of focus."""
    scene = _scene(rt, *CAMERAS[0][:5])
    cam = scene.camera
    p = rt.make_params(64, 36, 4, seed=95)
    jj, ii, ss = np.meshgrid(np.arange(36), np.arange(64), np.arange(4), indexing="ij")
    i, j, s = ii.ravel(), jj.ravel(), ss.ravel()
    o0, d0, _ = primary_rays(scene, p, i, j, s)
    o, d, _ = lens_ref.lens_rays(cam, p, i, j, s, 0.0, 1.0)
    assert np.array_equal(o.view(np.uint32), o0.view(np.uint32)) and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
    R, focus = 0.05, 10.0
    o, d, _ = lens_ref.lens_rays(cam, p, i, j, s, R, focus)
    org = np.array(list(cam.origin), np.float64)
    LU, LV = lens_ref.lens_vectors(cam, R)
    assert abs(np.linalg.norm(LU.astype(np.float64)) - R) < 1e-7 and abs(np.linalg.norm(LV.astype(np.float64)) - R) < 1e-7
    off = o.astype(np.float64) - org
    assert (np.linalg.norm(off, axis=1) <= R * (1 + 1e-5)).all() and np.linalg.norm(off, axis=1).max() > 0.9 * R
    w = -np.cross(np.array(list(cam.horizontal), np.float64), np.array(list(cam.vertical), np.float64))
    w /= np.linalg.norm(w)  # -w of camera.rs: towards the scene
    # the pinhole ray meets the plane of focus (distance focus * h along w) at origin + focus * dir: the lens ray must too
    dir0 = d0.astype(np.float64) / (d0.astype(np.float64) @ w)[:, None]  # dir scaled to reach the image plane at h = 1
    target = org + focus * dir0
    t = ((target - o.astype(np.float64)) @ w) / (d.astype(np.float64) @ w)
    hit = o.astype(np.float64) + t[:, None] * d.astype(np.float64)
    assert np.abs(hit - target).max() < 1e-4 * focus
