"""Light importance sampling without a GPU: rth_scene_lights (which emitters of a built scene become sampling targets), the density
p_L of tests/light_ref.py integrated over the sphere of directions, and the layout of RtLights against the C compiler."""
import ctypes as C
import os
import subprocess

import numpy as np

import light_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _arrays(lights):
    n = lights.n
    return tuple(np.ctypeslib.as_array(p, shape=(3 * n,)).reshape(n, 3).astype(f32) if n else np.zeros((0, 3), f32)
                 for p in (lights.q, lights.u, lights.v))


def test_cornell_box_has_its_one_light_and_sphere_scene_none(rt):
    lights = rt.Scene.build("cornell_box", 1.0).lights
    assert lights.n == 1 and lights.n_found == 1
    q, u, v = _arrays(lights)
    # demo_scene.rs:121 XZRect { min (113, 554, 127), max (443, 554, 432) } with the Emission material
    assert np.array_equal(q, f32([[113, 554, 127]])) and np.array_equal(u, f32([[330, 0, 0]])) and np.array_equal(v, f32([[0, 0, 305]]))
    none = rt.Scene.build("sphere_scene", 16 / 9).lights
    assert none.n == 0 and none.n_found == 0


def _hand_built(rt, n_rects):
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_BLACK)
    light = s.material(f.MAT_EMISSION, tex0=s.constant_tex((4, 4, 4)))
    grey = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.5, 0.5, 0.5)))
    s.rect(f.RECT_XZ, (-5, 0, -5), (5, 0, 5), grey)                       # not an emitter
    s.sphere((0, 3, 0), 0.5, light, "emissive sphere")                    # left out: a sphere
    s.translate(s.rect(f.RECT_XY, (0, 0, 0), (1, 1, 0), light), (0, 1, 0))  # left out: below a wrapper
    s.triangle((0, 2, 0), (1, 2, 0), (0, 2, 1), light)                    # left out: a triangle
    for k in range(n_rects):
        s.rect((f.RECT_YZ, f.RECT_XZ, f.RECT_XY)[k % 3], (k, 1, 2), (k + 0.5, 3, 5), light)
    s.quad((1, 4, 1), (1, 0, 0.5), (0, 0.2, 1), light)
    s.set_camera((0, 2, 10), (0, 1, 0), (0, 1, 0), 40.0, 1.0)
    return s.finish()


def test_wrapped_emitters_spheres_and_triangles_are_left_out(rt):
    lights = _hand_built(rt, 3).lights
    assert lights.n == 4 and lights.n_found == 4
    q, u, v = _arrays(lights)
    # the rectangles in world order (YZ: u along y, v along z; XZ: x, z; XY: x, y), in the plane min[axis], then the quad as given
    assert np.array_equal(q, f32([[0, 1, 2], [1, 1, 2], [2, 1, 2], [1, 4, 1]]))
    assert np.array_equal(u, f32([[0, 2, 0], [0.5, 0, 0], [0.5, 0, 0], [1, 0, 0.5]]))
    assert np.array_equal(v, f32([[0, 0, 3], [0, 0, 3], [0, 2, 0], [0, 0.2, 1]]))


def test_more_than_16_emitters_keep_the_first_16_and_report_the_count(rt):
    lights = _hand_built(rt, 19).lights
    assert lights.n == rt._ffi.MAX_LIGHTS == 16 and lights.n_found == 20
    q, _, _ = _arrays(lights)
    assert np.array_equal(q[:, 0], np.arange(16, dtype=f32))  # the first 16 rectangles; the quad behind them fell out


def test_p_light_integrates_to_one_over_the_sphere_of_directions():
    """p_L is a density over directions: for a point that sees both lights whole, its integral over the sphere is 1.  Midpoint rule in
    (cos theta, phi), equal-area cells, float64 sums of the float32 function; the two quads subtend 1.1 and 0.35 sr, their outlines are
    curves in these coordinates, so the error is the boundary cells' (about 5000 of 2.9 M cells, each off by at most half its share),
    far below the 1e-3 asked."""
    L = light_ref.setup([[-1.0, 1.5, -1.0], [2.0, -0.5, 0.2]], [[2.0, 0.0, 0.0], [0.0, 1.5, 0.3]], [[0.0, 0.3, 2.0], [0.2, 0.0, 1.2]])
    po = f32([0.1, -0.2, 0.05])
    nz, nphi = 1200, 2400
    z = (np.arange(nz) + 0.5) / nz * 2.0 - 1.0
    phi = (np.arange(nphi) + 0.5) / nphi * 2.0 * np.pi
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - zz * zz)
    d = np.stack([r * np.cos(pp), r * np.sin(pp), zz], axis=-1).reshape(-1, 3).astype(f32)
    p_l, count = light_ref.p_light(L, np.broadcast_to(po, d.shape), d)
    integral = float(p_l.astype(np.float64).sum()) * (4.0 * np.pi / (nz * nphi))
    assert (count == 1).sum() > 1000 and (count == 0).sum() > 1000
    assert abs(integral - 1.0) <= 1e-3, integral


def test_rtlights_layout_matches_the_c_compiler(rt, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x.h"\nint main(void){printf("%zu %zu %zu %zu %zu %u\\n",'
                   'sizeof(RtLights),offsetof(RtLights,n),offsetof(RtLights,q),offsetof(RtLights,u),offsetof(RtLights,v),RT_MAX_LIGHTS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    f = rt._ffi
    assert got == [C.sizeof(f.RtLights), f.RtLights.n.offset, f.RtLights.q.offset, f.RtLights.u.offset, f.RtLights.v.offset, f.MAX_LIGHTS]
