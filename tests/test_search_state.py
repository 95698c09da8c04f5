"""The search state of one context through every transition that builds, replaces or puts it back (rt_scene_upload, rt_set_motion,
rt_set_quads, rt_set_lights and their clears): after each step the context must render the very bytes, and report the very
rt_debug_scene_info, of a context that was created fresh and brought to that state directly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32


def _quads(rt, n, scale=1.0, at=(0.0, 1.0, 0.0), mat=0):
    """n planar primitives (quads and triangles in turn) around `at`"""
    c = np.array(at, f32)
    q = np.array([c + f32([-1, 0, 0]) * scale, c + f32([0.2, 0.1, 0.5]) * scale, c + f32([-0.4, 0.6, -0.8]) * scale], f32)[:n]
    u = (np.array([[1.5, 0.3, 0.2], [0.0, 1.0, 0.4], [0.7, 0.0, 0.9]], f32) * f32(scale))[:n]
    v = (np.array([[0.1, 1.2, -0.3], [0.9, 0.1, -0.5], [0.0, 0.8, 0.1]], f32) * f32(scale))[:n]
    return rt.make_quads(q, u, v, [0, 1, 0][:n], [mat] * n)


def test_one_context_walks_every_search_state(rt):
    spheres = rt.Scene.build("sphere_scene", 64 / 36)
    cornell = rt.Scene.build("cornell_box", 1.0)
    p_sph = rt.make_params(64, 36, 2, max_depth=4, seed=7)
    p_cor = rt.make_params(48, 48, 2, max_depth=4, seed=7)
    a = spheres.arrays()
    moved = 5  # a bare sphere
    motion = rt.make_motion([moved], [[a["sph_cx"][moved] + f32(0.3), a["sph_cy"][moved] + f32(0.2), a["sph_cz"][moved]]])
    set_a, set_b = _quads(rt, 2), _quads(rt, 3, 0.5, (0.5, 0.8, 0.3))
    set_c = _quads(rt, 2, 150.0, (278.0, 200.0, 278.0))
    light = rt.make_lights([[-1.0, 3.0, -1.0]], [[2.0, 0.0, 0.0]], [[0.0, 0.0, 2.0]])

    def up(scene):
        return lambda r: r.upload(scene)

    # (what the step does to the walking context, how a fresh context gets to the same state, scene, params)
    first = [up(spheres)]
    walk = [
        ("upload", up(spheres), first, spheres, p_sph),
        ("set_motion", lambda r: r.set_motion(motion), [up(spheres), lambda r: r.set_motion(motion)], spheres, p_sph),
        ("set_motion(None)", lambda r: r.set_motion(None), first, spheres, p_sph),
        ("set_quads", lambda r: r.set_quads(set_a), [up(spheres), lambda r: r.set_quads(set_a)], spheres, p_sph),
        ("set_lights", lambda r: r.set_lights(light), [up(spheres), lambda r: r.set_quads(set_a), lambda r: r.set_lights(light)], spheres, p_sph),
        ("set_quads replaces", lambda r: r.set_quads(set_b), [up(spheres), lambda r: r.set_quads(set_b), lambda r: r.set_lights(light)], spheres, p_sph),
        ("set_quads(None), lights stay", lambda r: r.set_quads(None), [up(spheres), lambda r: r.set_lights(light)], spheres, p_sph),
        ("set_lights(None)", lambda r: r.set_lights(None), first, spheres, p_sph),
        ("upload cornell_box", up(cornell), [up(cornell)], cornell, p_cor),
        ("set_quads on cornell_box", lambda r: r.set_quads(set_c), [up(cornell), lambda r: r.set_quads(set_c)], cornell, p_cor),
        ("upload sphere_scene again", up(spheres), first, spheres, p_sph),
    ]

    def state(r, scene, p):
        return r.render(scene.camera, p)[0].tobytes(), r.scene_info()

    want_first = None  # the first stop's reference, computed once: the stops after the clears and the last upload must equal it
    seen = []
    r = rt.Renderer(0)
    try:
        for what, step, direct, scene, p in walk:
            step(r)
            got = state(r, scene, p)
            if direct is first and want_first is not None:
                want = want_first
            else:
                ref = rt.Renderer(0)
                try:
                    for s in direct:
                        s(ref)
                    want = state(ref, scene, p)
                finally:
                    ref.close()
                if direct is first:
                    want_first = want
            assert got[1] == want[1], (what, {k: (got[1][k], want[1][k]) for k in want[1] if got[1][k] != want[1][k]})
            assert got[0] == want[0], (what, "the frame differs from a fresh context's")
            seen.append((what, got))
    finally:
        r.close()
    # the walk went somewhere: every set shows in the frame and in the tree, and cornell_box is the general tree path without a grid
    by = dict(seen)
    for what in ("set_motion", "set_quads", "set_lights", "set_quads replaces", "set_quads(None), lights stay"):
        assert by[what][0] != by["upload"][0], what
    assert by["upload"][1]["grid"] and by["upload"][1]["n_planar"] == 0
    assert by["set_quads"][1]["n_planar"] == 2 and by["set_quads replaces"][1]["n_planar"] == 3 and not by["set_quads"][1]["grid"]
    assert by["upload cornell_box"][1]["general_kernels"] and not by["upload cornell_box"][1]["grid"] and by["upload cornell_box"][1]["n_tree_nodes"] > 0
    assert by["set_quads on cornell_box"][1]["n_planar"] == 2
