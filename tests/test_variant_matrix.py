"""Every kernel instantiation launched and checked (csrc/rt_api.hip "kernel variants"): one test per row of tests/variant_matrix.py.
A row uploads its scene with its options and set, shows the placement it names, and then — with the context's launch ledger reset —
sends its single rays through the production kernels (the non-GEN k_shade and k_intersect keys) and through rt_debug_bounce with the
tree and with the list walk (the k_debug_bounce keys) against the row's reference, renders its frames on the default path, with the
list walk and with materialised primaries, without and with a lens (GEN and GEN|LENS tied bit for bit to the non-GEN keys, every tree
to the list walk), and at the end the ledger equals the row's claims exactly: a launch the row does not claim fails like a claim that
was not launched.  tests/test_variant_matrix_host.py shows that the claims of all rows are the tables."""
import numpy as np
import pytest

import variant_matrix as vm
from test_gpu_parity import _compare_frames, _oracle, _rays_agree

pytestmark = pytest.mark.gpu
_bits = vm._bits


@pytest.fixture
def fresh(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


def _same(a, b, what):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), (what, int((_bits(a[0]) != _bits(b[0])).any(axis=2).sum()), "pixels differ")
    assert a[2].n_rays == b[2].n_rays and list(a[2].rays_per_depth) == list(b[2].rays_per_depth), what


def _apply_sets(r, B, lights=True):
    if B["motion"] is not None:
        r.set_motion(B["motion"])
    if B["quads"] is not None:
        r.set_quads(B["quads"])
    r.set_lights(B["lights"] if lights else None)


@pytest.mark.parametrize("name", vm.ROW_NAMES)
def test_row(rt, orc, fresh, name):
    f = rt._ffi
    row = vm.ROWS[vm.ROW_NAMES.index(name)]
    X = vm.expected(rt, orc, row)
    vm.check_coverage(row, X["stats"])
    B, o, d, keys = X["B"], X["o"], X["d"], X["keys"]
    scene = B["scene"]
    r = fresh
    for opt, val in row["opts"].items():
        r.set_option(opt, val)
    r.upload(scene)
    _apply_sets(r, B)
    info = r.scene_info()
    assert {k: info[k] for k in row["info"]} == row["info"], info
    if row["grid"]:
        assert (info["grid_cells"][1] == 1) == (row["grid"] == "flat"), info["grid_cells"]
    r.launched_variants(reset=True)

    # a. single rays through the production kernels
    p = r.debug_bounce(o, d, keys, depth=vm.DEPTH, flags=f.FLAG_PRODUCTION_KERNELS)
    vm.check_rays(p, X, "production kernels", production=True)
    # b. the same rays through rt_debug_bounce: tree and list walk, byte for byte, and against the reference
    g = r.debug_bounce(o, d, keys, depth=vm.DEPTH)
    b = r.debug_bounce(o, d, keys, depth=vm.DEPTH, flags=f.FLAG_BRUTE_FORCE)
    for k in g:
        assert np.array_equal(g[k].view(np.uint8), b[k].view(np.uint8)), ("tree against list walk", k)
    vm.check_rays(g, X, "rt_debug_bounce", production=False)

    # c. frames: default path == list walk == materialised primaries, without and with a lens
    prm = rt.make_params(seed=7 + vm.ROW_NAMES.index(name), **vm.FRAME)
    brute = rt.make_params(seed=7 + vm.ROW_NAMES.index(name), flags=f.FLAG_BRUTE_FORCE, **vm.FRAME)
    for lens in (None, vm.LENS):
        r.set_lens(lens)
        ref = r.render(scene.camera, prm)
        if row["grid"]:
            assert r.render_parts()["primary_lists_overflow"] == 0  # depth 0 from the candidate lists alone: no k_intersect<GEN>
        _same(ref, r.render(scene.camera, brute), ("list walk", lens))
        r.set_option("materialise_primaries", 1)
        _same(ref, r.render(scene.camera, prm), ("materialised primaries", lens))
        r.set_option("materialise_primaries", 0)
        if lens is None and not row["sets"]:  # a static row: the oracle's image too
            img, _, st = ref
            want, _, so = _oracle(orc, scene, prm, accel=orc.ACCEL_LIST)
            _rays_agree(st, so, scene, prm)
            _compare_frames(orc, scene, prm, img, want, name, rt, r)
    r.set_lens(None)

    # d. the ledger: exactly what the row claims
    launched = r.launched_variants()
    claims = vm.claims(rt, row)
    for family in claims:
        assert launched[family] == claims[family], (family, "launched, not claimed:", sorted(launched[family] - claims[family]),
                                                    "claimed, not launched:", sorted(claims[family] - launched[family]))

    # rays the set does not touch equal the same call without the set bit for bit: every ray a light set leaves to the oracle, and
    # under any set the rays that meet a Perlin-textured primitive which the scene without the set shows them too
    if row["sets"] and ("lights" in row["sets"] or row["perlin"]):
        _apply_sets(r, B, lights=False)
        if "lights" not in row["sets"]:
            r.upload(scene)  # (clears motion and planar set)
        plain = r.debug_bounce(o, d, keys, depth=vm.DEPTH, flags=f.FLAG_PRODUCTION_KERNELS)
        sel = ~X["restated"] if "lights" in row["sets"] else (X["perlin_ray"] & (plain["hit"] == X["want"]["hit"]) & (_bits(plain["t"]) == _bits(X["want"]["t"])))
        assert sel.sum() >= 100, int(sel.sum())
        for k in p:
            assert np.array_equal(_bits(p[k][sel]), _bits(plain[k][sel])), ("without the set", k)
