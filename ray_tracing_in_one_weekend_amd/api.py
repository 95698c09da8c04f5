"""Host-side Python surface over the two C ABIs.

`Scene` wraps the C++ mirror of the reference's constructors (librtow_host.so);
`Renderer` wraps the GPU library (librtow_mi355x.so).  Nothing here computes pixels: every
render call goes through the HIP kernels, and a missing GPU library raises.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import RtAdaptive, RtAdaptiveInfo, RtBounceIO, RtCamera, RtDenoise, RtDisplay, RtDisplayInfo, RtFlatScene, RtGlare, RtGlareInfo, RtLens, RtLights, RtMotion, RtNoise, RtParams, RtQuads, RtResidual, RtSelect, RtSelectInfo, RtStats


class RtError(RuntimeError):
    pass


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _lens_ptr(lens):
    """None -> NULL (the pinhole); an RtLens or a (lens_radius, focus_dist) pair -> a pointer to an RtLens"""
    if lens is None:
        return None
    if not isinstance(lens, RtLens):
        lens = RtLens(*[float(x) for x in lens])
    return C.byref(lens)


def make_motion(spheres, center1, shutter=(0.0, 1.0)):
    """An RtMotion (with its arrays kept alive on it) from sphere indices, their centres at time 1 [n, 3] and the shutter interval."""
    idx = np.ascontiguousarray(spheres, dtype=np.uint32).ravel()
    c1 = np.ascontiguousarray(center1, dtype=np.float32).reshape(-1)
    if c1.size != 3 * idx.size:
        raise RtError("make_motion: center1 must hold three floats per listed sphere")
    m = RtMotion(idx.size, idx.ctypes.data_as(C.POINTER(C.c_uint32)), c1.ctypes.data_as(C.POINTER(C.c_float)), float(shutter[0]), float(shutter[1]))
    m._keep = (idx, c1)
    return m


def _motion_ptr(motion):
    """None -> NULL (the static renderer); an RtMotion (Scene.motion, make_motion) -> a pointer to it"""
    if motion is None:
        return None
    if not isinstance(motion, RtMotion):
        motion = make_motion(*motion)
    return C.byref(motion)


def make_quads(q, u, v, kind, mat):
    """An RtQuads (with its arrays kept alive on it) from corners Q [n, 3], edge vectors u, v [n, 3], kinds [n] (0 quad, 1 triangle) and
    material indices [n] of the uploaded scene."""
    qa = np.ascontiguousarray(q, dtype=np.float32).reshape(-1)
    ua = np.ascontiguousarray(u, dtype=np.float32).reshape(-1)
    va = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    ka = np.ascontiguousarray(kind, dtype=np.uint8).ravel()
    ma = np.ascontiguousarray(mat, dtype=np.uint32).ravel()
    n = ka.size
    if not (qa.size == ua.size == va.size == 3 * n and ma.size == n):
        raise RtError("make_quads: q, u, v must hold three floats and kind, mat one entry per primitive")
    fp = C.POINTER(C.c_float)
    s = RtQuads(n, qa.ctypes.data_as(fp), ua.ctypes.data_as(fp), va.ctypes.data_as(fp), ka.ctypes.data_as(C.POINTER(C.c_uint8)),
                ma.ctypes.data_as(C.POINTER(C.c_uint32)))
    s._keep = (qa, ua, va, ka, ma)
    return s


def _quads_ptr(quads):
    """None -> NULL (no planar primitives); an RtQuads (Scene.quads, make_quads) -> a pointer to it"""
    if quads is None:
        return None
    if not isinstance(quads, RtQuads):
        quads = make_quads(*quads)
    return C.byref(quads)


def make_lights(q, u, v):
    """An RtLights (with its arrays kept alive on it) from the world-space parallelograms Q + a u + b v: corners Q [n, 3] and edge
    vectors u, v [n, 3].  They are sampling targets only."""
    qa = np.ascontiguousarray(q, dtype=np.float32).reshape(-1)
    ua = np.ascontiguousarray(u, dtype=np.float32).reshape(-1)
    va = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    if not (qa.size == ua.size == va.size and qa.size % 3 == 0):
        raise RtError("make_lights: q, u, v must hold three floats per light")
    fp = C.POINTER(C.c_float)
    s = RtLights(qa.size // 3, qa.ctypes.data_as(fp), ua.ctypes.data_as(fp), va.ctypes.data_as(fp))
    s._keep = (qa, ua, va)
    return s


def _lights_ptr(lights):
    """None -> NULL (no light sampling); an RtLights (Scene.lights, make_lights) -> a pointer to it"""
    if lights is None:
        return None
    if not isinstance(lights, RtLights):
        lights = make_lights(*lights)
    return C.byref(lights)


def planar_bounds(quads, world_mag=0.0):
    """rt_debug_planar_bounds (host code, no GPU): (box [n, 6], slack [n]) — the leaf box of every primitive before the tree's pad and
    the slack it was grown by."""
    lib = _ffi.load_gpu_library()
    if not isinstance(quads, RtQuads):
        quads = make_quads(*quads)
    box = np.zeros((quads.n, 6), np.float32)
    slack = np.zeros(quads.n, np.float32)
    rc = lib.rt_debug_planar_bounds(C.byref(quads), C.c_float(world_mag), box.ctypes.data, slack.ctypes.data)
    if rc != 0:
        raise RtError("rt_debug_planar_bounds", rc)
    return box, slack


class Scene:
    """A flattened scene + camera built with the reference's constructors
    (demo_scene.rs scene fns, or piecewise: textures -> materials -> spheres -> camera)."""

    def __init__(self, handle):
        self._lib = _ffi.load_host_library()
        self._h = handle

    # -- named scene functions (demo_scene.rs:37,229 + the two build-authored ones) --------
    @classmethod
    def build(cls, name, aspect_ratio):
        lib = _ffi.load_host_library()
        h = C.c_void_p()
        rc = lib.rth_scene_build(name.encode(), C.c_float(aspect_ratio), C.byref(h))
        if rc != 0:
            raise RtError(lib.rth_last_error().decode())
        return cls(h)

    # -- piecewise construction ----------------------------------------------------------------
    @classmethod
    def new(cls):
        lib = _ffi.load_host_library()
        h = C.c_void_p()
        if lib.rth_scene_new(C.byref(h)) != 0:
            raise RtError(lib.rth_last_error().decode())
        return cls(h)

    def _check(self, handle):
        if handle == _ffi.RTH_INVALID:
            raise RtError(self._lib.rth_last_error().decode())
        return handle

    def constant_tex(self, col):
        return self._check(self._lib.rth_tex_constant(self._h, _f3(col)))

    def checker_tex(self, odd, even):
        return self._check(self._lib.rth_tex_checker(self._h, _f3(odd), _f3(even)))

    def perlin_tex(self, scale):
        return self._check(self._lib.rth_tex_perlin(self._h, C.c_float(scale)))

    def image_tex(self, path):
        return self._check(self._lib.rth_tex_image(self._h, path.encode()))

    def material(self, mat_type, tex0=_ffi.RTH_INVALID, tex1=_ffi.RTH_INVALID, color=(0, 0, 0), p=(0, 0, 0, 0)):
        p = list(p) + [0.0] * (4 - len(p))
        return self._check(self._lib.rth_material(self._h, mat_type, tex0, tex1, _f3(color),
                                                  (C.c_float * 4)(*[float(x) for x in p])))

    def sphere(self, c, r, material, name=""):
        return self._check(self._lib.rth_sphere(self._h, _f3(c), C.c_float(r), material, name.encode()))

    def moving_sphere(self, c0, c1, r, material, name=""):
        """A sphere whose centre moves linearly from c0 (time 0) to c1 (time 1): motion blur.  Only at the top level of the world."""
        return self._check(self._lib.rth_moving_sphere(self._h, _f3(c0), _f3(c1), C.c_float(r), material, name.encode()))

    def quad(self, q, u, v, material):
        """The parallelogram Q + a u + b v, 0 <= a, b <= 1 ("The Next Week" ch. 6).  Only at the top level of the world; it becomes an entry
        of Scene.quads."""
        return self._check(self._lib.rth_quad(self._h, _f3(q), _f3(u), _f3(v), material))

    def triangle(self, a, b, c, material):
        """The triangle with the corners a, b, c, stored as Q = a, u = b - a, v = c - a.  Only at the top level of the world."""
        return self._check(self._lib.rth_triangle(self._h, _f3(a), _f3(b), _f3(c), material))

    def rect(self, axis, mn, mx, material):
        return self._check(self._lib.rth_rect(self._h, axis, _f3(mn), _f3(mx), material))

    def gbox(self, mn, mx, material):
        return self._check(self._lib.rth_gbox(self._h, _f3(mn), _f3(mx), material))

    def translate(self, hitable, offset):
        return self._check(self._lib.rth_translate(self._h, hitable, _f3(offset)))

    def rotate_y(self, hitable, angle_degrees):
        return self._check(self._lib.rth_rotate_y(self._h, hitable, C.c_float(angle_degrees)))

    def constant_medium(self, hitable, density, phase_tex):
        return self._check(self._lib.rth_constant_medium(self._h, hitable, C.c_float(density), phase_tex))

    def bbox(self, hitable):
        """Hitable::bbox of a world entry (hitable.rs:52): (has_box, [min.xyz, max.xyz])."""
        out = (C.c_float * 6)()
        rc = self._lib.rth_hitable_bbox(self._h, hitable, out)
        if rc < 0:
            raise RtError(self._lib.rth_last_error().decode())
        return bool(rc), np.array(out, dtype=np.float32)

    def set_sky(self, sky, env_path=None):
        if self._lib.rth_set_sky(self._h, sky, env_path.encode() if env_path else None) != 0:
            raise RtError(self._lib.rth_last_error().decode())

    def set_camera(self, lookfrom, lookat, vup, vfov, aspect_ratio, aperture=0.0, focus_dist=1.0, shutter=(0.0, 1.0)):
        """Camera::new (camera.rs:14-39); with an aperture, the book's thin-lens camera (chapter 13): the same RtCamera, and
        Scene.lens = (aperture / 2, focus_dist) for Renderer.set_lens.  shutter = (open, close) within [0, 1]: the interval the
        times of Scene.motion are drawn from."""
        if aperture == 0.0 and focus_dist == 1.0:
            rc = self._lib.rth_set_camera(self._h, _f3(lookfrom), _f3(lookat), _f3(vup), C.c_float(vfov), C.c_float(aspect_ratio))
        else:
            rc = self._lib.rth_set_camera_lens(self._h, _f3(lookfrom), _f3(lookat), _f3(vup), C.c_float(vfov), C.c_float(aspect_ratio),
                                               C.c_float(aperture), C.c_float(focus_dist))
        if rc != 0:
            raise RtError(self._lib.rth_last_error().decode())
        if tuple(shutter) != (0.0, 1.0) and self._lib.rth_set_camera_shutter(self._h, C.c_float(shutter[0]), C.c_float(shutter[1])) != 0:
            raise RtError(self._lib.rth_last_error().decode())

    def finish(self, use_bvh=True):
        if self._lib.rth_scene_finish(self._h, 1 if use_bvh else 0) != 0:
            raise RtError(self._lib.rth_last_error().decode())
        return self

    # -- accessors ----------------------------------------------------------------------------------
    @property
    def flat(self):
        p = self._lib.rth_scene_flat(self._h)
        if not p:
            raise RtError("scene not finished")
        return p.contents

    @property
    def flat_ptr(self):
        p = self._lib.rth_scene_flat(self._h)
        if not p:
            raise RtError("scene not finished")
        return p

    @property
    def camera(self):
        cam = RtCamera()
        if self._lib.rth_scene_camera(self._h, C.byref(cam)) != 0:
            raise RtError("scene not finished")
        return cam

    @property
    def lens(self):
        """RtLens of the camera (rth_scene_lens): (0, 1) for a pinhole one.  Renderer.upload does not apply it: pass it to set_lens."""
        lens = RtLens()
        if self._lib.rth_scene_lens(self._h, C.byref(lens)) != 0:
            raise RtError("scene not finished")
        return lens

    @property
    def motion(self):
        """RtMotion of the scene (rth_scene_motion): its moving spheres and the camera's shutter; n_moving 0 for a static scene.  It
        points into the scene.  Renderer.upload does not apply it: pass it to set_motion."""
        m = RtMotion()
        if self._lib.rth_scene_motion(self._h, C.byref(m)) != 0:
            raise RtError("scene not finished")
        m._keep = self
        return m

    @property
    def quads(self):
        """RtQuads of the scene (rth_scene_quads): its planar primitives; n 0 for a scene without any.  It points into the scene.
        Renderer.upload does not apply it: pass it to set_quads."""
        s = RtQuads()
        if self._lib.rth_scene_quads(self._h, C.byref(s)) != 0:
            raise RtError("scene not finished")
        s._keep = self
        return s

    @property
    def lights(self):
        """RtLights of the scene (rth_scene_lights): the parallelograms of its bare Emission rectangles and quads, at most 16 (n_found
        on the result: how many there were); n 0 for a scene without any.  Emitters below wrappers, spheres and triangles are left out.
        It points into the scene.  Renderer.upload does not apply it: pass it to set_lights."""
        s = RtLights()
        found = C.c_uint32(0)
        if self._lib.rth_scene_lights(self._h, C.byref(s), C.byref(found)) != 0:
            raise RtError("scene not finished")
        s._keep = self
        s.n_found = found.value
        return s

    def sphere_name(self, i):
        return self._lib.rth_scene_sphere_name(self._h, i).decode()

    def arrays(self):
        """numpy copies of the flat arrays (for tests and inspection)."""
        fs = self.flat

        def arr(ptr, n, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)
        ns, nm, nt = fs.n_spheres, fs.n_materials, fs.n_textures
        return {
            "sph_cx": arr(fs.sph_cx, ns, np.float32), "sph_cy": arr(fs.sph_cy, ns, np.float32),
            "sph_cz": arr(fs.sph_cz, ns, np.float32), "sph_r": arr(fs.sph_r, ns, np.float32),
            "sph_mat": arr(fs.sph_mat, ns, np.uint32),
            "rect_axis": arr(fs.rect_axis, fs.n_rects, np.uint8), "rect_min": arr(fs.rect_min, 3 * fs.n_rects, np.float32),
            "rect_max": arr(fs.rect_max, 3 * fs.n_rects, np.float32), "rect_mat": arr(fs.rect_mat, fs.n_rects, np.uint32),
            "xf_type": arr(fs.xf_type, fs.n_xforms, np.uint8), "xf_param": arr(fs.xf_param, 4 * fs.n_xforms, np.float32),
            "xf_parent": arr(fs.xf_parent, fs.n_xforms, np.uint32), "sph_xform": arr(fs.sph_xform, ns, np.uint32),
            "rect_xform": arr(fs.rect_xform, fs.n_rects, np.uint32),
            "med_neg_inv_density": arr(fs.med_neg_inv_density, fs.n_media, np.float32), "med_mat": arr(fs.med_mat, fs.n_media, np.uint32),
            "sph_medium": arr(fs.sph_medium, ns, np.uint32), "rect_medium": arr(fs.rect_medium, fs.n_rects, np.uint32),
            "med_xform": arr(fs.med_xform, fs.n_media, np.uint32),
            "mat_type": arr(fs.mat_type, nm, np.uint8), "mat_color": arr(fs.mat_color, 3 * nm, np.float32),
            "mat_p0": arr(fs.mat_p0, nm, np.float32), "mat_p1": arr(fs.mat_p1, nm, np.float32),
            "mat_p2": arr(fs.mat_p2, nm, np.float32), "mat_p3": arr(fs.mat_p3, nm, np.float32),
            "mat_tex0": arr(fs.mat_tex0, nm, np.uint32), "mat_tex1": arr(fs.mat_tex1, nm, np.uint32),
            "tex_type": arr(fs.tex_type, nt, np.uint8), "tex_color0": arr(fs.tex_color0, 3 * nt, np.float32),
            "tex_color1": arr(fs.tex_color1, 3 * nt, np.float32), "tex_scale": arr(fs.tex_scale, nt, np.float32),
            "tex_aux": arr(fs.tex_aux, nt, np.uint32),
            "perlin_vec": arr(fs.perlin_vec, fs.n_perlin * 768, np.float32),
            "perlin_perm": arr(fs.perlin_perm, fs.n_perlin * 768, np.uint16),
            "img_w": arr(fs.img_w, fs.n_images, np.uint32), "img_h": arr(fs.img_h, fs.n_images, np.uint32),
            "sky_type": fs.sky_type, "sky_image": fs.sky_image,
        }

    def close(self):
        if self._h:
            self._lib.rth_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grid_build(scene, cell_per_mille=0, lds_budget=0):
    """rt_debug_grid_build (host code of the GPU library, no GPU): the uniform grid rt_scene_upload would build over the spheres
    of `scene`, or None when the scene gets none.  -> dict(origin[3], cell[3], pad, max_coord, dims[3], cells u32 [nz, ny, nx]
    (offset << 12 | count), refs u16, large: list)."""
    lib = _ffi.load_gpu_library()
    ptr = scene.flat_ptr if isinstance(scene, Scene) else C.pointer(scene)
    grid, dims, large = (C.c_float * 8)(), (C.c_uint32 * 3)(), (C.c_uint32 * 4)()
    nc, nr, nl = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib.rt_debug_grid_build(ptr, cell_per_mille, lds_budget, grid, dims, None, C.byref(nc), None, C.byref(nr), large, C.byref(nl))
    if rc == -4:  # RT_ERR_UNSUPPORTED: no grid for this scene
        return None
    cells = np.zeros(max(nc.value, 1), np.uint32)
    refs = np.zeros(max(nr.value, 1), np.uint16)
    rc = lib.rt_debug_grid_build(ptr, cell_per_mille, lds_budget, grid, dims, cells.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nc),
                                 refs.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(nr), large, C.byref(nl))
    if rc != 0:
        raise RtError(f"rt_debug_grid_build failed ({rc})")
    d = [int(x) for x in dims]
    return {"origin": np.array(grid[0:3], np.float32), "cell": np.array(grid[3:6], np.float32), "pad": float(grid[6]), "max_coord": float(grid[7]),
            "dims": d, "cells": cells[:nc.value].reshape(d[2], d[1], d[0]), "refs": refs[:nr.value], "large": [int(large[k]) for k in range(nl.value)]}


def world_bounds(scene):
    """rt_debug_world_bounds (host code of the GPU library, no GPU): the world-space bounds rt_scene_upload culls with.
    -> dict(prim_box f32 [n_prims, 2, 3] (before the tree's pad), prim_box_padded [n_prims, 2, 3], world_sphere [n_spheres, 4],
    entry_id u32 [n_entries], entry_box_padded [n_entries, 2, 3], entry_bs [n_entries, 4]); primitives are the spheres, then the
    rectangles; entries the primitives that are not a medium boundary, then the media (id n_prims + m)."""
    lib = _ffi.load_gpu_library()
    ptr = scene.flat_ptr if isinstance(scene, Scene) else C.pointer(scene)
    fs = ptr.contents
    n_prims = fs.n_spheres + fs.n_rects
    cap = n_prims + fs.n_media
    out = {"prim_box": np.zeros((max(n_prims, 1), 2, 3), np.float32), "prim_box_padded": np.zeros((max(n_prims, 1), 2, 3), np.float32),
           "world_sphere": np.zeros((max(fs.n_spheres, 1), 4), np.float32), "entry_id": np.zeros(max(cap, 1), np.uint32),
           "entry_box_padded": np.zeros((max(cap, 1), 2, 3), np.float32), "entry_bs": np.zeros((max(cap, 1), 4), np.float32)}
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ne = C.c_uint32(cap)
    rc = lib.rt_debug_world_bounds(ptr, fp(out["prim_box"]), fp(out["prim_box_padded"]), fp(out["world_sphere"]), C.byref(ne),
                                   out["entry_id"].ctypes.data_as(C.POINTER(C.c_uint32)), fp(out["entry_box_padded"]), fp(out["entry_bs"]))
    if rc != 0:
        raise RtError(f"rt_debug_world_bounds failed ({rc})")
    for k in ("prim_box", "prim_box_padded"):
        out[k] = out[k][:n_prims]
    out["world_sphere"] = out["world_sphere"][:fs.n_spheres]
    for k in ("entry_id", "entry_box_padded", "entry_bs"):
        out[k] = out[k][:ne.value]
    return out


def variant_flag_names(family):
    """rt_debug_variant_flag_names: the flag names of a kernel family (_ffi.FAMILY_*) in bit order, read from the library."""
    lib = _ffi.load_gpu_library()
    buf = C.create_string_buffer(512)
    n = lib.rt_debug_variant_flag_names(family, buf, len(buf))
    if n < 0 or n > len(buf):
        raise RtError(f"rt_debug_variant_flag_names({family}) failed ({n})")
    return tuple(buf.value.decode().split())


def _ledger_sets(ledger):
    """An RtVariantLedger as {"shade": {flag-name tuples}, "intersect": {..}, "debug_bounce": {(form, flag names..)}, "untabled": {kernel
    names}}; a key without flags is the empty tuple.  The bits are named by the library (variant_flag_names)."""
    def keys(words, names):
        out = set()
        for k in range(32 * len(words)):
            if words[k >> 5] >> (k & 31) & 1:
                out.add(tuple(n for b, n in enumerate(names) if k >> b & 1))
        return out
    db = variant_flag_names(_ffi.FAMILY_DEBUG_BOUNCE)
    return {"shade": keys(ledger.shade, variant_flag_names(_ffi.FAMILY_SHADE)),
            "intersect": keys(ledger.intersect, variant_flag_names(_ffi.FAMILY_INTERSECT)),
            "debug_bounce": {(form,) + k for f, form in enumerate(variant_flag_names(_ffi.FAMILY_DEBUG_FORMS)) for k in keys([ledger.debug_bounce[f]], db)},
            "untabled": {n for b, n in enumerate(variant_flag_names(_ffi.FAMILY_UNTABLED)) if ledger.untabled >> b & 1}}


def variant_tables():
    """rt_debug_variant_tables (host code, no GPU): the keys of k_shade, k_intersect and k_debug_bounce that have a kernel, as sets of
    flag-name tuples such as ("GEN", "RECTS", "NEST", "LIGHTS") (k_debug_bounce: the search form first), and the names of the closest-hit
    kernels outside the tables."""
    lib = _ffi.load_gpu_library()
    led = _ffi.RtVariantLedger()
    rc = lib.rt_debug_variant_tables(C.byref(led))
    if rc != 0:
        raise RtError(f"rt_debug_variant_tables failed ({rc})")
    return _ledger_sets(led)


class _Snapshot:
    """What AccumState, AccumHalves and AccumBuckets share: scalar fields, per-pixel arrays in the row order of the f32 image, the library's
    check of the struct over them, and an .npz file.  A subclass declares _SCALARS (the scalar fields, in the file's order), _ARRAYS (name,
    dtype, trailing shape, leading shape — a leading entry may name an attribute) and _CHECK (the library's check function), and supplies
    as_struct().  _OPTIONAL: an array that is not given stays None and is left out of the file; else it is zeros."""
    _SCALARS, _ARRAYS, _CHECK, _OPTIONAL = (), (), None, False

    def _init(self, scalars, arrays):
        for k in self._SCALARS:
            setattr(self, k, int(scalars[k]))
        for name, dt, trailing, leading in self._ARRAYS:
            shape = tuple(getattr(self, d) if isinstance(d, str) else d for d in leading) + (self.rows, self.nx) + trailing
            arr = arrays[name]
            if arr is None and not self._OPTIONAL:
                arr = np.zeros(shape, dt)
            elif arr is not None:
                arr = np.ascontiguousarray(arr, dtype=dt)
                if arr.shape != shape:
                    raise ValueError(f"{type(self).__name__}.{name}: shape {arr.shape}, expected {shape}")
            setattr(self, name, arr)

    def check(self):
        """The library's check of the struct (rt_accum_state_check, rt_accum_halves_check, rt_accum_buckets_check; no GPU): True when the
        library would accept it before comparing it with an accumulation."""
        st = self.as_struct()
        return getattr(_ffi.load_gpu_library(), self._CHECK)(C.byref(st)) == 0

    def save(self, path):
        """Writes the snapshot as an .npz at exactly `path`, through a temporary file beside it and os.replace: a process killed while
        saving leaves the previous checkpoint or none, never half of one."""
        import os
        import tempfile
        data = {k: np.asarray(getattr(self, k), dtype=np.uint64) for k in self._SCALARS}
        data.update({name: getattr(self, name) for name, *_ in self._ARRAYS if getattr(self, name) is not None})
        fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(os.path.abspath(path)))
        try:
            with os.fdopen(fd, "wb") as f:
                np.savez(f, **data)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            kw = {k: int(z[k]) for k in cls._SCALARS}
            kw.update({name: z[name] for name, *_ in cls._ARRAYS if name in z.files or not cls._OPTIONAL})
        return cls(**kw)


class AccumHalves(_Snapshot):
    """The two half buffers of an accumulation (rtow_mi355x.h "half buffers"), as numpy arrays in the row order of the f32 image plus the
    scalar fields of RtAccumHalves: sum [2, rows, nx, 3] f32 (not divided) and moments [2, rows, nx, 2] f64, half 0 (the samples with an
    even absolute index) first.  It goes with the AccumState of the same accumulation: first_sample and done are that state's."""
    _SCALARS = ("nx", "rows", "first_sample", "done", "frame_id")
    _ARRAYS = (("sum", np.float32, (3,), (2,)), ("moments", np.float64, (2,), (2,)))
    _CHECK = "rt_accum_halves_check"

    def __init__(self, nx, rows, first_sample=0, done=0, frame_id=0, sum=None, moments=None):
        self._init(dict(nx=nx, rows=rows, first_sample=first_sample, done=done, frame_id=frame_id), dict(sum=sum, moments=moments))

    def as_struct(self):
        """The RtAccumHalves over these arrays (which must stay alive while it is used)."""
        hs = _ffi.RtAccumHalves(self.nx, self.rows, self.first_sample, self.done)
        hs.frame_id = self.frame_id
        for h in range(2):
            hs.sum[h] = self.sum[h].ctypes.data_as(C.POINTER(C.c_float))
            hs.moments[h] = self.moments[h].ctypes.data_as(C.POINTER(C.c_double))
        return hs

    def counts(self, n=None):
        """(n_0, n_1): how many of the `n` samples of a pixel (default: done; an array of per-pixel counts after adaptive adds) each half holds."""
        n = np.asarray(self.done if n is None else n, dtype=np.uint64)
        n0 = n // 2 + (n & 1 & ~np.uint64(self.first_sample))
        return n0, n - n0


class AccumBuckets(_Snapshot):
    """The M sample buckets of an accumulation (rtow_mi355x.h "sample buckets"), as a numpy array in the row order of the f32 image plus the
    scalar fields of RtAccumBuckets: sum [M, rows, nx, 3] f32 (not divided), bucket b holding the samples with absolute index i % M == b.
    It goes with the AccumState of the same accumulation: first_sample and done are that state's."""
    _SCALARS = ("nx", "rows", "first_sample", "done", "M", "frame_id")
    _ARRAYS = (("sum", np.float32, (3,), ("_planes",)),)
    _CHECK = "rt_accum_buckets_check"

    def __init__(self, nx, rows, M, first_sample=0, done=0, frame_id=0, sum=None):
        self._planes = min(max(int(M), 0), _ffi.BUCKETS_MAX)  # (an M the library refuses still makes a struct: check() says so)
        self._init(dict(nx=nx, rows=rows, first_sample=first_sample, done=done, M=M, frame_id=frame_id), dict(sum=sum))

    def as_struct(self):
        """The RtAccumBuckets over this array (which must stay alive while it is used)."""
        bs = _ffi.RtAccumBuckets(self.nx, self.rows, self.first_sample, self.done, self.M, 0)
        bs.frame_id = self.frame_id
        for b in range(self.sum.shape[0]):
            bs.sum[b] = self.sum[b].ctypes.data_as(C.POINTER(C.c_float))
        return bs

    def counts(self, n=None):
        """[M, ...]: how many of the `n` samples of a pixel (default: done; an array of per-pixel counts after adaptive adds) each bucket holds."""
        n = np.asarray(self.done if n is None else n, dtype=np.uint64)
        M, f = np.uint64(self.M), np.uint64(self.first_sample % self.M)
        q, r = n // M, n % M
        return np.stack([q + (((np.uint64(b) + M - f) % M) < r).astype(np.uint64) for b in range(self.M)])


def make_params(nx, ny, spp, max_depth=50, seed=95, shard_band=0, shard_count=1, shard_id=0, spp_slice=0, flags=0):
    p = RtParams()
    p.flags = flags
    p.nx, p.ny, p.spp, p.max_depth, p.seed = nx, ny, spp, max_depth, seed
    p.shard_band, p.shard_count, p.shard_id, p.spp_slice = shard_band, shard_count, shard_id, spp_slice
    return p


def make_adaptive(tolerance, luminance_floor=0.01, min_samples=16):
    """An RtAdaptive: the stopping criterion of Renderer.accum_add_adaptive / render_adaptive."""
    return RtAdaptive(float(tolerance), float(luminance_floor), int(min_samples), 0)


def adaptive_check(ad, n_samples=1):
    """rt_adaptive_check (no GPU): True when rt_accum_add_adaptive would accept the RtAdaptive and n_samples."""
    return _ffi.load_gpu_library().rt_adaptive_check(C.byref(ad) if ad is not None else None, int(n_samples)) == 0


def adaptive_converged(ad, s1, s2, n):
    """rt_adaptive_converged (no GPU): the criterion on the luminance moments (S1, S2) of a pixel's n samples."""
    rc = _ffi.load_gpu_library().rt_adaptive_converged(C.byref(ad), float(s1), float(s2), int(n))
    if rc < 0:
        raise RtError(f"rt_adaptive_converged failed ({rc}): the RtAdaptive is outside its ranges")
    return rc == 1


_EXPOSURE_MODES = {"manual": _ffi.EXPOSURE_MANUAL, "key": _ffi.EXPOSURE_KEY, "percentile": _ffi.EXPOSURE_PERCENTILE}
_TONE_CURVES = {"clamp": _ffi.TONE_CLAMP, "reinhard": _ffi.TONE_REINHARD, "aces": _ffi.TONE_ACES}
_TRANSFERS = {"gamma2": _ffi.TRANSFER_GAMMA2, "srgb": _ffi.TRANSFER_SRGB}
_DITHERS = {"none": _ffi.DITHER_NONE, "bayer8": _ffi.DITHER_BAYER8}


def make_display(exposure=1.0, auto=None, percentile=0.99, curve="clamp", white=float("inf"), transfer="gamma2", dither="none"):
    """An RtDisplay for Renderer.set_display.  auto None: `exposure` is the multiplier e; "key": `exposure` is the key the frame's log-average
    luminance maps to (0.18 is customary); "percentile": the linear level the `percentile` quantile of the lit luminances maps to.  curve
    "clamp" | "reinhard" (with `white`, inf: none) | "aces"; transfer "gamma2" | "srgb"; dither "none" | "bayer8".  Names or the
    _ffi numbers; the defaults are the reference quantisation."""
    pick = lambda table, v: table[v] if isinstance(v, str) else int(v)
    return RtDisplay(pick(_EXPOSURE_MODES, auto or "manual"), float(exposure), float(percentile), pick(_TONE_CURVES, curve), float(white),
                     pick(_TRANSFERS, transfer), pick(_DITHERS, dither), 0)


def display_check(display):
    """rt_display_check (no GPU): True when rt_set_display would accept the RtDisplay."""
    return _ffi.load_gpu_library().rt_display_check(C.byref(display) if display is not None else None) == 0


def make_glare(amount=_ffi.GLARE_DEFAULT_AMOUNT, spread=_ffi.GLARE_DEFAULT_SPREAD, threshold=0.0, levels=_ffi.GLARE_DEFAULT_LEVELS):
    """An RtGlare for Renderer.set_glare: `amount` in [0, 1] of every pixel's bright pass leaves the pixel and is spread by a 2x pyramid of
    `levels` levels (1 .. 8), each coarser level weighted `spread` (in (0, 1]) times the one below; `threshold` >= 0: the luminance below
    which a pixel does not glow (0: every pixel does and the frame's energy is conserved)."""
    return RtGlare(float(amount), float(spread), float(threshold), int(levels))


def glare_check(glare):
    """rt_glare_check (no GPU): True when rt_set_glare would accept the RtGlare."""
    return _ffi.load_gpu_library().rt_glare_check(C.byref(glare) if glare is not None else None) == 0


_FILTER_KINDS = {"box": _ffi.FILTER_BOX, "tent": _ffi.FILTER_TENT, "gaussian": _ffi.FILTER_GAUSSIAN, "mitchell": _ffi.FILTER_MITCHELL,
                 "blackman-harris": _ffi.FILTER_BLACKMAN_HARRIS}
# kind: (radius, p0, p1) where the caller gives none
_FILTER_DEFAULTS = {_ffi.FILTER_BOX: (0.5, 0.0, 0.0), _ffi.FILTER_TENT: (1.0, 0.0, 0.0), _ffi.FILTER_GAUSSIAN: (1.5, 0.5, 0.0),
                    _ffi.FILTER_MITCHELL: (2.0, 1.0 / 3.0, 1.0 / 3.0), _ffi.FILTER_BLACKMAN_HARRIS: (1.5, 0.0, 0.0)}


def make_pixel_filter(kind, radius=None, sigma=None, B=None, C=None):
    """An RtPixelFilter for Renderer.accum_track_filter: kind "box", "tent", "gaussian", "mitchell" or "blackman-harris" (or an
    _ffi.FILTER_* value) and its radius in pixels, 0.5 .. 3.  Defaults: box 0.5; tent 1.0; Gaussian 1.5 with sigma 0.5; Mitchell 2.0
    with B = C = 1/3; Blackman-Harris 1.5."""
    if isinstance(kind, str) and kind not in _FILTER_KINDS:
        raise ValueError(f"pixel filter {kind!r}: expected one of {sorted(_FILTER_KINDS)} (or an RT_FILTER_* value)")
    k = _FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
    r, p0, p1 = _FILTER_DEFAULTS.get(k, (0.5, 0.0, 0.0))
    if k == _ffi.FILTER_GAUSSIAN and sigma is not None:
        p0 = sigma
    if k == _ffi.FILTER_MITCHELL:
        p0, p1 = (p0 if B is None else B), (p1 if C is None else C)
    return _ffi.RtPixelFilter(k, float(r if radius is None else radius), float(p0), float(p1))


def pixel_filter_check(flt):
    """rt_pixel_filter_check (no GPU): True when rt_accum_track_filter would accept the RtPixelFilter."""
    return _ffi.load_gpu_library().rt_pixel_filter_check(C.byref(flt) if flt is not None else None) == 0


def pixel_filter_table(flt):
    """rt_pixel_filter_table (no GPU): (table [256] f32 — the filter's 1-D profile at the midpoints (k + 0.5) R / 256, exactly what the
    device looks up —, reach D in pixels)."""
    table = np.zeros(_ffi.FILTER_TABLE, dtype=np.float32)
    reach = C.c_uint32(0)
    rc = _ffi.load_gpu_library().rt_pixel_filter_table(C.byref(flt), table.ctypes.data_as(C.POINTER(C.c_float)), C.byref(reach))
    if rc != 0:
        raise RtError(f"rt_pixel_filter_table failed ({rc}): the RtPixelFilter is outside its ranges")
    return table, int(reach.value)


class AccumFilter(_Snapshot):
    """The filter plane of an accumulation (rtow_mi355x.h "pixel reconstruction filters"), as a numpy array in the row order of the f32 image
    plus the scalar fields of RtAccumFilter and the filter it was summed under: plane [rows, nx, 4] f32 = (sum w r, sum w g, sum w b,
    sum w), not divided.  It goes with the AccumState of the same accumulation: first_sample and done are that state's."""
    _SCALARS = ("nx", "rows", "first_sample", "done", "frame_id", "kind", "radius_bits", "p0_bits", "p1_bits")  # (the f32 fields as their bits)
    _ARRAYS = (("plane", np.float32, (4,), ()),)
    _CHECK = "rt_accum_filter_check"

    def __init__(self, nx, rows, first_sample=0, done=0, frame_id=0, kind=0, radius_bits=0x3F000000, p0_bits=0, p1_bits=0, plane=None, filter=None):
        if filter is not None:
            kind = filter.kind
            radius_bits, p0_bits, p1_bits = (int(np.float32(x).view(np.uint32)) for x in (filter.radius, filter.p0, filter.p1))
        self._init(dict(nx=nx, rows=rows, first_sample=first_sample, done=done, frame_id=frame_id, kind=kind, radius_bits=radius_bits, p0_bits=p0_bits,
                        p1_bits=p1_bits), dict(plane=plane))

    @property
    def filter(self):
        """The RtPixelFilter the plane was summed under."""
        r, p0, p1 = (float(np.uint32(b).view(np.float32)) for b in (self.radius_bits, self.p0_bits, self.p1_bits))
        return _ffi.RtPixelFilter(self.kind, r, p0, p1)

    def as_struct(self):
        """The RtAccumFilter over this array (which must stay alive while it is used)."""
        fs = _ffi.RtAccumFilter(self.nx, self.rows, self.first_sample, self.done)
        fs.frame_id, fs.filter = self.frame_id, self.filter
        fs.plane = self.plane.ctypes.data_as(C.POINTER(C.c_float))
        return fs


FEATURE_PIXEL = np.dtype([("albedo", "<f4", (3,)), ("n_f", "<u4"), ("normal", "<f4", (3,)), ("n_h", "<u4"), ("a2", "<f8"), ("n2", "<f8"),
                          ("z1", "<f8"), ("z2", "<f8")])  # RtFeaturePixel, 64 B


def features_check(stride):
    """rt_features_check (no GPU): True when rt_accum_track_features would accept the stride."""
    return _ffi.load_gpu_library().rt_features_check(C.byref(_ffi.RtFeatures(int(stride), 0))) == 0


def make_feature_guide(use=("albedo", "normal", "depth"), k=_ffi.FEATURE_GUIDE_DEFAULT_K, tau=_ffi.FEATURE_GUIDE_DEFAULT_TAU, demodulate=False):
    """An RtFeatureGuide for Renderer.accum_denoise_features: `use` names the features that guide ("albedo", "normal", "depth"; or the
    RT_FEATURE_USE_* mask), `k` and `tau` are one value for all three or a triple (albedo, normal, depth); the defaults are the 2013
    paper's, 0.6 and 1e-3."""
    names = {"albedo": _ffi.FEATURE_USE_ALBEDO, "normal": _ffi.FEATURE_USE_NORMAL, "depth": _ffi.FEATURE_USE_DEPTH}
    if isinstance(use, int):
        mask = use
    else:
        for u in use:
            if u not in names:
                raise ValueError(f"feature {u!r}: expected one of {sorted(names)}")
        mask = sum({names[u] for u in use})
    k3 = tuple(float(x) for x in k) if np.ndim(k) else (float(k),) * 3
    t3 = tuple(float(x) for x in tau) if np.ndim(tau) else (float(tau),) * 3
    if len(k3) != 3 or len(t3) != 3:
        raise ValueError("k and tau take one value or three (albedo, normal, depth)")
    return _ffi.RtFeatureGuide(*k3, *t3, int(mask), 1 if demodulate else 0)


def feature_guide_check(guide):
    """rt_feature_guide_check (no GPU): True when rt_accum_denoise_features would accept the RtFeatureGuide."""
    return _ffi.load_gpu_library().rt_feature_guide_check(C.byref(guide) if guide is not None else None) == 0


class AccumFeatures(_Snapshot):
    """The first-hit feature records of an accumulation (rtow_mi355x.h "First-hit features"), as a numpy array in the row order of the f32
    image plus the scalar fields of RtAccumFeatures and the stride: plane [rows, nx] of FEATURE_PIXEL (sums, not divided).  It goes with the
    AccumState of the same accumulation: first_sample and done are that state's."""
    _SCALARS = ("nx", "rows", "first_sample", "done", "frame_id", "stride")
    _ARRAYS = (("plane", FEATURE_PIXEL, (), ()),)
    _CHECK = "rt_accum_features_check"

    def __init__(self, nx, rows, first_sample=0, done=0, frame_id=0, stride=1, plane=None):
        self._init(dict(nx=nx, rows=rows, first_sample=first_sample, done=done, frame_id=frame_id, stride=stride), dict(plane=plane))

    def as_struct(self):
        """The RtAccumFeatures over this array (which must stay alive while it is used)."""
        fs = _ffi.RtAccumFeatures(self.nx, self.rows, self.first_sample, self.done)
        fs.frame_id, fs.features = self.frame_id, _ffi.RtFeatures(self.stride, 0)
        fs.plane = self.plane.ctypes.data_as(C.POINTER(_ffi.RtFeaturePixel))
        return fs


def make_select(strengths=_ffi.SELECT_DEFAULT_STRENGTHS, radius=5, patch=1, error_radius=0, blend_radius=1):
    """An RtSelect for Renderer.accum_denoise_select: 2 .. 4 strictly increasing candidate strengths of the cross filter, its window radius
    and patch radius, the radius of the window the per-pixel error estimate is summed over and that of the window the choice is blended
    over (0 .. 4 each).  The defaults are those of a NULL `sel`."""
    ks = [float(k) for k in strengths]
    if len(ks) > _ffi.SELECT_MAX:
        raise ValueError(f"at most {_ffi.SELECT_MAX} strengths, got {len(ks)}")
    return RtSelect(len(ks), (C.c_float * 4)(*ks), int(radius), int(patch), int(error_radius), int(blend_radius), 0)


def select_check(sel):
    """rt_select_check (no GPU): True when rt_accum_denoise_select would accept the RtSelect (None: the defaults)."""
    return _ffi.load_gpu_library().rt_select_check(C.byref(sel) if sel is not None else None) == 0


def denoise_level_size(nx, rows, level):
    """rt_denoise_level_size (no GPU): (nx_l, rows_l) of level `level` of the pyramid accum_denoise_multiscale filters."""
    nx_l, rows_l = C.c_uint32(), C.c_uint32()
    rc = _ffi.load_gpu_library().rt_denoise_level_size(int(nx), int(rows), int(level), C.byref(nx_l), C.byref(rows_l))
    if rc < 0:
        raise RtError(f"rt_denoise_level_size failed ({rc}): nx or rows 0, or a level outside 0 .. RT_DENOISE_MAX_LEVELS - 1")
    return nx_l.value, rows_l.value


def accum_frame_id(camera, params):
    """rt_accum_frame_id (no GPU): the 64-bit identity of the frame a camera and an RtParams describe — what an AccumState carries so that
    it is only imported into, or merged with, an accumulation of the same samples.  The scene and the sets are not part of it."""
    return int(_ffi.load_gpu_library().rt_accum_frame_id(C.byref(camera), C.byref(params)))


class AccumState(_Snapshot):
    """What an accumulation owns (rtow_mi355x.h "accumulation state"), as numpy arrays in the row order of the f32 image plus the scalar
    fields of RtAccumState: sum [rows, nx, 3] f32 (not divided), moments [rows, nx, 2] f64, counts [rows, nx] u32, converged [rows, nx] u8,
    channel_moments [rows, nx, 6] f64 or None.  `planes` says which of counts / converged and channel_moments belong to the state
    (_ffi.ACCUM_STATE_*); on a uniform state counts and converged are informative (done and 0) and are not handed to the library."""
    _SCALARS = ("nx", "rows", "first_sample", "done", "planes", "frame_id")
    _ARRAYS = (("sum", np.float32, (3,), ()), ("moments", np.float64, (2,), ()), ("counts", np.uint32, (), ()), ("converged", np.uint8, (), ()),
               ("channel_moments", np.float64, (6,), ()))
    _CHECK = "rt_accum_state_check"
    _OPTIONAL = True

    def __init__(self, nx, rows, first_sample=0, done=0, planes=0, frame_id=0, sum=None, moments=None, counts=None, converged=None,
                 channel_moments=None):
        self._init(dict(nx=nx, rows=rows, first_sample=first_sample, done=done, planes=planes, frame_id=frame_id),
                   dict(sum=sum, moments=moments, counts=counts, converged=converged, channel_moments=channel_moments))

    @property
    def adaptive(self):
        return bool(self.planes & _ffi.ACCUM_STATE_COUNTS)

    @property
    def channels(self):
        return bool(self.planes & _ffi.ACCUM_STATE_CHANNELS)

    def as_struct(self):
        """The RtAccumState over these arrays (which must stay alive while it is used): the planes that `planes` names, NULL for the others."""
        def ptr(arr, ctype):
            return arr.ctypes.data_as(C.POINTER(ctype)) if arr is not None else None
        st = _ffi.RtAccumState(self.nx, self.rows, self.first_sample, self.done, self.planes, 0, self.frame_id)
        st.sum, st.moments = ptr(self.sum, C.c_float), ptr(self.moments, C.c_double)
        if self.adaptive:
            st.counts, st.converged = ptr(self.counts, C.c_uint32), ptr(self.converged, C.c_uint8)
        if self.channels:
            st.channel_moments = ptr(self.channel_moments, C.c_double)
        return st


class Renderer:
    """One GPU context (rt_ctx_create).  Replaces the render half of main.rs:62-129."""

    def __init__(self, device=0):
        self._lib = _ffi.load_gpu_library()  # raises GpuLibraryMissing: no fallback
        self._ctx = C.c_void_p()
        rc = self._lib.rt_ctx_create(device, C.byref(self._ctx))
        if rc != 0:
            raise RtError(f"rt_ctx_create({device}) failed ({rc}): {self._lib.rt_last_error(None).decode()}")
        self.device = device

    def _raise(self, what, rc):
        raise RtError(f"{what} failed ({rc}): {self._lib.rt_last_error(self._ctx).decode()}")

    def _call(self, what, *args):
        """The library's function `what` on this context; anything but RT_OK raises with the context's last error."""
        rc = getattr(self._lib, what)(self._ctx, *args)
        if rc != 0:
            self._raise(what, rc)

    @property
    def build_id(self):
        """rt_build_id(): hash of the device sources + compiler flags the loaded library was built from."""
        return self._lib.rt_build_id().decode()

    def upload(self, scene):
        ptr = scene.flat_ptr if isinstance(scene, Scene) else C.pointer(scene)
        self._call("rt_scene_upload", ptr)

    def prepare(self, params):
        """rt_prepare: start requesting the work buffers of the frame `params` describes (a helper thread inside the library);
        call it before building the scene, as a host that knows its frame size up front would (main.rs:64-67)."""
        self._call("rt_prepare", C.byref(params))

    def set_option(self, option, value):
        """rt_debug_set_option: `option` an _ffi.OPT_* number or its lower-case name.  Per context; every setting renders the
        same bits (they select between equivalent search structures / placements / orders).  Upload-time options
        (tree_placement, texel_pool, grid_cell, general_lds) take effect at the next upload()."""
        opt = _ffi.OPT_NAMES[option] if isinstance(option, str) else int(option)
        self._call("rt_debug_set_option", opt, int(value))

    def get_option(self, option):
        opt = _ffi.OPT_NAMES[option] if isinstance(option, str) else int(option)
        v = C.c_uint32()
        self._call("rt_debug_get_option", opt, C.byref(v))
        return v.value

    def scene_info(self):
        """rt_debug_scene_info as a dict: what upload() built for the closest-hit search (tree placement, grid or not)."""
        info = _ffi.RtSceneInfo()
        self._call("rt_debug_scene_info", C.byref(info))
        d = info.as_dict()
        n, lds = C.c_uint32(0), C.c_uint32(0)
        self._call("rt_debug_planar_info", C.byref(n), C.byref(lds))
        d["n_planar"], d["plane_data_in_lds"] = n.value, lds.value  # (rt_set_quads: the count, and LDS or L2 for the plane data)
        return d

    def launched_variants(self, reset=False):
        """rt_debug_launched_variants: the kernel instantiations this context has launched since the last reset, in the form of
        variant_tables()."""
        led = _ffi.RtVariantLedger()
        self._call("rt_debug_launched_variants", C.byref(led), 1 if reset else 0)
        return _ledger_sets(led)

    def shard_rows(self, params):
        return self._lib.rt_shard_rows(params.ny, params.shard_band or 1, params.shard_count, params.shard_id)

    def _pinned(self, shape, dtype):
        """A numpy array over rt_host_alloc'ed (page-locked) memory, kept and reused by this Renderer: rt_render writes it
        by asynchronous copies at PCIe rate (what a host replacing main.rs:109-128 would allocate its frame in)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        key = np.dtype(dtype).char
        if not hasattr(self, "_pin"):
            self._pin, self._pin_retired = {}, []
        ptr, size = self._pin.get(key, (None, 0))
        if size < n:
            if ptr:  # arrays handed out earlier are views of it: an outgrown buffer lives until close()
                self._pin_retired.append(ptr)
            ptr = self._lib.rt_host_alloc(max(n, 1))
            if not ptr:
                raise RtError("rt_host_alloc failed")
            self._pin[key] = (ptr, n)
        buf = (C.c_char * max(n, 1)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def render(self, camera, params, want_rgb8=False, pinned=False):
        """Returns (f32 image [rows, nx, 3] (row 0 = bottom), rgb8 or None, RtStats).  pinned=True: the arrays are views of
        this Renderer's page-locked staging buffers: overwritten by the next pinned render, and their memory is FREED by close() —
        copy what must outlive the Renderer."""
        rows = self.shard_rows(params)
        if pinned:
            img = self._pinned((rows, params.nx, 3), np.float32)
            rgb8 = self._pinned((rows, params.nx, 3), np.uint8) if want_rgb8 else None
        else:
            img = np.zeros((rows, params.nx, 3), dtype=np.float32)
            rgb8 = np.zeros((rows, params.nx, 3), dtype=np.uint8) if want_rgb8 else None
        stats = RtStats()
        self._call("rt_render", C.byref(camera), C.byref(params), img.ctypes.data_as(C.POINTER(C.c_float)),
                   rgb8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgb8 else None, C.byref(stats))
        return img, rgb8, stats

    def accum_begin(self, camera, params, first_sample=0):
        """rt_accum_begin: opens the accumulation of this context for the frame of `params` (params.spp: the expected size of one add)
        and clears its sums; the first added sample gets the index first_sample."""
        self._call("rt_accum_begin", C.byref(camera), C.byref(params), int(first_sample))
        self._accum_shape = (self.shard_rows(params), params.nx)

    def accum_add(self, n):
        """rt_accum_add: n more samples per pixel onto the running sums; returns the RtStats of these samples."""
        stats = RtStats()
        self._call("rt_accum_add", int(n), C.byref(stats))
        return stats

    def _accum_outputs(self, want_rgb8, want_sem):
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        img = np.zeros((rows, nx, 3), dtype=np.float32)
        rgb8 = np.zeros((rows, nx, 3), dtype=np.uint8) if want_rgb8 else None
        sem = np.zeros((rows, nx), dtype=np.float32) if want_sem else None
        return img, rgb8, sem, (img.ctypes.data_as(C.POINTER(C.c_float)), rgb8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgb8 else None,
                                sem.ctypes.data_as(C.POINTER(C.c_float)) if want_sem else None)

    def accum_read(self, want_rgb8=False, want_sem=False):
        """rt_accum_read: (f32 image [rows, nx, 3] as render() returns it, rgb8 or None, sem [rows, nx] f32 or None — the standard error
        of each pixel's mean luminance —, RtNoise) of the samples accumulated so far."""
        img, rgb8, sem, ptrs = self._accum_outputs(want_rgb8, want_sem)
        noise = RtNoise()
        self._call("rt_accum_read", *ptrs, C.byref(noise))
        return img, rgb8, sem, noise

    def accum_end(self):
        """rt_accum_end: ends the accumulation (no error when none is open)."""
        self._call("rt_accum_end")

    def render_to_noise(self, camera, params, target, step, want_rgb8=False, want_sem=False):
        """rt_render_to_noise: samples in steps of `step` until RtNoise.noise <= target or params.spp, the maximum, are done.  Returns
        (img, rgb8 or None, sem or None, RtNoise, RtStats summed over the steps); img is render() with spp = RtNoise.spp_done, bit for bit."""
        self._accum_shape = (self.shard_rows(params), params.nx)
        img, rgb8, sem, ptrs = self._accum_outputs(want_rgb8, want_sem)
        noise, stats = RtNoise(), RtStats()
        self._call("rt_render_to_noise", C.byref(camera), C.byref(params), float(target), int(step), *ptrs, C.byref(noise), C.byref(stats))
        return img, rgb8, sem, noise, stats

    def accum_add_adaptive(self, n, tolerance, luminance_floor=0.01, min_samples=16):
        """rt_accum_add_adaptive: pixels that hold min_samples samples and whose mean luminance has a variance of at most
        (tolerance * max(mean, luminance_floor))^2 stop for good; every other pixel gets n more samples.  Returns the RtStats of the rays
        traced (n_paths = active pixels x n)."""
        ad, stats = make_adaptive(tolerance, luminance_floor, min_samples), RtStats()
        self._call("rt_accum_add_adaptive", int(n), C.byref(ad), C.byref(stats))
        return stats

    def accum_counts(self):
        """rt_accum_read_counts: (sample counts [rows, nx] u32 laid out as accum_read's sem, RtAdaptiveInfo)."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        counts, info = np.zeros((rows, nx), dtype=np.uint32), RtAdaptiveInfo()
        self._call("rt_accum_read_counts", counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info))
        return counts, info

    def render_adaptive(self, camera, params, tolerance, step, luminance_floor=0.01, min_samples=16, want_rgb8=False, want_sem=False):
        """rt_render_adaptive: adaptive adds of `step` samples until no pixel is active or params.spp, the maximum, are issued.  Returns
        (img, rgb8 or None, sem or None, counts [rows, nx] u32, RtNoise, RtAdaptiveInfo, RtStats summed over the steps); pixel p of img is
        pixel p of render() with spp = counts[p], bit for bit."""
        self._accum_shape = (self.shard_rows(params), params.nx)
        img, rgb8, sem, ptrs = self._accum_outputs(want_rgb8, want_sem)
        counts = np.zeros(self._accum_shape, dtype=np.uint32)
        ad, noise, info, stats = make_adaptive(tolerance, luminance_floor, min_samples), RtNoise(), RtAdaptiveInfo(), RtStats()
        self._call("rt_render_adaptive", C.byref(camera), C.byref(params), C.byref(ad), int(step), *ptrs,
                   counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(noise), C.byref(info), C.byref(stats))
        return img, rgb8, sem, counts, noise, info, stats

    def debug_accum_set_moments(self, pixel, s1, s2):
        """rt_debug_accum_set_moments: overwrites (S1, S2) of pixel `pixel` (an index into accum_read's sem, flattened) of the open accumulation."""
        self._call("rt_debug_accum_set_moments", int(pixel), float(s1), float(s2))

    @staticmethod
    def _denoise_ptr(radius, patch, strength, default_strength=_ffi.DENOISE_DEFAULT_STRENGTH):
        dn = RtDenoise(int(radius), int(patch), float(default_strength if strength is None else strength), 0)
        return C.byref(dn)

    def _accum_filter(self, name, *lead, dn, want_rgb8):
        """An rt_accum_denoise* call with the arguments (`lead`, RtDenoise, out_rgb_f32, out_rgb8).  Returns (img, rgb8 or None)."""
        img, rgb8, _, ptrs = self._accum_outputs(want_rgb8, False)
        self._call(name, *lead, dn, ptrs[0], ptrs[1])
        return img, rgb8

    def accum_denoise(self, radius=5, patch=1, strength=None, want_rgb8=False):
        """rt_accum_denoise: the frame of the open accumulation through the variance-guided non-local-means filter (window radius, patch
        radius, strength; None: RT_DENOISE_DEFAULT_STRENGTH).  Returns (img [rows, nx, 3] f32, rgb8 or None) laid out as accum_read's; the
        accumulation itself is not changed."""
        return self._accum_filter("rt_accum_denoise", dn=self._denoise_ptr(radius, patch, strength), want_rgb8=want_rgb8)

    def debug_denoise(self, rgb, y, v, radius=5, patch=1, strength=None):
        """rt_debug_denoise: the filter kernel of accum_denoise over host arrays in image order — rgb [rows, nx, 3], y and v [rows, nx]
        (a pixel's mean luminance and the variance of that mean); returns the filtered [rows, nx, 3] f32 image."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        y, v = np.ascontiguousarray(y, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)
        rows, nx = y.shape
        assert rgb.shape == (rows, nx, 3) and v.shape == (rows, nx)
        out = np.zeros_like(rgb)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        self._call("rt_debug_denoise", nx, rows, fp(rgb), fp(y), fp(v), self._denoise_ptr(radius, patch, strength), fp(out))
        return out

    def accum_track_channels(self):
        """rt_accum_track_channels: the open accumulation also keeps two f64 moments per pixel and channel (48 B per pixel); right after
        accum_begin, before the first add.  Everything else the accumulation returns stays bit for bit."""
        self._call("rt_accum_track_channels")

    def accum_channel_sem(self):
        """rt_accum_read_channel_sem: [rows, nx, 3] f32, the standard error of each pixel's mean per channel, laid out as accum_read's image."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        sem = np.zeros((rows, nx, 3), dtype=np.float32)
        self._call("rt_accum_read_channel_sem", sem.ctypes.data_as(C.POINTER(C.c_float)))
        return sem

    def accum_denoise_channels(self, radius=5, patch=1, strength=None, want_rgb8=False):
        """rt_accum_denoise_channels: accum_denoise with the distance on the three channels and their own variances, so that edges between
        colours of equal luminance stay; the accumulation must track channels (accum_track_channels).  Returns (img, rgb8 or None)."""
        return self._accum_filter("rt_accum_denoise_channels", dn=self._denoise_ptr(radius, patch, strength), want_rgb8=want_rgb8)

    def debug_denoise_channels(self, rgb, var_rgb, radius=5, patch=1, strength=None):
        """rt_debug_denoise_channels: the filter kernel of accum_denoise_channels over host arrays in image order — rgb and var_rgb
        [rows, nx, 3] (a pixel's channel means and the variances of those means); returns the filtered [rows, nx, 3] f32 image."""
        rgb, var_rgb = np.ascontiguousarray(rgb, dtype=np.float32), np.ascontiguousarray(var_rgb, dtype=np.float32)
        rows, nx, _ = rgb.shape
        assert rgb.shape == (rows, nx, 3) == var_rgb.shape
        out = np.zeros_like(rgb)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        self._call("rt_debug_denoise_channels", nx, rows, fp(rgb), fp(var_rgb), self._denoise_ptr(radius, patch, strength), fp(out))
        return out

    _GUIDES = {"luminance": _ffi.DENOISE_GUIDE_LUMINANCE, "channels": _ffi.DENOISE_GUIDE_CHANNELS}

    def accum_denoise_multiscale(self, levels=None, guide="luminance", radius=5, patch=1, strength=None, want_rgb8=False):
        """rt_accum_denoise_multiscale: accum_denoise (guide "luminance") or accum_denoise_channels (guide "channels") on a 2x pyramid of
        `levels` levels (1 .. DENOISE_MAX_LEVELS; None: RT_DENOISE_DEFAULT_LEVELS), each coarser level replacing the low frequencies of
        the finer one; levels=1 is the single-scale filter bit for bit.  Returns (img [rows, nx, 3] f32, rgb8 or None)."""
        ms = _ffi.RtMultiscale(_ffi.DENOISE_DEFAULT_LEVELS if levels is None else int(levels), self._GUIDES[guide] if isinstance(guide, str) else int(guide))
        img, rgb8, _, ptrs = self._accum_outputs(want_rgb8, False)
        self._call("rt_accum_denoise_multiscale", self._denoise_ptr(radius, patch, strength), C.byref(ms), ptrs[0], ptrs[1])
        return img, rgb8

    def debug_denoise_multiscale(self, rgb, mean, var, levels, guide="luminance", radius=5, patch=1, strength=None, probe_level=None):
        """rt_debug_denoise_multiscale: the kernels of accum_denoise_multiscale over host arrays in image order.  guide "luminance": rgb
        [rows, nx, 3], mean and var [rows, nx] as debug_denoise takes them; guide "channels": rgb and var [rows, nx, 3] as
        debug_denoise_channels takes them, `mean` is not read (None).  Returns the filtered [rows, nx, 3] f32 image, or with probe_level
        (img, (c, mean, var)): the filter's inputs of that level, shaped as the arguments are at the level's size."""
        g = self._GUIDES[guide] if isinstance(guide, str) else int(guide)
        channels = g == _ffi.DENOISE_GUIDE_CHANNELS
        rgb, var = np.ascontiguousarray(rgb, dtype=np.float32), np.ascontiguousarray(var, dtype=np.float32)
        rows, nx, _ = rgb.shape
        assert var.shape == ((rows, nx, 3) if channels else (rows, nx))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
        if not channels:
            mean = np.ascontiguousarray(mean, dtype=np.float32)
            assert mean.shape == (rows, nx)
        out = np.zeros_like(rgb)
        probes = [None, None, None]
        if probe_level is not None:
            nx_l, rows_l = denoise_level_size(nx, rows, probe_level)
            tail = (3,) if channels else ()
            probes = [np.zeros((rows_l, nx_l, 3), np.float32), np.zeros((rows_l, nx_l) + tail, np.float32), np.zeros((rows_l, nx_l) + tail, np.float32)]
        self._call("rt_debug_denoise_multiscale", nx, rows, g, fp(rgb), None if channels else fp(mean), fp(var), self._denoise_ptr(radius, patch, strength),
                   int(levels), fp(out), int(probe_level or 0), *[fp(a) for a in probes])
        return out if probe_level is None else (out, tuple(probes))

    def accum_export(self):
        """rt_accum_export: the open accumulation as an AccumState — every plane it holds; on a uniform accumulation counts and converged
        are `done` and 0.  The accumulation is read and not changed."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        probe = _ffi.RtAccumState()
        self._call("rt_accum_export", C.byref(probe))  # the scalar fields only: which planes are there to ask for
        channels = bool(probe.planes & _ffi.ACCUM_STATE_CHANNELS)
        state = AccumState(probe.nx, probe.rows, sum=np.zeros((rows, nx, 3), np.float32), moments=np.zeros((rows, nx, 2), np.float64),
                           counts=np.zeros((rows, nx), np.uint32), converged=np.zeros((rows, nx), np.uint8),
                           channel_moments=np.zeros((rows, nx, 6), np.float64) if channels else None)
        state.planes = _ffi.ACCUM_STATE_COUNTS | (_ffi.ACCUM_STATE_CHANNELS if channels else 0)  # (every array below gets a pointer)
        st = state.as_struct()
        self._call("rt_accum_export", C.byref(st))
        state.first_sample, state.done, state.planes, state.frame_id = st.first_sample, st.done, st.planes, st.frame_id
        return state

    def accum_import(self, state):
        """rt_accum_import: puts an AccumState into the accumulation just begun (before its first add); it then goes on, bit for bit, as
        the exported one would have."""
        st = state.as_struct()
        self._call("rt_accum_import", C.byref(st))

    def accum_merge(self, state):
        """rt_accum_merge: adds the AccumState of the sample window that follows the open accumulation's onto it (both uniform)."""
        st = state.as_struct()
        self._call("rt_accum_merge", C.byref(st))

    def accum_track_halves(self):
        """rt_accum_track_halves: the open accumulation also keeps the even and the odd samples of every pixel apart (56 B per pixel); right
        after accum_begin, before the first add.  Everything else the accumulation returns stays bit for bit."""
        self._call("rt_accum_track_halves")

    def accum_half(self, h, want_sem=False):
        """rt_accum_read_halves: (img [rows, nx, 3] f32 of half h — 0: the samples with an even absolute index —, sem [rows, nx] f32 or None),
        laid out as accum_read's."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        img = np.zeros((rows, nx, 3), dtype=np.float32)
        sem = np.zeros((rows, nx), dtype=np.float32) if want_sem else None
        self._call("rt_accum_read_halves", int(h), img.ctypes.data_as(C.POINTER(C.c_float)), sem.ctypes.data_as(C.POINTER(C.c_float)) if want_sem else None)
        return img, sem

    def accum_denoise_halves(self, radius=5, patch=1, strength=None, want_rgb8=False, want_err=False):
        """rt_accum_denoise_halves: each half filtered with the weights of the other, the two combined; the accumulation must track halves.
        Returns (img [rows, nx, 3] f32, rgb8 or None, err [rows, nx] f32 or None — the per-pixel residual variance e_p —, RtResidual).
        RtResidual.residual_rms is the variance half of the filtered frame's error: a lower bound, blur is not in it.  strength None:
        RT_DENOISE_HALVES_DEFAULT_STRENGTH."""
        img, rgb8, err, ptrs = self._accum_outputs(want_rgb8, want_err)
        res = RtResidual()
        self._call("rt_accum_denoise_halves", self._denoise_ptr(radius, patch, strength, _ffi.DENOISE_HALVES_DEFAULT_STRENGTH), *ptrs, C.byref(res))
        return img, rgb8, err, res

    def accum_denoise_select(self, select=None, want_rgb8=False):
        """rt_accum_denoise_select: the cross filter of accum_denoise_halves at every candidate strength of `select` (make_select; None: the
        defaults), the luminance error of each estimated per pixel against the other half, the smallest chosen and the candidates blended;
        the accumulation must track halves.  Returns (img [rows, nx, 3] f32, rgb8 or None, index [rows, nx] u8 — the candidate each pixel
        chose —, est [rows, nx] f32 — the estimated squared luminance error of a half filter there —, RtSelectInfo).  RtSelectInfo.best is
        the frame-wide choice: select.strength[best] is what to hand to accum_denoise_halves."""
        img, rgb8, est, ptrs = self._accum_outputs(want_rgb8, True)
        index = np.zeros(est.shape, dtype=np.uint8)
        info = RtSelectInfo()
        self._call("rt_accum_denoise_select", C.byref(select) if select is not None else None, ptrs[0], ptrs[1], index.ctypes.data_as(C.POINTER(C.c_uint8)), ptrs[2],
                   C.byref(info))
        return img, rgb8, index, est, info

    def debug_denoise_select(self, c, yv, select=None, first_sample=0, n=16, counts=None, probe=None):
        """rt_debug_denoise_select: the kernels of accum_denoise_select over host arrays in image order — c = (c_0, c_1), [rows, nx, 3] each;
        yv = ((y_0, v_0), (y_1, v_1)), [rows, nx] each; the halves hold the samples [first_sample, first_sample + n), with n = counts[p]
        per pixel where counts [rows, nx] u32 is given.  Returns (img, index, est, RtSelectInfo), and with probe = j also (out_j, E_j)."""
        c = [np.ascontiguousarray(x, dtype=np.float32) for x in c]
        rows, nx, _ = c[0].shape
        g = [np.ascontiguousarray(np.stack([np.asarray(y, np.float32), np.asarray(v, np.float32)], -1)) for y, v in yv]
        assert c[1].shape == (rows, nx, 3) and all(x.shape == (rows, nx, 2) for x in g)
        cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        assert cnt is None or cnt.shape == (rows, nx)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
        out, est, index = np.zeros((rows, nx, 3), np.float32), np.zeros((rows, nx), np.float32), np.zeros((rows, nx), np.uint8)
        p_out = np.zeros((rows, nx, 3), np.float32) if probe is not None else None
        p_err = np.zeros((rows, nx), np.float32) if probe is not None else None
        info = RtSelectInfo()
        self._call("rt_debug_denoise_select", nx, rows, fp(c[0]), fp(c[1]), fp(g[0]), fp(g[1]), cnt.ctypes.data_as(C.POINTER(C.c_uint32)) if cnt is not None else None,
                   int(first_sample), int(n), C.byref(select) if select is not None else None, fp(out), index.ctypes.data_as(C.POINTER(C.c_uint8)), fp(est),
                   C.byref(info), int(probe or 0), fp(p_out), fp(p_err))
        return (out, index, est, info) if probe is None else (out, index, est, info, p_out, p_err)

    def debug_select_chain(self, chain):
        """rt_debug_select_chain: which filter chain accum_denoise_select and debug_denoise_select run on this Renderer — "auto", "plain"
        (2 K launches of the filter) or "fused" (one launch per half for all K strengths), or the _ffi.SELECT_CHAIN_* number.  Every chain
        gives the same bits."""
        names = {"auto": _ffi.SELECT_CHAIN_AUTO, "plain": _ffi.SELECT_CHAIN_PLAIN, "fused": _ffi.SELECT_CHAIN_FUSED}
        self._call("rt_debug_select_chain", names[chain] if isinstance(chain, str) else int(chain))

    def accum_export_halves(self):
        """rt_accum_export_halves: the half buffers of the open accumulation as an AccumHalves.  Read, not changed."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        halves = AccumHalves(nx, rows)
        hs = halves.as_struct()
        self._call("rt_accum_export_halves", C.byref(hs))
        halves.first_sample, halves.done, halves.frame_id = hs.first_sample, hs.done, hs.frame_id
        return halves

    def accum_import_halves(self, halves):
        """rt_accum_import_halves: puts an AccumHalves into the accumulation just begun — fresh, or right after accum_import of the state it
        belongs to — and turns tracking on."""
        hs = halves.as_struct()
        self._call("rt_accum_import_halves", C.byref(hs))

    def accum_track_filter(self, flt):
        """rt_accum_track_filter: the open accumulation also keeps, per pixel, the samples of the pixel and of its neighbours weighted by the
        reconstruction filter `flt` (make_pixel_filter; 16 B per pixel); right after accum_begin, before the first add.  Everything else the
        accumulation returns stays bit for bit.  Not on a sharded accumulation."""
        self._call("rt_accum_track_filter", C.byref(flt) if flt is not None else None)

    def accum_filtered(self, want_rgb8=False, want_weight=False):
        """rt_accum_read_filtered: (img [rows, nx, 3] f32 = sum w rgb / sum w — the box mean of accum_read where the weight sum is not
        positive —, rgb8 or None, made as the denoisers' is, weight [rows, nx] f32 = sum w or None)."""
        img, rgb8, w, ptrs = self._accum_outputs(want_rgb8, want_weight)
        self._call("rt_accum_read_filtered", *ptrs)
        return img, rgb8, w

    def accum_export_filter(self):
        """rt_accum_export_filter: the filter and its plane of the open accumulation as an AccumFilter.  Read, not changed."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        snap = AccumFilter(nx, rows)
        fs = snap.as_struct()
        self._call("rt_accum_export_filter", C.byref(fs))
        return AccumFilter(nx, rows, fs.first_sample, fs.done, fs.frame_id, plane=snap.plane, filter=fs.filter)

    def accum_import_filter(self, snap):
        """rt_accum_import_filter: puts an AccumFilter into the accumulation just begun — fresh, or right after accum_import of the state it
        belongs to — and turns tracking on under its filter."""
        fs = snap.as_struct()
        self._call("rt_accum_import_filter", C.byref(fs))

    def debug_filter_add(self, i0, rad):
        """rt_debug_filter_add: the production resolve kernel over rad [n, rows, nx, 3] f32 — designed radiance in image order, as the samples
        with the absolute indices i0 .. i0 + n - 1 — onto the filter plane of the open accumulation only."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        rad = np.ascontiguousarray(rad, dtype=np.float32)
        assert rad.ndim == 4 and rad.shape[1:] == (rows, nx, 3), rad.shape
        self._call("rt_debug_filter_add", int(i0), rad.shape[0], rad.ctypes.data_as(C.POINTER(C.c_float)))

    def accum_track_features(self, stride=1):
        """rt_accum_track_features: the open accumulation also keeps, per pixel, the albedo, normal and depth of the first hit of every
        stride-th sample (by absolute index) with their second moments (64 B per pixel); right after accum_begin, before the first add.
        A kernel of its own recomputes the first hits; everything else the accumulation returns stays bit for bit.  Not on a sharded
        accumulation."""
        self._call("rt_accum_track_features", C.byref(_ffi.RtFeatures(int(stride), 0)))

    def accum_features(self):
        """rt_accum_read_features: a dict of f32 arrays in image order — albedo [rows, nx, 3], normal [rows, nx, 3], depth [rows, nx],
        hit [rows, nx] (the fraction of feature samples that hit) and var [rows, nx, 3] (the variance of the mean of albedo, normal,
        depth)."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        out = {"albedo": np.zeros((rows, nx, 3), np.float32), "normal": np.zeros((rows, nx, 3), np.float32), "depth": np.zeros((rows, nx), np.float32),
               "hit": np.zeros((rows, nx), np.float32), "var": np.zeros((rows, nx, 3), np.float32)}
        self._call("rt_accum_read_features", *(out[k].ctypes.data_as(C.POINTER(C.c_float)) for k in ("albedo", "normal", "depth", "hit", "var")))
        return out

    def accum_export_features(self):
        """rt_accum_export_features: the stride and the records of the open accumulation as an AccumFeatures.  Read, not changed."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        snap = AccumFeatures(nx, rows)
        fs = snap.as_struct()
        self._call("rt_accum_export_features", C.byref(fs))
        return AccumFeatures(nx, rows, fs.first_sample, fs.done, fs.frame_id, fs.features.stride, plane=snap.plane)

    def accum_import_features(self, snap):
        """rt_accum_import_features: puts an AccumFeatures into the accumulation just begun — fresh, or right after accum_import of the state
        it belongs to — and turns tracking on under its stride."""
        fs = snap.as_struct()
        self._call("rt_accum_import_features", C.byref(fs))

    def accum_denoise_features(self, guide, radius=5, patch=1, strength=None, want_rgb8=False):
        """rt_accum_denoise_features: accum_denoise with the first-hit features of the accumulation beside the colour guide (`guide`:
        make_feature_guide).  Returns (img [rows, nx, 3] f32, rgb8 or None) laid out as accum_read's; the accumulation is not changed."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        img = np.zeros((rows, nx, 3), dtype=np.float32)
        rgb8 = np.zeros((rows, nx, 3), dtype=np.uint8) if want_rgb8 else None
        self._call("rt_accum_denoise_features", self._denoise_ptr(radius, patch, strength), C.byref(guide) if guide is not None else None,
                   img.ctypes.data_as(C.POINTER(C.c_float)), rgb8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgb8 else None)
        return img, rgb8

    def debug_denoise_features(self, rgb, y, v, feat_mean, feat_var, guide, radius=5, patch=1, strength=None):
        """rt_debug_denoise_features: the kernels of accum_denoise_features over host arrays in image order — rgb [rows, nx, 3], y and v
        [rows, nx], feat_mean [rows, nx, 7] (albedo 3, normal 3, depth) and feat_var [rows, nx, 3]; returns the filtered [rows, nx, 3]."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        y, v = np.ascontiguousarray(y, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)
        fm, fv = np.ascontiguousarray(feat_mean, dtype=np.float32), np.ascontiguousarray(feat_var, dtype=np.float32)
        rows, nx = y.shape
        assert rgb.shape == (rows, nx, 3) and v.shape == (rows, nx) and fm.shape == (rows, nx, 7) and fv.shape == (rows, nx, 3)
        out = np.zeros_like(rgb)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        self._call("rt_debug_denoise_features", nx, rows, fp(rgb), fp(y), fp(v), fp(fm), fp(fv), self._denoise_ptr(radius, patch, strength),
                   C.byref(guide) if guide is not None else None, fp(out))
        return out

    def debug_features_add(self, i0, n_samples):
        """rt_debug_features_add: the production kernel k_features over the samples i0 .. i0 + n_samples - 1 of every pixel, onto the
        feature records of the open accumulation only; nothing is traced."""
        self._call("rt_debug_features_add", int(i0), int(n_samples))

    def accum_track_buckets(self, M):
        """rt_accum_track_buckets: the open accumulation also keeps the samples of every pixel in M buckets by sample index (12 M bytes per
        pixel, 3 <= M <= 16); right after accum_begin, before the first add.  Everything else the accumulation returns stays bit for bit."""
        self._call("rt_accum_track_buckets", int(M))

    @staticmethod
    def _robust(mode, trim):
        modes = {"gini": _ffi.ROBUST_GINI, "median": _ffi.ROBUST_MEDIAN, "trim": _ffi.ROBUST_TRIM}
        if isinstance(mode, str) and mode not in modes:
            raise ValueError(f"robust mode {mode!r}: expected one of {sorted(modes)} (or an RT_ROBUST_* value)")
        return _ffi.RtRobust(modes[mode] if isinstance(mode, str) else int(mode), int(trim))

    def accum_robust(self, mode="gini", trim=0, want_trim=False, want_rgb8=False):
        """rt_accum_read_robust: the frame as the trimmed mean of its sorted bucket means — mode "gini" (the trim follows the Gini
        coefficient of the means), "median", or "trim" with `trim` means dropped per side.  Returns (img [rows, nx, 3] f32, RtRobustInfo
        [, trim [rows, nx, 3] u8][, rgb8]).  The estimator is biased: RtRobustInfo.energy_removed is the share of luminance it took away."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        img = np.zeros((rows, nx, 3), dtype=np.float32)
        t = np.zeros((rows, nx, 3), dtype=np.uint8) if want_trim else None
        rgb8 = np.zeros((rows, nx, 3), dtype=np.uint8) if want_rgb8 else None
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None
        rb, info = self._robust(mode, trim), _ffi.RtRobustInfo()
        self._call("rt_accum_read_robust", C.byref(rb), img.ctypes.data_as(C.POINTER(C.c_float)), u8(rgb8), u8(t), C.byref(info))
        return (img, info) + ((t,) if want_trim else ()) + ((rgb8,) if want_rgb8 else ())

    def accum_denoise_robust(self, mode="gini", trim=0, radius=5, patch=1, strength=None, want_rgb8=False):
        """rt_accum_denoise_robust: accum_denoise with the colours replaced by the robust read-out; the guide stays the luminance moments'.
        Returns (img [rows, nx, 3] f32, rgb8 or None)."""
        rb = self._robust(mode, trim)
        return self._accum_filter("rt_accum_denoise_robust", C.byref(rb), dn=self._denoise_ptr(radius, patch, strength), want_rgb8=want_rgb8)

    def accum_export_buckets(self):
        """rt_accum_export_buckets: the sample buckets of the open accumulation as an AccumBuckets.  Read, not changed."""
        rows, nx = getattr(self, "_accum_shape", (0, 0))
        probe = _ffi.RtAccumBuckets()
        self._call("rt_accum_export_buckets", C.byref(probe))  # the scalar fields only: M
        buckets = AccumBuckets(nx, rows, probe.M)
        bs = buckets.as_struct()
        self._call("rt_accum_export_buckets", C.byref(bs))
        buckets.first_sample, buckets.done, buckets.frame_id = bs.first_sample, bs.done, bs.frame_id
        return buckets

    def accum_import_buckets(self, buckets):
        """rt_accum_import_buckets: puts an AccumBuckets into the accumulation just begun — fresh, or right after accum_import (and
        accum_import_halves) of the state it belongs to — and turns tracking on."""
        bs = buckets.as_struct()
        self._call("rt_accum_import_buckets", C.byref(bs))

    def render_to_residual(self, camera, params, target, step, radius=5, patch=1, strength=None, want_rgb8=False, want_err=False):
        """Renders until the DENOISED frame is clean: an accumulation that tracks halves gets adds of `step` samples (the first one at least
        4) until RtResidual.residual_noise <= target or params.spp, the maximum, are issued; one cross filter per step, a host loop.
        Returns what accum_denoise_halves returns plus the samples per pixel done.  residual_noise is a lower bound of the filtered
        frame's relative error (its variance half), so the target bounds the noise that is left, not the blur."""
        if step <= 0 or not target >= 0.0 or params.spp < 4:
            raise ValueError("render_to_residual: step must be > 0, target >= 0 and params.spp, the maximum, >= 4")
        p = RtParams.from_buffer_copy(params)
        p.spp = min(max(int(step), 4), params.spp)
        self.accum_begin(camera, p, 0)
        try:
            self.accum_track_halves()
            done = 0
            while True:
                n = min(max(int(step), 4 - done), params.spp - done)
                self.accum_add(n)
                done += n
                out = self.accum_denoise_halves(radius, patch, strength, want_rgb8, want_err)
                if done >= params.spp or out[3].residual_noise <= target or out[0].size == 0:
                    return out + (done,)
        finally:
            self.accum_end()

    def set_display(self, display):
        """rt_set_display: every rgb8 of accum_read, the accum_denoise* calls and accum_robust becomes the display transform (make_display)
        of the f32 image the same call returns; None: the reference quantisation again.  Does not end an open accumulation; upload()
        keeps it.  render() and the progress preview are not covered."""
        self._call("rt_set_display", C.byref(display) if display is not None else None)

    def display_info(self):
        """rt_display_info: the RtDisplayInfo (exposure applied, L_q or the log average, lit / non-finite pixels, saturated values) of the
        last rgb8 this Renderer wrote under a display."""
        info = RtDisplayInfo()
        self._call("rt_display_info", C.byref(info))
        return info

    def debug_display(self, rgb, display):
        """rt_debug_display: the display kernels over a host image [rows, nx, 3] f32 in the row order of accum_read's img; returns
        (rgb8 [rows, nx, 3] with row 0 on top, RtDisplayInfo).  Neither reads nor changes the display set on this Renderer."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        rows, nx = rgb.shape[:2]
        assert rgb.shape == (rows, nx, 3)
        out, info = np.zeros((rows, nx, 3), np.uint8), RtDisplayInfo()
        self._call("rt_debug_display", nx, rows, rgb.ctypes.data_as(C.POINTER(C.c_float)), C.byref(display), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                   C.byref(info))
        return out, info

    def set_glare(self, glare):
        """rt_set_glare: every rgb8 of accum_read, the accum_denoise* calls and accum_robust is made from the glared image (make_glare) of
        the f32 image the same call returns — through the display where one is set, else through the reference quantisation; None: no
        glare.  Does not end an open accumulation; upload() keeps it.  render() and the progress preview are not covered."""
        self._call("rt_set_glare", C.byref(glare) if glare is not None else None)

    def glare_info(self):
        """rt_glare_info: the RtGlareInfo (effective levels, size of the coarsest level) of the last rgb8 written under a glare."""
        info = RtGlareInfo()
        self._call("rt_glare_info", C.byref(info))
        return info

    def glare_image(self, nx, rows):
        """rt_glare_image: the glared linear image [rows, nx, 3] f32 (row 0 at the bottom, as accum_read's img) behind the last rgb8
        written under a glare; nx and rows are that call's."""
        out = np.zeros((rows, nx, 3), np.float32)
        self._call("rt_glare_image", out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def debug_glare(self, rgb, glare, display=None, want_rgb8=True):
        """rt_debug_glare: the glare kernels over a host image [rows, nx, 3] f32 in the row order of accum_read's img, then `display` (None:
        the reference quantisation); returns (out [rows, nx, 3] f32, rgb8 [rows, nx, 3] with row 0 on top or None, RtGlareInfo).  Neither
        reads nor changes the glare and the display set on this Renderer."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        rows, nx = rgb.shape[:2]
        assert rgb.shape == (rows, nx, 3)
        out, info = np.zeros((rows, nx, 3), np.float32), RtGlareInfo()
        u8 = np.zeros((rows, nx, 3), np.uint8) if want_rgb8 else None
        self._call("rt_debug_glare", nx, rows, rgb.ctypes.data_as(C.POINTER(C.c_float)), C.byref(glare), C.byref(display) if display is not None else None,
                   out.ctypes.data_as(C.POINTER(C.c_float)), u8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgb8 else None, C.byref(info))
        return out, u8, info

    def debug_glare_chain(self, chain):
        """rt_debug_glare_chain: "auto" | "plain" | "fused" (or the _ffi number): which down chain the glare of this Renderer runs; the
        same bits either way."""
        table = {"auto": _ffi.GLARE_CHAIN_AUTO, "plain": _ffi.GLARE_CHAIN_PLAIN, "fused": _ffi.GLARE_CHAIN_FUSED}
        self._call("rt_debug_glare_chain", table[chain] if isinstance(chain, str) else int(chain))

    def set_progress(self, fn):
        """fn(spp_done, spp_total, rgb8[rows, nx, 3]) after every slice but the last of a following render()
        (main.rs:114-123, the partial saves); None removes it.  Pick the cadence with make_params(spp_slice=...)."""
        if fn is None:
            self._progress = None
            rc = self._lib.rt_set_progress(self._ctx, _ffi.RtProgressFn(), None)
        else:
            def tramp(_user, done, total, ptr, nx, rows):
                fn(done, total, np.ctypeslib.as_array(ptr, shape=(rows, nx, 3)).copy())
            self._progress = _ffi.RtProgressFn(tramp)  # keep the thunk alive as long as it is registered
            rc = self._lib.rt_set_progress(self._ctx, self._progress, None)
        if rc != 0:
            self._raise("rt_set_progress", rc)

    def set_lens(self, lens):
        """rt_set_lens: the thin lens of the following renders — an RtLens, a (lens_radius, focus_dist) pair or Scene.lens;
        lens_radius = aperture / 2 of the book's Camera::new.  None or lens_radius 0: the pinhole.  Per context, and like the
        camera it is passed, not taken from the uploaded scene."""
        self._call("rt_set_lens", _lens_ptr(lens))

    def set_motion(self, motion):
        """rt_set_motion: the moving spheres of the following renders — Scene.motion, make_motion(..) or a (spheres, center1[, shutter])
        tuple; None: the static renderer.  After upload(); upload() clears it."""
        if motion is not None and not isinstance(motion, RtMotion):
            motion = make_motion(*motion)
        self._call("rt_set_motion", _motion_ptr(motion))
        self._n_moving = motion.n_moving if motion is not None else 0  # (motion_bounds sizes its cell table by it)

    def set_quads(self, quads):
        """rt_set_quads: the planar primitives (quads, triangles) of the following renders — Scene.quads, make_quads(..) or a
        (q, u, v, kind, mat) tuple; None: none.  After upload(); upload() clears them.  Not together with set_motion."""
        self._call("rt_set_quads", _quads_ptr(quads))

    def set_lights(self, lights):
        """rt_set_lights: light importance sampling for the following renders — Scene.lights, make_lights(..) or a (q, u, v) tuple of
        world-space parallelograms; None: none.  After upload(); upload() clears it.  The lights are sampling targets only: any set gives
        the same mean, the one that covers the emitters gives less noise.  Not together with set_motion."""
        self._call("rt_set_lights", _lights_ptr(lights))

    def motion_bounds(self):
        """rt_debug_motion_bounds as a dict: the bounds set_motion built (padded entry boxes, candidate-list spheres, entry ids, the
        grid and the cells that list each moving sphere; a cell list [0xFFFFFFFF] = tested for every ray)."""
        n, nc = C.c_uint32(0), C.c_uint32(0)
        grid, dims = (C.c_float * 6)(), (C.c_uint32 * 3)()
        # the sizing call: RT_ERR_INVALID ("a buffer is missing", the counts are filled in) is its expected answer
        rc = self._lib.rt_debug_motion_bounds(self._ctx, None, None, None, 0, C.byref(n), grid, dims, None, None, 0, C.byref(nc))
        if rc not in (0, -1):
            self._raise("rt_debug_motion_bounds", rc)
        boxes = np.zeros((n.value, 6), np.float32)
        bs = np.zeros((n.value, 4), np.float32)
        ids = np.zeros(n.value, np.uint32)
        cells = np.zeros(max(nc.value, 1), np.uint32)
        begin = np.zeros(getattr(self, "_n_moving", 0) + 1, np.uint32)  # the call writes n_moving + 1 entries
        self._call("rt_debug_motion_bounds", boxes.ctypes.data, bs.ctypes.data, ids.ctypes.data, n.value, C.byref(n), grid, dims,
                   begin.ctypes.data, cells.ctypes.data, cells.size, C.byref(nc))
        return {"entry_box_padded": boxes, "entry_sphere": bs, "entry_id": ids, "grid_min": np.array(grid[0:3], np.float32),
                "grid_cell": np.array(grid[3:6], np.float32), "grid_dims": tuple(dims), "cell_begin": begin, "cell_id": cells[:nc.value]}

    def render_device(self, camera, params, device_ptr, stream=None, want_stats=True):
        """Renders into HBM at `device_ptr` (e.g. torch_tensor.data_ptr()); nothing crosses PCIe."""
        stats = RtStats()
        self._call("rt_render_device", C.byref(camera), C.byref(params), C.c_void_p(device_ptr), C.c_void_p(stream) if stream else None,
                   C.byref(stats) if want_stats else None)
        return stats

    def render_parts(self):
        """rt_debug_render_parts: host-side timeline of the last render as {label: ms} in call order (allocations one by one, the
        hardware-queue probe = first kernel launch, candidate lists + the in-frame synchronisation, enqueue, wait), plus counters:
        "primary_lists_overflow" = pixels whose candidate list overflowed (-1: no lists, or a general scene)."""
        import json
        buf = C.create_string_buffer(4096)
        n = self._lib.rt_debug_render_parts(self._ctx, buf, len(buf))
        if n < 0:
            self._raise("rt_debug_render_parts", n)
        return json.loads(buf.value.decode())

    def depth_timings(self, max_n=128):
        """(isect_ms, shade_ms, rays) per depth of the first slice of the last render with FLAG_TIME_DEPTHS."""
        a = np.zeros(max_n, np.float32)
        b = np.zeros(max_n, np.float32)
        r = np.zeros(max_n, np.uint64)
        n = self._lib.rt_get_depth_timings(self._ctx, max_n, a.ctypes.data_as(C.POINTER(C.c_float)),
                                           b.ctypes.data_as(C.POINTER(C.c_float)), r.ctypes.data_as(C.POINTER(C.c_uint64)))
        if n < 0:
            self._raise("rt_get_depth_timings", n)
        return a[:n], b[:n], r[:n]

    def debug_bounce(self, origins, dirs, keys, depth=0, flags=0):
        """One closest-hit + shade step for caller-given rays (rt_debug_bounce)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
        n = o.shape[0]
        out = {"hit": np.zeros(n, np.int32), "t": np.zeros(n, np.float32), "radiance": np.zeros((n, 3), np.float32),
               "attenuation": np.zeros((n, 3), np.float32), "o": np.zeros((n, 3), np.float32),
               "d": np.zeros((n, 3), np.float32), "alive": np.zeros(n, np.uint8)}
        io = RtBounceIO()
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        io.n, io.depth, io.flags = n, depth, flags
        io.in_o, io.in_d, io.in_key = fp(o), fp(d), k.ctypes.data_as(C.POINTER(C.c_uint32))
        io.out_hit = out["hit"].ctypes.data_as(C.POINTER(C.c_int32))
        io.out_t, io.out_radiance, io.out_attenuation = fp(out["t"]), fp(out["radiance"]), fp(out["attenuation"])
        io.out_o, io.out_d = fp(out["o"]), fp(out["d"])
        io.out_alive = out["alive"].ctypes.data_as(C.POINTER(C.c_uint8))
        self._call("rt_debug_bounce", C.byref(io))
        return out

    def debug_shared_division(self, x, a):
        """x / a element by element through the kernels' shared-reciprocal division (rt_debug_arithmetic)."""
        return self._debug_arithmetic(0, x, a)

    def debug_sqrt(self, x):
        """sqrt(x) element by element as the kernels take it of discriminants and squared lengths (rt_debug_arithmetic)."""
        return self._debug_arithmetic(1, x, None)

    def debug_to_i32(self, x):
        """`x as i32` (Rust: toward zero, saturating, NaN -> 0) as the kernels convert (rt_debug_arithmetic)."""
        return self._debug_arithmetic(2, x, None).view(np.int32)

    def debug_to_u32(self, x):
        """`x as u32` as the kernels convert (rt_debug_arithmetic)."""
        return self._debug_arithmetic(3, x, None).view(np.uint32)

    def debug_acos(self, x):
        """acosf(x) element by element as Sphere::get_uv calls it (rt_debug_arithmetic)."""
        return self._debug_arithmetic(4, x, None)

    def debug_atan2(self, y, x):
        """atan2f(y, x) element by element as Sphere::get_uv calls it (rt_debug_arithmetic)."""
        return self._debug_arithmetic(5, y, x)

    def debug_sin(self, x):
        """sinf(x) element by element as the checker and Perlin textures and world_to_local_with_rot call it (rt_debug_arithmetic)."""
        return self._debug_arithmetic(6, x, None)

    def debug_cos(self, x):
        """cosf(x) element by element as world_to_local_with_rot calls it (rt_debug_arithmetic)."""
        return self._debug_arithmetic(7, x, None)

    def debug_log(self, x):
        """logf(x) element by element as gtr1 and the media's free path call it (rt_debug_arithmetic)."""
        return self._debug_arithmetic(8, x, None)

    def _debug_arithmetic(self, op, x, a):
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        a = x if a is None else np.ascontiguousarray(a, dtype=np.float32).ravel()
        assert x.shape == a.shape
        out = np.zeros_like(x)
        fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
        self._call("rt_debug_arithmetic", op, len(x), fp(x), fp(a), fp(out))
        return out

    def deinterleave_bands(self, d_gathered, nx, ny, band, n_shards, d_out_f32=None, d_out_u8=None, stream=None):
        """rt_deinterleave_bands on device pointers (ints): gathered band buffers -> frame in image row order."""
        self._call("rt_deinterleave_bands", C.c_void_p(d_gathered), nx, ny, band, n_shards, C.c_void_p(d_out_f32) if d_out_f32 else None,
                   C.c_void_p(d_out_u8) if d_out_u8 else None, C.c_void_p(stream) if stream else None)

    @classmethod
    def _borrowed(cls, lib, ctx, device, accum_shape):
        """A Renderer over a context somebody else owns (MultiRenderer.accum_join): close() leaves the context alone."""
        r = cls.__new__(cls)
        r._lib, r._ctx, r.device, r._owned, r._accum_shape = lib, C.c_void_p(ctx), device, False, accum_shape
        return r

    def close(self):
        if self._ctx:
            if getattr(self, "_owned", True):
                self._lib.rt_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()
        for ptr in [q for q, _ in getattr(self, "_pin", {}).values()] + getattr(self, "_pin_retired", []):
            if ptr:
                self._lib.rt_host_free(ptr)  # (invalidates every array a pinned render() returned)
        self._pin, self._pin_retired = {}, []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def save_png(path, rgb8):
    """img.save(file_name) of main.rs:121,128: rgb8 is [ny, nx, 3] uint8 with row 0 at the top, as render(..., want_rgb8=True)
    returns it.  Written by the host library (rth_png_write), atomically."""
    lib = _ffi.load_host_library()
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("save_png: expected [ny, nx, 3] uint8")
    rc = lib.rth_png_write(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0])
    if rc != 0:
        raise RtError(f"rth_png_write({path}) failed ({rc})")


def output_file_name(unix_seconds=-1):
    """main.rs:110-112: local RFC 3339 time with ':' -> '-', cut before the fraction, + '.png'."""
    lib = _ffi.load_host_library()
    buf = C.create_string_buffer(64)
    if lib.rth_output_file_name(int(unix_seconds), buf, 64) != 0:
        raise RtError("rth_output_file_name failed")
    return buf.value.decode()


class MultiRenderer:
    """The GPUs of one node behind one handle (rt_multi_create): every device renders its row-interleaved bands, RCCL
    gathers the frame inside the library.  Replaces the thread-pool fan-out of main.rs:72-108 for a node.
    `copy_gather=True` (rt_multi_create_ex, RT_MULTI_COPY_GATHER): device-to-device copies instead of RCCL; `devices` may
    then repeat an id — several contexts side by side on one GPU, the test hook for the n > 1 code on a one-GPU box."""

    def __init__(self, devices, copy_gather=False):
        self._lib = _ffi.load_gpu_library()
        self._m = C.c_void_p()
        ids = (C.c_int * len(devices))(*devices)
        rc = self._lib.rt_multi_create_ex(ids, len(devices), _ffi.MULTI_COPY_GATHER if copy_gather else 0, C.byref(self._m))
        if rc != 0:
            raise RtError(f"rt_multi_create({list(devices)}) failed ({rc}): {self._lib.rt_multi_last_error(None).decode()}")
        self._devices = list(devices)

    def _raise(self, what, rc):
        raise RtError(f"{what} failed ({rc}): {self._lib.rt_multi_last_error(self._m).decode()}")

    @property
    def n_devices(self):
        return self._lib.rt_multi_device_count(self._m)

    def upload(self, scene):
        ptr = scene.flat_ptr if isinstance(scene, Scene) else C.pointer(scene)
        rc = self._lib.rt_multi_scene_upload(self._m, ptr)
        if rc != 0:
            self._raise("rt_multi_scene_upload", rc)

    def set_lens(self, lens):
        """rt_multi_set_lens: Renderer.set_lens on every device."""
        rc = self._lib.rt_multi_set_lens(self._m, _lens_ptr(lens))
        if rc != 0:
            self._raise("rt_multi_set_lens", rc)

    def set_motion(self, motion):
        """rt_multi_set_motion: Renderer.set_motion on every device."""
        rc = self._lib.rt_multi_set_motion(self._m, _motion_ptr(motion))
        if rc != 0:
            self._raise("rt_multi_set_motion", rc)

    def set_quads(self, quads):
        """rt_multi_set_quads: Renderer.set_quads on every device."""
        rc = self._lib.rt_multi_set_quads(self._m, _quads_ptr(quads))
        if rc != 0:
            self._raise("rt_multi_set_quads", rc)

    def set_lights(self, lights):
        """rt_multi_set_lights: Renderer.set_lights on every device."""
        rc = self._lib.rt_multi_set_lights(self._m, _lights_ptr(lights))
        if rc != 0:
            self._raise("rt_multi_set_lights", rc)

    def render(self, camera, params, want_rgb8=False):
        """Returns (f32 image [ny, nx, 3] (row 0 = bottom), rgb8 or None, RtStats summed over the devices)."""
        img = np.zeros((params.ny, params.nx, 3), dtype=np.float32)
        rgb8 = np.zeros((params.ny, params.nx, 3), dtype=np.uint8) if want_rgb8 else None
        st = RtStats()
        rc = self._lib.rt_multi_render(self._m, C.byref(camera), C.byref(params), img.ctypes.data_as(C.POINTER(C.c_float)),
                                       rgb8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgb8 else None, C.byref(st))
        if rc != 0:
            self._raise("rt_multi_render", rc)
        return img, rgb8, st

    def _call(self, what, *args):
        rc = getattr(self._lib, what)(self._m, *args)
        if rc != 0:
            self._raise(what, rc)

    def accum_begin(self, camera, params, first_sample=0, channels=False, halves=False, buckets=0):
        """rt_multi_accum_begin: Renderer.accum_begin on every device, device i on shard i of the frame of `params` (shard_band rows per
        band, 0 = 8), then the tracking asked for: channels, halves, buckets = M (0: none)."""
        track = ((_ffi.MULTI_TRACK_CHANNELS if channels else 0) | (_ffi.MULTI_TRACK_HALVES if halves else 0) |
                 (_ffi.MULTI_TRACK_BUCKETS if buckets else 0))
        self._call("rt_multi_accum_begin", C.byref(camera), C.byref(params), int(first_sample), track, int(buckets))
        self._accum_shape = (params.ny, params.nx)

    def accum_add(self, n):
        """rt_multi_accum_add: n more samples per pixel on every shard; returns the RtStats summed over the devices."""
        stats = RtStats()
        self._call("rt_multi_accum_add", int(n), C.byref(stats))
        return stats

    def accum_add_adaptive(self, n, tolerance, luminance_floor=0.01, min_samples=16):
        """rt_multi_accum_add_adaptive: Renderer.accum_add_adaptive on every shard (the decision is per pixel); the summed RtStats."""
        ad, stats = make_adaptive(tolerance, luminance_floor, min_samples), RtStats()
        self._call("rt_multi_accum_add_adaptive", int(n), C.byref(ad), C.byref(stats))
        return stats

    def accum_join(self):
        """rt_multi_accum_join: every plane of every shard into the whole-frame accumulation on the first device.  Returns a Renderer over
        that context, which this MultiRenderer owns (closing the Renderer destroys nothing): every reading accum_* call works on it and
        returns what one Renderer over the frame returns, bit for bit; every writing one raises (RT_ERR_STATE)."""
        ctx = C.c_void_p()
        self._call("rt_multi_accum_join", C.byref(ctx))
        return Renderer._borrowed(self._lib, ctx.value, self._devices[0], getattr(self, "_accum_shape", (0, 0)))

    def accum_import(self, state, halves=None, buckets=None):
        """rt_multi_accum_import: a whole-frame AccumState (and its AccumHalves / AccumBuckets) — what accum_join().accum_export*() or one
        Renderer over the frame exported — split by rows over the devices; right after accum_begin (begun without halves and buckets)."""
        st = state.as_struct()
        hs = halves.as_struct() if halves is not None else None
        bs = buckets.as_struct() if buckets is not None else None
        self._call("rt_multi_accum_import", C.byref(st), C.byref(hs) if hs is not None else None, C.byref(bs) if bs is not None else None)

    def accum_end(self):
        """rt_multi_accum_end: ends the accumulation on every device; the joined context holds nothing afterwards."""
        self._call("rt_multi_accum_end")

    def close(self):
        if self._m:
            self._lib.rt_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
