"""A frame as the in-order sum of its paths: the reference of tests/test_frame_replay.py for frames under rt_set_lens, rt_set_motion,
rt_set_quads and rt_set_lights, which the oracle does not know.

Nothing of the frame machinery is used: no queue, slot, tile, candidate list, slice, resolve or finalize.  A path is named by
(pixel, sample) alone.  Its primary ray is helpers.primary_rays (the pinhole) or lens_ref.lens_rays (a lens), its key helpers.path_keys.
Each bounce is Renderer.debug_bounce(o, d, keys, depth, FLAG_BRUTE_FORCE): the single-kernel list walk over caller-given rays, which
tests/test_gpu_parity.py, test_motion.py, test_quads.py, test_lights.py and test_lights_materials.py hold per ray to the oracle, np_ref,
motion_ref, quad_ref, light_ref and pbr_ref64 under every set.  With motion the hook derives the ray's time from the key it is given
(counter 254), as motion_ref.path_time does; the replay computes that time too and keeps it for the report of a differing ray.

The estimator order is that of k_shade (rt_kernels.h), restated:
    T_0 = (1, 1, 1);  a ray whose fl(fl(dx dx + dy dy) + dz dz) lies outside [0x3f7fffe0, 0x3f800011] is dropped: its path is worth 0;
    a path that ends at depth k is worth T_k * radiance_k, component by component, one f32 product each (radiance = emitted | sky);
    a path that scatters goes on with T_{k+1} = T_k * attenuation_k, component by component, one f32 product each;
    a path that still scatters at depth max_depth is worth 0.  Russian roulette is off.
A pixel is ((((0 + x[0]) + x[1]) + ...) + x[spp - 1]) / f32(spp) in f32, per channel: k_resolve adds a slice's samples onto the running sum
in sample order, one addition each, and k_finalize divides once."""
import numpy as np

import lens_ref
import motion_ref
from helpers import primary_rays

f32 = np.float32
FLAG_BRUTE_FORCE = 1
NEAR_ONE_LO, NEAR_ONE_HI = np.uint32(0x3f7fffe0).view(f32), np.uint32(0x3f800011).view(f32)
SKY, EMITTER, ABSORBED, DEPTH_LIMIT, DROPPED = range(5)  # how a path ended
END_NAMES = ("sky", "emitter", "absorbed", "depth limit", "dropped")


# ---- rows of a shard (rt_shard_rows / rt_shard_row_to_image_row, restated) -------------------------------------------------------------
def shard_image_rows(ny, band=0, count=1, sid=0):
    """The image rows of shard `sid`, in the shard's local row order: the rows j with (j // band) % count == sid."""
    if count <= 1:
        return np.arange(ny, dtype=np.int64)
    band = band or 1
    j = np.arange(ny, dtype=np.int64)
    return j[(j // band) % count == sid]


def local_row_to_image_row(lj, band, count, sid):
    if count <= 1:
        return lj
    band = band or 1
    return ((lj // band) * count + sid) * band + lj % band


# ---- sums ---------------------------------------------------------------------------------------------------------------------------
def sum_in_order(x, spp=None):
    """x [n, rows, nx, 3] f32 -> the f32 sum of the first spp frames, one addition per sample, in sample order"""
    x = np.asarray(x, f32)
    total = np.zeros(x.shape[1:], f32)
    for s in range(len(x) if spp is None else spp):
        total = (total + x[s]).astype(f32)
    return total


def mean_in_order(x, spp=None):
    n = len(x) if spp is None else spp
    return (sum_in_order(x, spp) / f32(n)).astype(f32)


def near_one(d):
    d = np.asarray(d, f32)
    l2 = (((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32) + (d[:, 2] * d[:, 2]).astype(f32)).astype(f32)
    return (l2 >= NEAR_ONE_LO) & (l2 <= NEAR_ONE_HI)  # (a NaN fails both)


class Frame:
    """The replay of a whole frame (every image row; a shard is a selection of rows).
    x [spp, ny, nx, 3] f32: the value of path (sample, row, column); last [spp, ny, nx]: the depth of its last ray; how: SKY .. DROPPED;
    bounces: per depth a dict(path, keys, hit, alive) over the rays of that depth (path = flat index into [spp, ny, nx])."""

    def __init__(self, x, last, how, bounces, max_depth):
        self.x, self.last, self.how, self.bounces, self.max_depth = x, last, how, bounces, max_depth
        for a in (self.x, self.last, self.how):
            a.setflags(write=False)
        self.spp, self.ny, self.nx = last.shape

    def frames(self, rows=None, spp=None):
        """x[s] over the given image rows (a shard's, in its local order): what adaptive_ref.Replay and noise_ref.accumulate take"""
        x = self.x if rows is None else self.x[:, rows]
        return [x[s] for s in range(self.spp if spp is None else spp)]

    def image(self, rows=None, spp=None):
        x = self.x if rows is None else self.x[:, rows]
        if x.shape[1] == 0:
            return np.zeros((0, self.nx, 3), f32)
        return mean_in_order(x, spp)

    def rays_per_depth(self, rows=None, samples=None):
        """rays traced at depth 0 .. max_depth by the paths of the given rows and samples"""
        last = self.last if rows is None else self.last[:, rows]
        if samples is not None:
            last = last[samples]
        return [int((last >= k).sum()) for k in range(self.max_depth + 1)]

    def ends(self):
        return {END_NAMES[k]: int((self.how == k).sum()) for k in range(5)}


def _describe(k, depth, o, d, keys, tm, a, b):
    tail = "" if tm is None else ", time %r" % float(tm[k])
    return ("depth %d, ray o %r d %r key %r%s: list walk hit %d t %r alive %d, default hook hit %d t %r alive %d"
            % (depth, o[k].tolist(), d[k].tolist(), keys[k].tolist(), tail, a["hit"][k], float(a["t"][k]), a["alive"][k], b["hit"][k],
               float(b["t"][k]), b["alive"][k]))


def _hooks_agree(depth, o, d, keys, tm, a, b):
    """the list walk (a) and the context's default search (b) on the same rays: everything the replay reads"""
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)
    live = a["alive"] == 1
    bad = (a["hit"] != b["hit"]) | (bits(a["t"]) != bits(b["t"])) | (a["alive"] != b["alive"])
    bad |= ~live & (bits(a["radiance"]) != bits(b["radiance"])).any(axis=1)
    for key in ("o", "d", "attenuation"):
        bad |= live & (bits(a[key]) != bits(b[key])).any(axis=1)
    if bad.any():
        raise AssertionError("the two single-kernel hooks disagree on %d replayed rays; the first: %s"
                             % (int(bad.sum()), _describe(int(np.nonzero(bad)[0][0]), depth, o, d, keys, tm, a, b)))


def replay(r, scene, p, lens=None, shutter=None, cross_check=True):
    """The frame of params `p` (nx, ny, spp, max_depth, seed; every row, whatever shard p names) on Renderer `r`, which holds the
    uploaded scene and its sets.  lens: (lens_radius, focus_dist) or None; shutter: (open, close) when a motion set is on.
    cross_check: every replayed ray also goes through debug_bounce(flags=0), and a difference raises with the ray."""
    nx, ny, spp, max_depth = int(p.nx), int(p.ny), int(p.spp), int(p.max_depth)
    ss, jj, ii = np.meshgrid(np.arange(spp), np.arange(ny), np.arange(nx), indexing="ij")
    s, j, i = ss.ravel(), jj.ravel(), ii.ravel()
    n = len(s)
    if lens is not None and f32(lens[0]) > 0:
        o, d, keys = lens_ref.lens_rays(scene.camera, p, i, j, s, lens[0], lens[1])
    else:
        o, d, keys = primary_rays(scene, p, i, j, s)
    tm_all = motion_ref.path_time(keys, *shutter) if shutter is not None else None
    value = np.zeros((n, 3), f32)
    last = np.zeros(n, np.int64)
    how = np.full(n, -1, np.int64)
    T = np.ones((n, 3), f32)
    path = np.arange(n)
    bounces = []
    for depth in range(max_depth + 1):
        if len(path) == 0:
            break
        last[path] = depth
        ok = near_one(d)
        how[path[~ok]] = DROPPED  # (worth 0)
        path, o, d, T = path[ok], o[ok], d[ok], T[ok]
        if len(path) == 0:
            bounces.append(dict(path=path, keys=keys[path], hit=np.zeros(0, np.int32), alive=np.zeros(0, np.uint8)))
            break
        k = keys[path]
        out = r.debug_bounce(o, d, k, depth=depth, flags=FLAG_BRUTE_FORCE)
        if cross_check:
            _hooks_agree(depth, o, d, k, None if tm_all is None else tm_all[path], out, r.debug_bounce(o, d, k, depth=depth, flags=0))
        bounces.append(dict(path=path, keys=k, hit=out["hit"].copy(), alive=out["alive"].copy()))
        live = out["alive"] == 1
        ended = path[~live]
        value[ended] = (T[~live] * out["radiance"][~live]).astype(f32)  # L = T_n * (emitted | sky)
        emits = (out["radiance"][~live] != 0).any(axis=1)
        how[ended] = np.where(out["hit"][~live] < 0, SKY, np.where(emits, EMITTER, ABSORBED))
        if depth == max_depth:
            how[path[live]] = DEPTH_LIMIT  # (worth 0)
            break
        path, o, d = path[live], out["o"][live], out["d"][live]
        T = (T[live] * out["attenuation"][live]).astype(f32)  # T_{k+1} = T_k * a_k
    assert (how >= 0).all()
    shape = (spp, ny, nx)
    return Frame(value.reshape(shape + (3,)), last.reshape(shape), how.reshape(shape), bounces, max_depth)
