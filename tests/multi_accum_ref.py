"""Reference for the row map of rt_multi_accum_* (rtow_mi355x.h "progressive accumulation across devices") in numpy, on top of
tests/accum_state_ref.py: which image rows shard r of n owns, `split` of a whole-frame snapshot into the n shard snapshots that
rt_multi_accum_import hands the devices, and `join`, its inverse, which is what rt_multi_accum_join does to the planes.  A snapshot here is
a plain dict as in accum_state_ref: the fields of RtAccumState, optionally "halves" = dict(sum [2, rows, nx, 3], moments [2, rows, nx, 2])
and "buckets" = array [M, rows, nx, 3]; arrays in image order.  `frame` = (camera12, ny, max_depth, seed, flags): what frame_id needs."""
import numpy as np

import accum_state_ref as ref

DEFAULT_BAND = 8  # RtParams.shard_band 0 in rt_multi_*


def shard_row_map(ny, band, n, r):
    """The image rows of shard r of n in the shard's local order: lj -> ((lj // band) * n + r) * band + lj % band, while below ny."""
    band = band or DEFAULT_BAND
    if n <= 1:
        return np.arange(ny)
    return np.array([j for j in range(ny) if (j // band) % n == r], dtype=np.int64)


def _rows(a, rows, axis):
    return None if a is None else np.ascontiguousarray(np.take(a, rows, axis=axis))


def split(whole, band, n, frame=None):
    """The n shard snapshots of `whole`; with `frame` every frame_id is accum_state_ref.frame_id of that shard, else 0."""
    band = band or DEFAULT_BAND
    out = []
    for r in range(n):
        rows = shard_row_map(whole["rows"], band, n, r)
        fid = 0
        if frame is not None:
            cam12, ny, max_depth, seed, flags = frame
            fid = ref.frame_id(cam12, whole["nx"], ny, max_depth, seed, band, n, r, flags)
        s = dict(whole, rows=len(rows), frame_id=fid)
        for k in ("sum", "moments", "counts", "converged", "channel_moments"):
            s[k] = _rows(whole.get(k), rows, 0)
        if whole.get("halves") is not None:
            s["halves"] = {k: _rows(v, rows, 1) for k, v in whole["halves"].items()}
        if whole.get("buckets") is not None:
            s["buckets"] = _rows(whole["buckets"], rows, 1)
        out.append(s)
    return out


def join(shards, band, frame_id=0):
    """The whole-frame snapshot of the shard snapshots `shards` (shard r of len(shards) at index r)."""
    band = band or DEFAULT_BAND
    n = len(shards)
    ny = sum(s["rows"] for s in shards)
    maps = [shard_row_map(ny, band, n, r) for r in range(n)]
    assert [len(m) for m in maps] == [s["rows"] for s in shards]

    def put(get, axis):
        first = get(shards[0])
        if first is None:
            return None
        shape = list(first.shape)
        shape[axis] = ny
        whole = np.zeros(shape, first.dtype)
        for s, m in zip(shards, maps):
            idx = [slice(None)] * len(shape)
            idx[axis] = m
            whole[tuple(idx)] = get(s)
        return whole
    w = dict(shards[0], rows=ny, frame_id=frame_id)
    for k in ("sum", "moments", "counts", "converged", "channel_moments"):
        w[k] = put(lambda s, k=k: s.get(k), 0)
    if shards[0].get("halves") is not None:
        w["halves"] = {k: put(lambda s, k=k: s["halves"][k], 1) for k in shards[0]["halves"]}
    if shards[0].get("buckets") is not None:
        w["buckets"] = put(lambda s: s["buckets"], 1)
    return w


def designed(nx, ny, first_sample=5, done=9, M=3, seed=1, frame_id=0):
    """A whole-frame snapshot of designed bits that accum_state_ref.state_check accepts: counts and converged flags, channel moments,
    halves and M buckets; every value distinct per (pixel, plane, part), among them NaNs with payloads, both infinities and -0.0."""
    npix = nx * ny
    rng = np.random.default_rng(seed)
    tag = [0]

    def f32(shape):  # distinct finite bit patterns: a plane tag in the high mantissa bits, the element's index below
        tag[0] += 1
        n = int(np.prod(shape))
        assert n < (1 << 18) and tag[0] < 32
        bits = (np.uint32(0x3F000000) + (np.uint32(tag[0]) << np.uint32(18)) + np.arange(n, dtype=np.uint32))
        return bits.view(np.float32).reshape(shape).copy()

    def f64(shape):
        tag[0] += 1
        n = int(np.prod(shape))
        bits = (np.uint64(0x3FF0000000000000) + (np.uint64(tag[0]) << np.uint64(40)) + np.arange(n, dtype=np.uint64))
        return bits.view(np.float64).reshape(shape).copy()

    def sprinkle(a, specials):
        flat = a.reshape(-1)
        view = flat.view(np.uint32 if a.dtype == np.float32 else np.uint64)
        where = rng.choice(flat.size, size=min(len(specials), flat.size), replace=False)
        expo, mant = (0x7F800000, 0x007FFFFF) if a.dtype == np.float32 else (0x7FF0000000000000, 0x000FFFFFFFFFFFFF)
        for k, w in enumerate(where):  # a NaN's payload also carries the element's index, so the NaNs of a plane stay distinct
            nan = (specials[k] & mant) != 0 and (specials[k] & expo) == expo
            view[w] = specials[k] | ((int(w) & 0xFFFF) if nan else 0)
        return a
    s32 = [0x7FC00000 | 0x10000, 0xFFC00000 | 0x20000, 0x7F800000 | 0x30000, 0x7F800000, 0xFF800000, 0x80000000]  # qNaN, -qNaN, sNaN, +inf, -inf, -0.0
    s64 = [0x7FF8000000100000, 0xFFF8000000200000, 0x7FF0000000300000, 0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000]
    conv = (rng.random((ny, nx)) < 0.4).astype(np.uint8)
    if npix > 1:
        conv.reshape(-1)[0], conv.reshape(-1)[-1] = 0, 1
    counts = np.where(conv == 1, rng.integers(1, done + 1, (ny, nx)), done).astype(np.uint32)
    st = dict(nx=nx, rows=ny, first_sample=first_sample, done=done, planes=ref.COUNTS | ref.CHANNELS, reserved=0, frame_id=frame_id,
              sum=sprinkle(f32((ny, nx, 3)), s32), moments=sprinkle(f64((ny, nx, 2)), s64), counts=counts, converged=conv,
              channel_moments=sprinkle(f64((ny, nx, 6)), s64),
              halves=dict(sum=sprinkle(f32((2, ny, nx, 3)), s32), moments=sprinkle(f64((2, ny, nx, 2)), s64)),
              buckets=sprinkle(f32((M, ny, nx, 3)), s32))
    assert ref.state_check(st)
    return st
