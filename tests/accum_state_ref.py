"""Reference for the accumulation state of rtow_mi355x.h ("accumulation state") in numpy: the frame identity (FNV-1a 64 over the bytes the
header lists), the well-formedness check, the merge as np.float32 / np.float64 additions, and the state an accumulation must export after
given adds — predicted from single-sample frames with noise_ref.accumulate, adaptive_ref.Replay and denoise_channels_ref.  A state here
is a plain dict with the fields of RtAccumState; arrays are in image order, [rows, nx(, k)]."""
import struct

import numpy as np

import adaptive_ref
import denoise_channels_ref
import noise_ref

COUNTS, CHANNELS = 1, 2
FLAG_RUSSIAN_ROULETTE = 2
FNV_OFFSET, FNV_PRIME, MASK64 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1


def fnv1a64(data):
    h = FNV_OFFSET
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & MASK64
    return h


def frame_bytes(camera12, nx, ny, max_depth, seed, shard_band=0, shard_count=1, shard_id=0, flags=0):
    """The little-endian bytes the identity is taken over.  camera12: the 12 camera floats in struct order (origin, horizontal, vertical,
    lower_left_corner), as f32 values — their bit patterns enter."""
    cam = np.asarray(camera12, dtype=np.float32).reshape(12)
    if shard_count <= 1:
        shard_band, shard_count, shard_id = 0, 1, 0
    return (cam.astype("<f4").tobytes() + struct.pack("<III", nx, ny, max_depth & 0xFFFFFFFF) + struct.pack("<Q", seed) +
            struct.pack("<III", shard_band, shard_count, shard_id) + struct.pack("<I", flags & FLAG_RUSSIAN_ROULETTE))


def frame_id(camera12, nx, ny, max_depth, seed, shard_band=0, shard_count=1, shard_id=0, flags=0):
    return fnv1a64(frame_bytes(camera12, nx, ny, max_depth, seed, shard_band, shard_count, shard_id, flags))


def camera12(cam):
    """The 12 floats of an RtCamera (ctypes) in struct order."""
    return [float(v) for part in (cam.origin, cam.horizontal, cam.vertical, cam.lower_left_corner) for v in part]


def frame_id_of(cam, p):
    """frame_id of an RtCamera and an RtParams (ctypes)."""
    return frame_id(camera12(cam), p.nx, p.ny, p.max_depth, p.seed, p.shard_band, p.shard_count, p.shard_id, p.flags)


def state_check(st):
    """rt_accum_state_check on a dict: None stands for a NULL pointer.  True when the state is well formed."""
    if st.get("reserved", 0) != 0 or st["planes"] & ~(COUNTS | CHANNELS):
        return False
    if st.get("sum") is None or st.get("moments") is None:
        return False
    counts, channels = bool(st["planes"] & COUNTS), bool(st["planes"] & CHANNELS)
    if counts != (st.get("counts") is not None) or counts != (st.get("converged") is not None):
        return False
    if channels != (st.get("channel_moments") is not None):
        return False
    if st["first_sample"] + st["done"] > 2 ** 32 - 1:
        return False
    if counts:
        cnt, conv = np.asarray(st["counts"]).astype(np.uint64), np.asarray(st["converged"])
        if (conv > 1).any() or (cnt > st["done"]).any() or (cnt[conv == 0] != st["done"]).any():
            return False
    return True


def make_state(nx, rows, first_sample, done, fid, total, s1, s2, counts=None, converged=None, channel_moments=None):
    planes = (COUNTS if counts is not None else 0) | (CHANNELS if channel_moments is not None else 0)
    return dict(nx=nx, rows=rows, first_sample=first_sample, done=done, planes=planes, reserved=0, frame_id=fid,
                sum=np.asarray(total, np.float32), moments=np.stack([np.asarray(s1, np.float64), np.asarray(s2, np.float64)], axis=-1),
                counts=None if counts is None else np.asarray(counts, np.uint32),
                converged=None if converged is None else np.asarray(converged, np.uint8),
                channel_moments=None if channel_moments is None else np.asarray(channel_moments, np.float64))


def channel_moments(frames):
    """[rows, nx, 6] f64: S1_r, S2_r, S1_g, S2_g, S1_b, S2_b of the frames in sample order (denoise_channels_ref.accumulate_channels)."""
    s1, s2 = denoise_channels_ref.accumulate_channels(frames)[:2]
    out = np.zeros(s1.shape[:2] + (6,), np.float64)
    out[..., 0::2], out[..., 1::2] = s1, s2
    return out


def channel_moments_counted(frames, counts):
    """channel_moments of an adaptive accumulation: pixel p holds its first counts[p] frames."""
    s1, s2 = denoise_channels_ref.accumulate_channels(frames, counts)[:2]
    out = np.zeros(s1.shape[:2] + (6,), np.float64)
    out[..., 0::2], out[..., 1::2] = s1, s2
    return out


def uniform_state(frames, first_sample, fid, channels=False):
    """The state of rt_accum_begin(first_sample) and uniform adds over `frames` = x[first_sample], x[first_sample + 1], ..."""
    frames = list(frames)
    total, s1, s2, n = noise_ref.accumulate(frames)
    rows, nx = total.shape[:2]
    return make_state(nx, rows, first_sample, n, fid, total, s1, s2, channel_moments=channel_moments(frames) if channels else None)


def replay_state(rp, fid):
    """The state of an adaptive accumulation that adaptive_ref.Replay `rp` has followed (it begins at sample 0)."""
    rows, nx = rp.cnt.shape
    return make_state(nx, rows, 0, rp.issued, fid, rp.total, rp.s1, rp.s2, counts=rp.cnt, converged=rp.conv.astype(np.uint8))


def merge(a, b):
    """rt_accum_merge: state b, the window that continues a's, added onto a — one np.float32 add per channel sum, one np.float64 add per
    moment.  Raises ValueError where the library refuses."""
    if (a["planes"] | b["planes"]) & COUNTS:
        raise ValueError("unsupported: adaptive")
    if (a["nx"], a["rows"], a["frame_id"]) != (b["nx"], b["rows"], b["frame_id"]) or b["first_sample"] != a["first_sample"] + a["done"]:
        raise ValueError("invalid: not the window that follows")
    if a["planes"] != b["planes"] or a["first_sample"] + a["done"] + b["done"] > 2 ** 32 - 1:
        raise ValueError("invalid")
    out = dict(a, done=a["done"] + b["done"])
    with np.errstate(invalid="ignore", over="ignore"):
        out["sum"] = (a["sum"].astype(np.float32) + b["sum"].astype(np.float32)).astype(np.float32)
        out["moments"] = a["moments"].astype(np.float64) + b["moments"].astype(np.float64)
        if a["planes"] & CHANNELS:
            out["channel_moments"] = a["channel_moments"].astype(np.float64) + b["channel_moments"].astype(np.float64)
    return out
