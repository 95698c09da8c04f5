"""The figures behind RT_GLARE_DEFAULT_AMOUNT and RT_GLARE_DEFAULT_SPREAD (DESIGN.md "Glare"):
python scripts/glare_defaults.py [--spp 256 --out-dir DIR]
Renders the cornell-box frame and the simple_light frame, then puts the f32 image of each through rt_debug_glare on the grid amount in
{0.05, 0.1, 0.2} x spread in {0.5, 0.7, 1}, levels 6, threshold 0, behind the reference quantisation.  One JSON line; per frame and
configuration, against the un-glared 8-bit image:
  halo      the share of the pixels that were not saturated and gain at least one 8-bit level in their brightest channel — the glow one sees
  veil      the mean rise, in 8-bit levels, of the darkest half of the pixels (by luminance) — the fog one does not want
  veil_max  the largest rise among them
  lost      the share of the values at 255 that leave 255 — emitters that stop looking white
  energy    sum(out) / sum(c) - 1 over the frame (the border rule; 0 in the interior)
--out-dir: also the PNGs, <frame>_a<amount>_s<spread>.png and <frame>_plain.png."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ray_tracing_in_one_weekend_amd as rt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=256)
ap.add_argument("--out-dir", default=None)
args = ap.parse_args()

rt.register_default_images()
FRAMES = (("cornell_box", 512, 512), ("simple_light_scene", 640, 360))
GRID = [(a, s) for a in (0.05, 0.1, 0.2) for s in (0.5, 0.7, 1.0)]
F32 = np.float32


def luminance(img):
    return 0.2126 * img[..., 0] + 0.7152 * img[..., 1] + 0.0722 * img[..., 2]


out = {"spp": args.spp, "levels": 6, "threshold": 0.0}
r = rt.Renderer(0)
out["build"] = r.build_id
for name, nx, ny in FRAMES:
    scene = rt.Scene.build(name, nx / ny)
    r.upload(scene)
    img, rgb8, _ = r.render(scene.camera, rt.make_params(nx, ny, args.spp), want_rgb8=True)
    y = luminance(np.nan_to_num(img[::-1].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))  # row 0 on top, as rgb8
    dark = y <= np.median(y)
    base = rgb8.astype(np.int32)
    unsat = base.max(axis=-1) < 255
    frame = {"nx": nx, "ny": ny, "saturated_values": int((base == 255).sum()), "dark_half_mean_level": float(base[dark].mean()),
             "mean_luminance": float(y.mean()), "max_luminance": float(y.max())}
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        rt.save_png(os.path.join(args.out_dir, f"{name}_plain.png"), rgb8)
    for a, s in GRID:
        glared, g8, info = r.debug_glare(img, rt.make_glare(a, s, 0.0, 6))
        rise = g8.astype(np.int32) - base
        frame[f"a{a} s{s}"] = {
            "halo": float((rise.max(axis=-1)[unsat] >= 1).mean()),
            "veil": float(rise[dark].mean()),
            "veil_max": int(rise[dark].max()),
            "lost": float(((base == 255) & (g8 < 255)).sum() / max(1, (base == 255).sum())),
            "energy": float(np.nansum(glared.astype(np.float64)) / np.nansum(np.where(np.isfinite(img), np.maximum(img, 0), 0).astype(np.float64)) - 1),
            "levels": info.levels,
        }
        if args.out_dir:
            rt.save_png(os.path.join(args.out_dir, f"{name}_a{a}_s{s}.png"), g8)
    out[name] = frame
r.close()
print(json.dumps(out))
