"""The measurement behind the defaults of a NULL RtSelect: python scripts/select_defaults.py
On the two bit-reproducible cornell_box frames of tests/test_select.py (64 x 64, depth 8, 16 spp, with and without Scene.lights, against
4 096 spp of another seed): the RMSE of rt_accum_denoise_select for every error_radius S and blend_radius T in {0, 1, 2, 4}, for the four
default candidates and for the three of DESIGN.md 4.10, beside the RMSE of rt_accum_denoise_halves at every candidate; and `best`,
est_mse and how many pixels chose each candidate.  One line per row, then one JSON line with all of it."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ray_tracing_in_one_weekend_amd as rt  # noqa: E402

SEED = 1234
rt.register_default_images()
rmse = lambda a, b: float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))
r = rt.Renderer(0)
scene = rt.Scene.build("cornell_box", 1.0)
r.upload(scene)
out = {"build": r.build_id}
for which in ("lights", "no_lights"):
    r.set_lights(scene.lights if which == "lights" else None)
    truth = r.render(scene.camera, rt.make_params(64, 64, 4096, max_depth=8, seed=SEED + 1))[0]
    r.accum_begin(scene.camera, rt.make_params(64, 64, 16, max_depth=8, seed=SEED))
    r.accum_track_halves()
    r.accum_add(16)
    noisy = rmse(r.accum_read()[0], truth)
    res = {"16 spp": noisy}
    for ks in ((0.45, 0.7, 1.0, 1.4), (0.45, 0.7, 1.0), (0.7, 1.0, 1.4), (0.7, 1.4)):
        single = {k: rmse(r.accum_denoise_halves(strength=k)[0], truth) for k in ks}
        print(f"{which} candidates {ks}: 16 spp {noisy:.5f}, single " + " / ".join(f"{e:.5f}" for e in single.values()))
        for S in (0, 1, 2, 4):
            row = []
            for T in (0, 1, 2, 4):
                img, _, index, est, info = r.accum_denoise_select(rt.make_select(ks, 5, 1, S, T))
                row.append(rmse(img, truth))
                res[f"{ks} S {S} T {T}"] = row[-1]
            print(f"  S {S}: T 0 / 1 / 2 / 4: " + " / ".join(f"{e:.5f}" for e in row) + f"; best {info.best}, chosen {list(info.chosen)}, est_mse " +
                  " / ".join(f"{e:.6f}" for e in list(info.est_mse)[:len(ks)]) + f", selected {info.est_mse_selected:.6f}")
    r.accum_end()
    out[which] = res
r.set_lights(None)
r.close()
print(json.dumps(out))
