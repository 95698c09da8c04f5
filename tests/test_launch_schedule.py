"""The launch schedule of a frame: `chains`, `queue_shards`, `isect_workgroups`, `materialise_primaries` and RT_FLAG_TIME_DEPTHS select
how many shard groups, streams and workgroups a slice uses and whether depth 0 reads a materialised queue.  RtCtx promises that every
setting renders the same bits; this holds the promise at a size where every branch of the slice loop runs: three slices (the last one
short), two shard groups of equal and of unequal size, the doubling of the k_intersect grid, the single timed chain."""
import numpy as np
import pytest

MAX_DEPTH = 6
# (options, flags): every one must render what all-zero options render
SETTINGS = [
    ({"chains": 1}, 0),
    ({"chains": 2}, 0),
    ({"queue_shards": 7}, 0),                           # one group: below 2 * RT_ISECT_MAX_SHARDS
    ({"queue_shards": 8}, 0),                           # two groups of 4
    ({"queue_shards": 9}, 0),                           # groups of 4 and 5
    ({"queue_shards": 9, "isect_workgroups": 1}, 0),    # one workgroup would own 9 shards: the grid doubles until it owns <= RT_ISECT_MAX_SHARDS
    ({"isect_workgroups": 3}, 0),
    ({}, 4),                                            # RT_FLAG_TIME_DEPTHS: one chain, events around every launch of the first slice
    ({"materialise_primaries": 1}, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,nx,ny", [("sphere_scene", 64, 36), ("cornell_box", 48, 48)])
def test_every_launch_schedule_renders_the_same_frame(rt, name, nx, ny):
    f = rt._ffi
    scene = rt.Scene.build(name, nx / ny)
    r = rt.Renderer(0)
    try:
        r.upload(scene)

        def render(options, flags=0, spp=5):
            for opt in f.OPT_NAMES.values():
                r.set_option(opt, 0)
            for opt, value in options.items():
                r.set_option(opt, value)
            img, _, st = r.render(scene.camera, rt.make_params(nx, ny, spp, max_depth=MAX_DEPTH, seed=7, spp_slice=2, flags=flags))
            return img, st

        base, sb = render({})
        assert sb.n_slices == 3 and base.std() > 0.01
        for options, flags in SETTINGS:
            img, st = render(options, flags)
            assert np.array_equal(img.view(np.uint32), base.view(np.uint32)), (name, options, flags)
            assert st.n_rays == sb.n_rays and list(st.rays_per_depth) == list(sb.rays_per_depth) and st.n_slices == sb.n_slices, (name, options, flags)
        # per-depth timing covers the first slice: samples 0 and 1 of every pixel, what a one-slice render of 2 spp traces
        _, st2 = render({}, spp=2)
        assert st2.n_slices == 1
        render({}, f.FLAG_TIME_DEPTHS)
        isect_ms, shade_ms, rays = r.depth_timings()
        assert len(isect_ms) == len(shade_ms) == len(rays) == MAX_DEPTH + 1
        assert [int(x) for x in rays] == list(st2.rays_per_depth)[:MAX_DEPTH + 1]
        # without candidate lists no depth skips its closest-hit launch: two logical launches per depth and slice
        _, sl = render({"primary_lists": 1})
        assert sl.n_trace_launches == 2 * (MAX_DEPTH + 1) * sl.n_slices and sl.n_slices == 3
    finally:
        r.close()
