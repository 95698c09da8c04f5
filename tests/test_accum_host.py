"""Accumulation and noise without a GPU: the layout of RtNoise against the C compiler, and tests/noise_ref.py — the reference the GPU tests
of tests/test_accum.py hold the kernels to — against numpy's own variance."""
import ctypes as C
import os
import subprocess

import numpy as np

import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtnoise_layout_matches_the_c_compiler(rt, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(RtNoise),offsetof(RtNoise,spp_done),offsetof(RtNoise,reserved),offsetof(RtNoise,mean_luminance),'
                   'offsetof(RtNoise,rms_sem),offsetof(RtNoise,noise));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    n = rt._ffi.RtNoise
    assert got == [C.sizeof(n), n.spp_done.offset, n.reserved.offset, n.mean_luminance.offset, n.rms_sem.offset, n.noise.offset] == [32, 0, 4, 8, 16, 24]


def test_the_accumulation_entry_points_are_bound(rt):
    lib = rt._ffi.load_gpu_library()
    for name in ("rt_accum_begin", "rt_accum_add", "rt_accum_read", "rt_accum_end", "rt_render_to_noise"):
        assert name in rt._ffi.GPU_SYMBOLS and getattr(lib, name).restype is C.c_int
    for name in ("accum_begin", "accum_add", "accum_read", "accum_end", "render_to_noise"):
        assert callable(getattr(rt.Renderer, name))
    assert rt.RtNoise is rt._ffi.RtNoise


def _samples(n, rows=5, nx=7, seed=3):
    """Per-sample frames whose every pixel has contrast: even samples are dim (0.1 .. 0.5 of the pixel's level), odd ones bright (1 .. 2).
    The one-pass formula S2 - S1 S1 / n loses log2(kappa) bits, kappa = S2 / (S2 - S1 S1 / n) ~ 1 + mean^2 / variance; here
    mean^2 / variance stays below 10 for every n >= 2, so a handful of f64 roundings (2^-53 each) times kappa lies far inside the 1e-12
    the comparison with numpy's two-pass variance allows.  (Two samples that happen to agree to 4 digits would not: kappa 1e8.)"""
    rng = np.random.default_rng(seed)
    level = rng.uniform(0.05, 4.0, size=(rows, nx, 1))
    return [(level * (rng.uniform(1.0, 2.0, size=(rows, nx, 3)) if s & 1 else rng.uniform(0.1, 0.5, size=(rows, nx, 3)))).astype(np.float32)
            for s in range(n)]


def test_variance_of_the_mean_is_numpys():
    for n in (2, 3, 7, 64):
        x = _samples(n)
        total, s1, s2, cnt = noise_ref.accumulate(x)
        assert cnt == n
        y = np.stack([noise_ref.luminance(f) for f in x])
        ybar, v = noise_ref.pixel_figures(s1, s2, n)
        want = np.var(y, axis=0, ddof=1) / n
        assert np.all(np.abs(v - want) <= 1e-12 * want), float(np.max(np.abs(v - want) / want))
        assert np.all(np.abs(ybar - y.mean(axis=0)) <= 1e-12 * ybar)
        assert np.array_equal(noise_ref.sem(s1, s2, n), np.sqrt(v).astype(np.float32))
        mean, rms, noise = noise_ref.frame_figures(s1, s2, n)
        assert abs(mean - y.mean()) <= 1e-12 * mean and abs(rms - np.sqrt(want.mean())) <= 1e-12 * rms and noise == rms / mean
        # the f32 sum is sequential: one rounding per sample
        seq = np.zeros_like(x[0])
        for f in x:
            seq = (seq + f).astype(np.float32)
        assert np.array_equal(total.view(np.uint32), seq.view(np.uint32))


def test_luminance_is_the_three_term_sum_in_order():
    x = np.array([[[0.1, 0.7, 0.3]]], np.float32)
    r, g, b = (np.float64(v) for v in x[0, 0])
    assert noise_ref.luminance(x)[0, 0] == (0.2126 * r + 0.7152 * g) + 0.0722 * b


def test_no_variance_from_one_sample_or_constant_samples():
    x = _samples(1)
    _, s1, s2, n = noise_ref.accumulate(x)
    assert n == 1 and not noise_ref.pixel_figures(s1, s2, 1)[1].any() and not noise_ref.sem(s1, s2, 1).any()
    assert noise_ref.frame_figures(s1, s2, 1)[2] == np.inf  # no estimate yet
    const = [np.full((4, 6, 3), 0.3, np.float32)] * 5  # (S2 - S1 S1 / n may round below 0: clamped)
    _, s1, s2, n = noise_ref.accumulate(const)
    ybar, v = noise_ref.pixel_figures(s1, s2, n)
    assert np.all(v >= 0.0) and np.all(v <= 1e-30) and np.allclose(ybar, noise_ref.luminance(const[0]))
    exact = [np.full((4, 6, 3), 0.5, np.float32)] * 4  # exactly representable: V is exactly 0
    _, s1, s2, n = noise_ref.accumulate(exact)
    assert not noise_ref.pixel_figures(s1, s2, n)[1].any() and noise_ref.frame_figures(s1, s2, n)[2] == 0.0


def test_noise_of_black_and_empty_frames():
    black = [np.zeros((3, 4, 3), np.float32)] * 3
    assert noise_ref.noise_of(black) == (0.0, 0.0, 0.0)  # mean 0 and rms 0: 0
    assert noise_ref.noise_of([]) == (0.0, 0.0, np.inf)  # nothing added
    assert noise_ref.noise_of(black[:1]) == (0.0, 0.0, np.inf)  # n < 2
    # mean 0, rms > 0: +inf (luminances that cancel)
    a = np.zeros((1, 2, 3), np.float32)
    a[0, 0, 1], a[0, 1, 1] = 1.0, -1.0
    mean, rms, noise = noise_ref.noise_of([a, -a, a])
    assert mean == 0.0 and rms > 0.0 and noise == np.inf
