// rt_features.h — the first-hit features of an accumulation (rtow_mi355x.h "First-hit features"): new kernels only; no kernel of
// rt_kernels.h, rt_grid.h, rt_adaptive.h, rt_denoise.h, rt_filter.h or rt_accum_state_kernels.h changes.  k_features is a family of its own:
// it is no k_shade, k_intersect or k_debug_bounce key, so it enters no variant table and no ledger family.
//
//   k_features<USE_BVH, LDS_NODES, MOTION, PLANAR, LENS> : the contributing samples of a window onto the record of every pixel
//   k_features_read                                      : the read-out of rt_accum_read_features in image order
//   k_features_inputs, k_features_demodulate, k_denoise_features<F> : the feature-guided filter (rtow_mi355x.h "The feature-guided filter")
// (rt_accum_export_features and _import_features move the records as ONE PlaneTable row of 16 B elements in 4 parts through k_planes_move,
// rt_accum_state_kernels.h: rt_features_plan.h.)
//
// k_features.  A workgroup of RT_BVH_BLOCK threads owns a 32 x 32 block of image pixels, lane t the pixel (t & 31, t >> 5) of it — whatever
// the local pixel order: the record and the converged flag are found through local_of_pixel, as k_resolve_filter finds its slots.  The
// search state is staged ONCE per workgroup (stage_bvh: the tree and the geometry in LDS where the scene upload put them there, else only
// the traversal stacks) and serves every sample of the window; the thread keeps its record in registers between one load and one store of
// its four quarters.  Per sample: the primary ray by gen_primary<LENS> itself (the slice's GenParams with s0 = the sample and the slot =
// the local pixel, so the key, the jitter and the lens draws are the render's operation for operation), its time by path_time, the closest
// hit by the code of k_debug_bounce — bvh_step and media_step on the tree, or the list walk (closest_hit_tile / _spheres_general, _rects,
// _planar) where the context has no tree or RT_FLAG_BRUTE_FORCE is set — and the surface record by first_hit_surface below.
//
// first_hit_surface RESTATES the part of shade() (rt_device.h) that rebuilds p, the outward normal, the face-forwarded normal unwound
// through the wrappers, the rectangle / planar uv and the value of the material's first texture.  A restatement, not a shared helper, so
// that shade() and every kernel built from it keep their bytes without having to be shown to.  It is shade<RECTS = true, NEST = true>: the
// general form, which every scene may run.  Whoever changes one changes the other; tests/test_features.py holds the albedo to shade()'s
// attenuation through rt_debug_bounce and the normal to a numpy restatement of the reference's HitRecord.
#pragma once
#include "rt_accum_state_kernels.h"
#include "rt_denoise.h"
#include "rt_features_plan.h"

namespace rt {

// What one feature sample adds to a record (the header's a, n, hit, z).
struct FeatureSample {
    V3 a, n;
    float z;
    bool hit;
};

__device__ __forceinline__ float feature_clamp01(float x) { return x == x ? fminf(fmaxf(x, 0.0f), 1.0f) : 0.0f; } // (NaN -> 0)

// The HitRecord of a known closest hit and what the header derives from it.  `ro`, `rd`: the world ray.
template <bool MOTION, bool PLANAR>
__device__ __forceinline__ FeatureSample first_hit_surface(const DevScene& sc, const PerlinTables& pt, V3 ro, V3 rd, int hit, float t, const float4* sph_dc,
                                                           float tm, const float4* pq, uint32_t pbase) {
    FeatureSample fs;
    fs.a = splat(1.0f), fs.n = splat(0.0f), fs.z = 0.0f, fs.hit = false;
    if (hit < 0) return fs;
    fs.hit = true, fs.z = t;
    const float4* rec = sc.sph_rec + 5u * (uint32_t)hit;
    float4 g = rec[0];
    const float4 r1 = rec[1], r2 = rec[2];
    if (MOTION && (uint32_t)hit < sc.n_spheres) g = sphere_at(g, sph_dc[hit], tm);
    const bool is_planar = PLANAR && (uint32_t)hit >= pbase;
    const bool is_medium = !is_planar && (uint32_t)hit >= sc.n_prims;
    const bool is_rect = !is_planar && !is_medium && (uint32_t)hit >= sc.n_spheres;
    Chain chain;
    chain.n = 0;
    uint32_t deep_n = 0u, deep_p0 = 0u;
    const V3 wo = ro, wd = rd;
    if (!is_planar) {
        const uint32_t xf = is_medium ? sc.med_xform[(uint32_t)hit - sc.n_prims].y : sc.prim_xform[hit];
        deep_p0 = xf != RT_NO_XFORM_DEV ? __float_as_uint(sc.xf_param[xf].w) : 0u;
        if (deep_p0 != 0u) {
            deep_n = sc.xf_meta[deep_p0].y;
            for (uint32_t k = 0; k < deep_n; ++k) xform_ray(sc, sc.xf_meta[deep_p0 + k].x, ro, rd);
        } else {
            chain = load_chain(sc, xf);
            chain_to_object(sc, chain, ro, rd);
        }
    }
    V3 p = ro + rd * t;
    V3 on;
    V2 rect_uv = V2{0.0f, 0.0f};
    if (is_rect) {
        const float4 g1 = rec[4];
        const uint32_t axis = __float_as_uint(g1.y);
        const float pu = axis == 0u ? p.y : p.x;
        const float pv = axis == 2u ? p.y : p.z;
        rect_uv = V2{(pu - g.y) / (g.z - g.y), (pv - g.w) / (g1.x - g.w)};
        on = v3(axis == 0u ? 1.0f : 0.0f, axis == 1u ? 1.0f : 0.0f, axis == 2u ? 1.0f : 0.0f);
    } else if (is_planar) {
        const float4* g5 = pq + 5u * ((uint32_t)hit - pbase);
        const float4 nd = g5[0];
        planar_coords(g5, p, rect_uv.x, rect_uv.y);
        on = v3(nd.x, nd.y, nd.z);
    } else if (is_medium) {
        on = v3(1.0f, 0.0f, 0.0f);
    } else {
        const SharedRcp rr = shared_rcp(g.w);
        const V3 pc = p - v3(g.x, g.y, g.z);
        on = v3(div_shared(pc.x, rr), div_shared(pc.y, rr), div_shared(pc.z, rr));
    }
    bool front_face = is_medium ? true : dot(rd, on) < 0.0f;
    V3 n = front_face ? on : -on;
    if (chain.n > 0) {
#pragma unroll
        for (int k = 0; k < RT_MAX_CHAIN; ++k) {
            if (k < chain.n) {
                const uint32_t x = chain.id[k];
                const float4 q = sc.xf_param[x];
                if (sc.xf_meta[x].x == 0u) {
                    p = p + v3(q.x, q.y, q.z);
                } else {
                    const float sin_theta = q.x, cos_theta = q.y;
                    const float px = cos_theta * p.x + sin_theta * p.z, pz = -sin_theta * p.x + cos_theta * p.z;
                    const float nx = cos_theta * n.x + sin_theta * n.z, nz = -sin_theta * n.x + cos_theta * n.z;
                    p.x = px, p.z = pz, n.x = nx, n.z = nz;
                    V3 dk = wd, ok = wo;
#pragma unroll
                    for (int j = RT_MAX_CHAIN - 1; j >= 0; --j)
                        if (j < chain.n && j >= k) xform_ray(sc, chain.id[j], ok, dk);
                    front_face = dot(dk, n) < 0.0f;
                    n = front_face ? n : -n;
                }
            }
        }
    }
    if (deep_n) {
        for (uint32_t k = 0; k < deep_n; ++k) {
            const uint32_t x = sc.xf_meta[deep_p0 + deep_n - 1u - k].x;
            const float4 q = sc.xf_param[x];
            if (sc.xf_meta[x].x == 0u) {
                p = p + v3(q.x, q.y, q.z);
            } else {
                const float sin_theta = q.x, cos_theta = q.y;
                const float px = cos_theta * p.x + sin_theta * p.z, pz = -sin_theta * p.x + cos_theta * p.z;
                const float nx = cos_theta * n.x + sin_theta * n.z, nz = -sin_theta * n.x + cos_theta * n.z;
                p.x = px, p.z = pz, n.x = nx, n.z = nz;
                V3 dk = wd, ok = wo;
                for (uint32_t j = 0; j < deep_n - k; ++j) xform_ray(sc, sc.xf_meta[deep_p0 + j].x, ok, dk);
                front_face = dot(dk, n) < 0.0f;
                n = front_face ? n : -n;
            }
        }
    }
    fs.n = is_medium ? splat(0.0f) : n;
    const uint32_t type = __float_as_uint(r1.x);
    const uint32_t TEX0_USERS = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 5) | (1u << 6) | (1u << 7) | (1u << 8) | (1u << 9) | (1u << 10) | (1u << 11);
    V3 a = splat(0.0f); // an unknown tag
    if (type < 32u && ((TEX0_USERS >> type) & 1u)) {
        uint32_t n_fetch = 0u; // (the render's fetch statistics are not this kernel's)
        a = texture_value_inline(sc, pt, __float_as_uint(r1.y), __float_as_uint(r1.z), rec[3].z, v3(r2.x, r2.y, r2.z), __float_as_uint(rec[3].w), on,
                                 is_rect || is_planar, rect_uv, p, n_fetch);
    } else if (type == 3u) {
        a = v3(r2.x, r2.y, r2.z);
    } else if (type == 4u || type == 12u) {
        a = splat(1.0f);
    }
    fs.a = v3(feature_clamp01(a.x), feature_clamp01(a.y), feature_clamp01(a.z));
    return fs;
}

struct FeatureArgs {
    uint4* plane;        // the four quarter planes, local pixel order (rt_features_plan.h)
    const uint8_t* flag; // the converged flags of an adaptive add, local pixel order, or NULL
    uint32_t s_first;    // the absolute index of the window's first contributing sample
    uint32_t n_feat;     // how many contribute (> 0), `stride` apart
    uint32_t stride;
    GenMotion motion;    // MOTION
    GenPlanar planar;    // PLANAR
};

// Waves per SIMD the kernel is bounded to: 8 = two workgroups of RT_BVH_BLOCK per CU wherever the LDS of the search state admits two, as
// k_intersect: 64 VGPRs and 124 to 140 B of scratch per lane.  4 = one workgroup per CU, 104 to 112 VGPRs and no scratch: a build with
// -DRT_FEATURES_WAVES=4 gives the same bits; DESIGN.md 4.18 has both timed (8 is cheaper on sphere_scene, dearer on cornell_box).
#ifndef RT_FEATURES_WAVES
#define RT_FEATURES_WAVES 8
#endif
constexpr uint32_t RT_FEATURES_BLOCK_X = 32u, RT_FEATURES_BLOCK_Y = RT_BVH_BLOCK / 32u;

// `gp`: the GenParams of the frame (s0, n_rays and cap are not read); `gl` is read by LENS only.
template <bool USE_BVH, bool LDS_NODES, bool MOTION, bool PLANAR, bool LENS>
__global__ __launch_bounds__(RT_BVH_BLOCK, RT_FEATURES_WAVES) void k_features(DevScene sc, GenParams gp, GenLens gl, FeatureArgs fa) {
    constexpr int BLOCK = RT_BVH_BLOCK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t t = threadIdx.x;
    const uint32_t pi = blockIdx.x * RT_FEATURES_BLOCK_X + (t & 31u), pj = blockIdx.y * RT_FEATURES_BLOCK_Y + (t >> 5);
    const bool mine = pi < gp.nx && pj < gp.npix / gp.nx;
    const uint32_t lp = mine ? local_of_pixel(gp.nx, gp.tiles_per_row, gp.tile_pixels, pi, pj) : 0u;
    const bool active = mine && !(fa.flag && fa.flag[lp] != 0u);
    const float4* dc = MOTION ? fa.motion.sph_dc : nullptr;
    const PerlinTables pt{sc.perlin_vec, sc.perlin_perm2};

    BvhLds L;
    if (USE_BVH) {
        L = stage_bvh<BLOCK, LDS_NODES>(sc, smem);
        if (MOTION) L.dc = dc;
        if (PLANAR) L.dc = nullptr, L.pq = fa.planar.pq, L.pbase = fa.planar.base;
        __syncthreads();
    }

    uint4* q = fa.plane + lp;
    const size_t qs = gp.npix; // quarter k lies k * npix elements behind quarter 0
    float4 qa = make_float4(0.f, 0.f, 0.f, 0.f), qn = qa;
    double2 m0 = make_double2(0.0, 0.0), m1 = m0;
    if (active) {
        qa = *reinterpret_cast<const float4*>(q), qn = *reinterpret_cast<const float4*>(q + qs);
        m0 = *reinterpret_cast<const double2*>(q + 2 * qs), m1 = *reinterpret_cast<const double2*>(q + 3 * qs);
    }
    uint32_t n_f = __float_as_uint(qa.w), n_h = __float_as_uint(qn.w);

    GenParams g = gp;
    for (uint32_t k = 0; k < fa.n_feat; ++k) {
        g.s0 = fa.s_first + k * fa.stride;
        V3 o = splat(0.0f), d = v3(0.f, 0.f, 1.f);
        uint32_t k0 = 0u, k1 = 0u;
        if (active) gen_primary<LENS>(g, gl, lp, o, d, k0, k1);
        const float tm = MOTION && active ? path_time(fa.motion, k0, k1) : 0.0f;
        float tbest = RT_FLT_MAX;
        int hit = -1;
        const float a = length_squared(d);
        const MediumCtx mc{k0, k1, depth_counter_base(0)};
        if (USE_BVH) {
            if (active && (PLANAR || sc.n_prims)) {
                const float ix = 1.0f / d.x, iy = 1.0f / d.y, iz = 1.0f / d.z;
                const float nox = -(o.x * ix), noy = -(o.y * iy), noz = -(o.z * iz);
                float eps = 2.4e-7f * fmaxf(fmaxf(fabsf(nox), fabsf(noy)), fabsf(noz));
                const bool exact = !(eps <= sc.bvh_exact_eps);
                if (exact) eps = 0.0f;
                int cur = 0, sp = 0;
                uint32_t pend = 0u;
                while (!bvh_step<BLOCK, true, false, true, MOTION, PLANAR>(L, o, d, ix, iy, iz, nox, noy, noz, eps, exact, a, pend, cur, sp, tbest, hit, nullptr, tm)) {
                }
                while (pend && !media_step<true>(L, o, d, mc, sc.n_media, pend, tbest, hit)) {
                }
            }
        } else {
            if (PLANAR || sc.n_xforms || sc.n_media) {
                closest_hit_spheres_general<MOTION>(sc, o, d, tbest, hit, dc, tm);
            } else {
                float4* s_geo = reinterpret_cast<float4*>(smem);
                for (uint32_t t0 = 0; t0 < sc.n_spheres; t0 += RT_SPHERE_TILE) {
                    const uint32_t nn = min(RT_SPHERE_TILE, sc.n_spheres - t0);
                    __syncthreads();
                    for (uint32_t j = t; j < nn; j += BLOCK) s_geo[j] = sc.sph_geo[t0 + j];
                    __syncthreads();
                    closest_hit_tile<MOTION>(s_geo, nn, t0, o, d, a, tbest, hit, dc, tm);
                }
            }
            closest_hit_rects(sc, o, d, mc, tbest, hit);
            if (PLANAR) closest_hit_planar(fa.planar, o, d, tbest, hit);
        }
        if (!active) continue;
        const FeatureSample fs = first_hit_surface<MOTION, PLANAR>(sc, pt, o, d, hit, tbest, dc, tm, PLANAR ? fa.planar.pq : nullptr, PLANAR ? fa.planar.base : 0u);
        qa.x += fs.a.x, qa.y += fs.a.y, qa.z += fs.a.z;
        qn.x += fs.n.x, qn.y += fs.n.y, qn.z += fs.n.z;
        ++n_f;
        const double ax = (double)fs.a.x, ay = (double)fs.a.y, az = (double)fs.a.z;
        const double nx = (double)fs.n.x, ny = (double)fs.n.y, nz = (double)fs.n.z;
        m0.x += (ax * ax + ay * ay) + az * az;
        m0.y += (nx * nx + ny * ny) + nz * nz;
        if (fs.hit) {
            const double z = (double)fs.z;
            ++n_h;
            m1.x += z;
            m1.y += z * z;
        }
    }
    if (!active) return;
    qa.w = __uint_as_float(n_f), qn.w = __uint_as_float(n_h);
    *reinterpret_cast<float4*>(q) = qa, *reinterpret_cast<float4*>(q + qs) = qn;
    *reinterpret_cast<double2*>(q + 2 * qs) = m0, *reinterpret_cast<double2*>(q + 3 * qs) = m1;
}

// Variance of the mean from (sum of squares, squared sum, count), as the header states it; 0 below two samples.
__device__ __forceinline__ float feature_var_of_mean(double s2, double sq, uint32_t count) {
    if (count < 2u) return 0.0f;
    const double n = (double)count;
    const double v = (s2 - sq / n) / (n - 1.0);
    return (float)((v < 0.0 ? 0.0 : v) / n);
}

// rt_accum_read_features: one thread per pixel in image order; `out` holds the five outputs one behind the other (albedo 3, normal 3,
// depth 1, hit 1, var 3 floats per pixel: rt_features_plan.h).
__global__ __launch_bounds__(256) void k_features_read(const uint4* __restrict__ plane, float* __restrict__ out, uint32_t nx, uint32_t rows,
                                                       uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const size_t npix = (size_t)nx * rows;
    if (p >= npix) return;
    const uint4* q = plane + local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    const float4 qa = *reinterpret_cast<const float4*>(q), qn = *reinterpret_cast<const float4*>(q + npix);
    const double2 m0 = *reinterpret_cast<const double2*>(q + 2 * npix), m1 = *reinterpret_cast<const double2*>(q + 3 * npix);
    const uint32_t n_f = __float_as_uint(qa.w), n_h = __float_as_uint(qn.w);
    const float N = (float)n_f;
    float* o_a = out + 3 * (size_t)p;
    float* o_n = out + 3 * npix + 3 * (size_t)p;
    float* o_v = out + 8 * npix + 3 * (size_t)p;
    o_a[0] = n_f ? qa.x / N : 0.0f, o_a[1] = n_f ? qa.y / N : 0.0f, o_a[2] = n_f ? qa.z / N : 0.0f;
    o_n[0] = n_f ? qn.x / N : 0.0f, o_n[1] = n_f ? qn.y / N : 0.0f, o_n[2] = n_f ? qn.z / N : 0.0f;
    out[6 * npix + p] = n_h ? (float)(m1.x / (double)n_h) : 0.0f;
    out[7 * npix + p] = n_f ? (float)n_h / N : 0.0f;
    const double sa = ((double)qa.x * (double)qa.x + (double)qa.y * (double)qa.y) + (double)qa.z * (double)qa.z;
    const double sn = ((double)qn.x * (double)qn.x + (double)qn.y * (double)qn.y) + (double)qn.z * (double)qn.z;
    o_v[0] = feature_var_of_mean(m0.x, sa, n_f);
    o_v[1] = feature_var_of_mean(m0.y, sn, n_f);
    o_v[2] = feature_var_of_mean(m1.y, m1.x * m1.x, n_h);
}

// ---- the feature-guided filter (rtow_mi355x.h "The feature-guided filter") ----------------------------------------------------------------
// Its inputs beside (c, y, v), which k_denoise_inputs makes: fmean [7 npix] and fvar [3 npix] in image order, from the records.
__global__ __launch_bounds__(256) void k_features_inputs(const uint4* __restrict__ plane, float* __restrict__ fmean, float* __restrict__ fvar, uint32_t nx,
                                                         uint32_t rows, uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const size_t npix = (size_t)nx * rows;
    if (p >= npix) return;
    const uint4* q = plane + local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    const float4 qa = *reinterpret_cast<const float4*>(q), qn = *reinterpret_cast<const float4*>(q + npix);
    const double2 m0 = *reinterpret_cast<const double2*>(q + 2 * npix), m1 = *reinterpret_cast<const double2*>(q + 3 * npix);
    const uint32_t n_f = __float_as_uint(qa.w), n_h = __float_as_uint(qn.w);
    float* fm = fmean + 7 * (size_t)p;
    float* fv = fvar + 3 * (size_t)p;
    if (n_f < 2u) { // no variance: the pixel stays what it is and spreads to no other
        const float none = __uint_as_float(0x7FC00000u);
        for (int k = 0; k < 7; ++k) fm[k] = none;
        fv[0] = fv[1] = fv[2] = none;
        return;
    }
    const float N = (float)n_f;
    fm[0] = qa.x / N, fm[1] = qa.y / N, fm[2] = qa.z / N;
    fm[3] = qn.x / N, fm[4] = qn.y / N, fm[5] = qn.z / N;
    fm[6] = n_h ? (float)(m1.x / (double)n_h) : 0.0f;
    const double sa = ((double)qa.x * (double)qa.x + (double)qa.y * (double)qa.y) + (double)qa.z * (double)qa.z;
    const double sn = ((double)qn.x * (double)qn.x + (double)qn.y * (double)qn.y) + (double)qn.z * (double)qn.z;
    fv[0] = feature_var_of_mean(m0.x, sa, n_f);
    fv[1] = feature_var_of_mean(m0.y, sn, n_f);
    fv[2] = feature_var_of_mean(m1.y, m1.x * m1.x, n_h);
}

// a' of the header: the albedo a colour is divided by and multiplied back with
__device__ __forceinline__ float demodulation_albedo(float abar) { return abar > 0.015625f ? abar : 0.015625f; }

// Demodulation, in place on the filter's inputs in image order: c / a', y / Ya, v / (Ya Ya).
__global__ __launch_bounds__(256) void k_features_demodulate(float* __restrict__ c, float2* __restrict__ yv, const float* __restrict__ fmean, uint32_t npix) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    const float* fm = fmean + 7 * (size_t)p;
    const float ar = demodulation_albedo(fm[0]), ag = demodulation_albedo(fm[1]), ab = demodulation_albedo(fm[2]);
    const float Ya = (0.2126f * ar + 0.7152f * ag) + 0.0722f * ab;
    float* cp = c + 3 * (size_t)p;
    cp[0] = cp[0] / ar, cp[1] = cp[1] / ag, cp[2] = cp[2] / ab;
    const float2 g = yv[p];
    yv[p] = make_float2(g.x / Ya, g.y / (Ya * Ya));
}

struct FeatureGuideArgs {
    float k2[3];   // k_f * k_f: albedo, normal, depth
    float tau[3];
    uint32_t use, demodulate;
};

// d_f of the header for one feature: s2 = |f_p - f_q|^2, (vp, vq) the variances of the mean, k2 = k_f k_f
__device__ __forceinline__ float feature_distance(float s2, float vp, float vq, float floor, float k2) {
    const float vmin = vq < vp ? vq : vp;
    const float vs = vp + vq;
    const float vmax = vs > floor ? vs : floor;
    return (s2 - (vp + vmin)) / (1e-10f + k2 * vmax);
}

// The body of nlm_filter<F, GuideLuminance> (rt_denoise.h: the tile, the shared map of the colour patch distance, the order of every
// operation) with the pointwise feature distances of the pair (p, q) beside D_c.  A body of its own, so that k_denoise<F>,
// k_denoise_channels<F> and k_denoise_multi keep their bytes; with use == 0 and no demodulation it performs nlm_filter's operations on
// nlm_filter's operands in nlm_filter's order.  fmean, fvar: image order, read from global memory (the 9 x 9 .. 21 x 21 window of a
// workgroup's pixels stays in L1 / L2).  Grid, block and dynamic LDS as k_denoise<F>.
template <int F>
__global__ __launch_bounds__(256) void k_denoise_features(const float* __restrict__ c, const float2* __restrict__ g, const float* __restrict__ fmean,
                                                          const float* __restrict__ fvar, float* __restrict__ out, uint32_t nx, uint32_t rows, int R, float k2,
                                                          FeatureGuideArgs fg) {
    extern __shared__ float2 dn_tile[];
    constexpr int T = (int)RT_DN_TILE, TP = (int)RT_DN_PITCH, MP = (int)RT_DN_MAP_PITCH;
    constexpr int E = T + 2 * F;
    const int H = R + F;
    const int side = T + 2 * H;
    const int plane = TP * side;
    float* const dmap = reinterpret_cast<float*>(dn_tile + plane);
    const int x0 = (int)(blockIdx.x * RT_DN_TILE) - H, y0 = (int)(blockIdx.y * RT_DN_TILE) - H;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int tid = ty * T + tx;
    for (int e = tid; e < side * side; e += 256) {
        const int ly = e / side, lx = e - ly * side;
        const int gx = min(max(x0 + lx, 0), (int)nx - 1), gy = min(max(y0 + ly, 0), (int)rows - 1);
        dn_tile[ly * TP + lx] = g[(size_t)gy * nx + gx];
    }
    __syncthreads();
    const int px = (int)(blockIdx.x * RT_DN_TILE) + tx, py = (int)(blockIdx.y * RT_DN_TILE) + ty;
    const bool live = px < (int)nx && py < (int)rows;
    const int m0y = tid / E, m0x = tid - m0y * E;
    const int e1 = tid + 256;
    const bool two = e1 < E * E;
    const int m1y = two ? e1 / E : 0, m1x = two ? e1 - m1y * E : 0;
    const float2* const a0p = dn_tile + (m0y + R) * TP + m0x + R;
    const float2* const a1p = dn_tile + (m1y + R) * TP + m1x + R;
    const float2 a0 = a0p[0], a1 = a1p[0];
    constexpr float cnt = (float)((2 * F + 1) * (2 * F + 1));
    // the features of p
    const size_t p = live ? (size_t)py * nx + px : 0u;
    float fp[7], vp[3];
#pragma unroll
    for (int k = 0; k < 7; ++k) fp[k] = fmean[7 * p + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) vp[k] = fvar[3 * p + k];
    const float floor_z = fg.tau[2] * (fp[6] * fp[6]);
    float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
    int buf = 0;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = py + dy;
        for (int dx = -R; dx <= R; ++dx, buf ^= 1) {
            float* const map = dmap + buf * (MP * E);
            const int off = dy * TP + dx;
            map[m0y * MP + m0x] = denoise_distance(a0, a0p[off], k2);
            if (two) map[m1y * MP + m1x] = denoise_distance(a1, a1p[off], k2);
            __syncthreads();
            const int qx = px + dx;
            if (!live || qy < 0 || qy >= (int)rows || qx < 0 || qx >= (int)nx) continue;
            const float* const mine = map + (ty + F) * MP + tx + F;
            float S = 0.0f;
            for (int oy = -F; oy <= F; ++oy) {
                float row = 0.0f;
                for (int ox = -F; ox <= F; ++ox) row = row + mine[oy * MP + ox];
                S = S + row;
            }
            const float D = S / cnt;
            float m = D < 0.0f ? 0.0f : D; // (a NaN stays one)
            bool bad = false;              // a used d_f is NaN
            const size_t q = (size_t)qy * nx + qx;
            if (fg.use) {
                const float* fq = fmean + 7 * q;
                const float* vq = fvar + 3 * q;
                if (fg.use & RT_FEATURE_USE_ALBEDO) {
                    const float ex = fp[0] - fq[0], ey = fp[1] - fq[1], ez = fp[2] - fq[2];
                    const float d = feature_distance((ex * ex + ey * ey) + ez * ez, vp[0], vq[0], fg.tau[0], fg.k2[0]);
                    bad = bad || d != d;
                    m = d > m ? d : m;
                }
                if (fg.use & RT_FEATURE_USE_NORMAL) {
                    const float ex = fp[3] - fq[3], ey = fp[4] - fq[4], ez = fp[5] - fq[5];
                    const float d = feature_distance((ex * ex + ey * ey) + ez * ez, vp[1], vq[1], fg.tau[1], fg.k2[1]);
                    bad = bad || d != d;
                    m = d > m ? d : m;
                }
                if (fg.use & RT_FEATURE_USE_DEPTH) {
                    const float ez = fp[6] - fq[6];
                    const float d = feature_distance(ez * ez, vp[2], vq[2], floor_z, fg.k2[2]);
                    bad = bad || d != d;
                    m = d > m ? d : m;
                }
            }
            float u = 1.0f - 0.25f * m;
            u = u > 0.0f ? u : 0.0f; // (a NaN becomes 0)
            if (bad) u = 0.0f;
            if (u != 0.0f) {
                const float w = (u * u) * (u * u);
                den = den + w;
                const float* cq = c + 3 * q;
                nr = nr + w * cq[0], ng = ng + w * cq[1], nb = nb + w * cq[2];
            }
        }
    }
    if (!live) return;
    float r = c[3 * p], gr = c[3 * p + 1], b = c[3 * p + 2]; // den == 0: p stays what it is
    if (den != 0.0f) r = nr / den, gr = ng / den, b = nb / den;
    if (fg.demodulate) r = r * demodulation_albedo(fp[0]), gr = gr * demodulation_albedo(fp[1]), b = b * demodulation_albedo(fp[2]);
    out[3 * p] = r, out[3 * p + 1] = gr, out[3 * p + 2] = b;
}

} // namespace rt
