// rt_scene_prep.h — host-side preparation of everything rt_scene_upload and the rt_set_* calls hand to the device.
//
// Every index, count, offset and bound the kernels trust without checking is made here: entry ids, medium boundary lists, listed
// wrapper chains, tree leaves, class keys, texel offsets, swept bounds, plane set-ups.  Like rt_bvh.h this is host arithmetic only: no
// context, no device call, no error state but a code and a message.  A prepare_* function validates its input, computes into its
// output struct and touches nothing else, so rt_api.hip runs it BEFORE it synchronises or writes anything (a refusal leaves device and
// context as they were), and tests/scene_prep_main.hip runs the same code under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x_debug.h"
#include "rt_kernels.h"
#include "rt_bvh.h"
#include "rt_grid.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace rt {

inline float fbits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// f32 below / above a double
inline float round_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafterf(f, -FLT_MAX);
    return f;
}
inline float round_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafterf(f, FLT_MAX);
    return f;
}

inline bool mat_needs_tex0(uint32_t t) {
    return t == RT_MAT_EMISSION || t == RT_MAT_DIFFUSE || t == RT_MAT_LAMBERT || t == RT_MAT_ISOTROPIC ||
           t == RT_MAT_OREN_NAYAR || t == RT_MAT_BURLEY_DIFFUSE || t == RT_MAT_ROUGH_PLASTIC ||
           t == RT_MAT_DISNEY_DIFFUSE || t == RT_MAT_DISNEY_METAL || t == RT_MAT_DISNEY_SHEEN;
}

// The cheap shading classes (1 + material*4 + texture of tex0; 0 = miss): no hit under the gradient / black sky, and
// the material.rs materials over a ConstantTex (Metal and Dielectric have no texture).
inline bool class_is_light(uint32_t cls, uint32_t sky_type) {
    if (cls == 0) return sky_type != RT_SKY_ENV;
    const uint32_t ty = (cls - 1u) / 4u, tt = (cls - 1u) % 4u;
    return tt == RT_TEX_CONSTANT && ty <= RT_MAT_ISOTROPIC;
}

// Sort keys of k_shade's class sort: the classes present (a miss always is) ranked cheap classes first (a miss and the
// constant-texture material.rs materials, then the textured and pbr.rs ones), so that the long Perlin / PBR segments of a block sit
// together at its end.  Raw classes in, keys out; returns the key of a miss.
inline uint32_t rank_classes(std::vector<uint8_t>& cls, uint32_t sky_type) {
    bool class_present[RT_NCLASS] = {};
    class_present[0] = true;
    for (uint8_t c : cls) class_present[c] = true;
    uint32_t class_key[RT_NCLASS] = {}, n_keys = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t c = 0; c < RT_NCLASS; ++c)
            if (class_present[c] && class_is_light(c, sky_type) == (pass == 0)) class_key[c] = n_keys++;
    for (uint8_t& c : cls) c = (uint8_t)class_key[c];
    return class_key[0];
}

// The shading record (5 float4 at `rec`) of a world entry with material m and geometry (geo0, geo1); returns its raw class
// (1 + material * 4 + texture of tex0, < RT_NCLASS).
inline uint8_t shading_record(const MatRec& m, const std::vector<TexRec>& texs, float4 geo0, float4 geo1, float4* rec) {
    const bool has_t0 = mat_needs_tex0(m.type) && m.tex0 < texs.size();
    const TexRec t0 = has_t0 ? texs[m.tex0] : TexRec{};
    rec[0] = geo0;
    rec[1] = make_float4(fbits(m.type), fbits(t0.type), fbits(t0.aux), fbits(m.tex1));
    // colour slot: the texture's colour 0 for textured materials, the albedo for Metal
    rec[2] = has_t0 ? make_float4(t0.c0r, t0.c0g, t0.c0b, m.p0) : make_float4(m.cr, m.cg, m.cb, m.p0);
    rec[3] = make_float4(m.p1, m.p2, t0.scale, fbits(m.tex0));
    rec[4] = geo1;
    return (uint8_t)(1u + m.type * 4u + t0.type);
}

// The tree over a set of world entries as the kernels read it, and what the host decides by.
struct HostTree {
    HostBvh4 bvh4;
    uint32_t depth = 0;     // of the binary tree it was collapsed from (configure_search holds it against RT_BVH_MAX_DEPTH)
    float exact_eps = 0.0f; // DevScene::bvh_exact_eps
};
inline void build_tree(const std::vector<PrimBox>& eboxes, const std::vector<uint32_t>& entry_ids, HostTree& t) {
    HostBvh bvh;
    build_prim_bvh(eboxes, RT_BVH_MAX_DEPTH, bvh);
    for (auto& dd : bvh.d) { // leaf ids: index into eboxes -> world entry id
        if (dd.x < 0 && dd.x != INT_MIN) dd.x = ~(int)entry_ids[(size_t)~dd.x];
        if (dd.y < 0 && dd.y != INT_MIN) dd.y = ~(int)entry_ids[(size_t)~dd.y];
    }
    collapse_bvh4(bvh, t.bvh4);
    t.depth = bvh.depth;
    // rays whose slab slack exceeds 2^-10 of the scene extent use the cancellation-free slab test (bvh_step)
    double ext2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        float lo = FLT_MAX, hi = -FLT_MAX;
        for (const PrimBox& b : eboxes) lo = std::min(lo, b.mn[k]), hi = std::max(hi, b.mx[k]);
        if (hi > lo) ext2 += ((double)hi - lo) * ((double)hi - lo);
    }
    t.exact_eps = (float)(std::sqrt(ext2) / 1024.0);
}

// World-space bounds the closest-hit search culls with, from a validated scene: rt_scene_upload builds the tree over `ent` and
// k_primary_lists tests `ent_bs`; rt_debug_world_bounds hands the same arrays to the tests.
struct WorldBounds {
    std::vector<PrimBox> prim;        // per primitive (spheres, then rectangles), world space, before the tree's pad
    std::vector<float4> world_sphere; // per sphere: world centre and radius of an instanced sphere (bare: its own)
    std::vector<uint32_t> pxf, pmed;  // per primitive: innermost wrapper, medium
    std::vector<PrimBox> ent;         // world entries: primitives that are not a medium boundary, then the media
    std::vector<uint32_t> entry_ids;  // their ids (primitive i, or n_prims + medium m)
    std::vector<float4> ent_bs;       // their bounding spheres
};

// Grows `box` (and `*ws`, a sphere's world sphere) to contain the region primitive i covers in world space under the exact ray map of
// its chain.  The kernels map a world ray outermost wrapper first: Translate o -= q (hitable.rs:411), RotateY (x, z) -> (c x - s z,
// s x + c z) (hitable.rs:483-492) with the STORED f32 s = sin, c = cos.  Those c, s lie off the unit circle (s2 = c^2 + s^2 = 1 +- 8e-8):
// the exact inverse of a RotateY level is (x, z) -> (c x + s z, -s x + c z) / s2, and it scales x and z by 1 / sqrt(s2).  So an object
// point goes to the world innermost wrapper first through these inverses, a rectangle's region is the hull of its four mapped corners,
// and a sphere's the ellipsoid around its mapped centre with semi-axes r / S (x, z) and r (y), S = the product of sqrt(s2).
// Error model: all of this runs in double.  A level rounds at most 6 times (s2: two; the rotation: two products, a sum, a quotient; a
// Translate: one sum), each by 2^-53 of a value below 2 M, M = the largest magnitude any point takes on the way, and carries the error of
// the levels inside it scaled by 1 / sqrt(s2) < 1 + 1e-7: n levels err by less than 16 n 2^-53 M, and S by 4 n 2^-53 of itself.  The
// bound is widened by that and rounded outward to f32.
// The kernels take the same map in f32, so the ray they test lies off the exact one, and the hit they report sits off the exact region
// along the world ray: a box that held the exact region only would let the tree cull a primitive whose f32 root comes before the
// box, behind the root of another primitive it already has (two hits a rounding apart, both real in exact arithmetic).  Error model
// of the f32 map, for a ray whose origin at every level is no larger than M_l, the largest magnitude the primitive's own points take
// at that level (a ray that starts among the primitives of the chain, or nearer the origin of each frame): a Translate rounds o - q
// once, 2^-24 M_l per coordinate; a RotateY rounds two products and a sum of origin and of direction, 4 2^-24 M_l for the origin and
// 4 2^-24 of the direction, which the root t carries over a distance below 2 M_l: 12 2^-24 M_l.  Later levels move these errors
// without growing them (1 / sqrt(s2) < 1 + 1e-7), so the object-space hit lies within sqrt(3) 2^-24 sum_l c_l M_l of the primitive
// (c = 1 per Translate, 12 per RotateY), and its world point within that over S.  The box is widened by this too.  A ray from
// farther out errs in proportion to its distance; the tree's relative widening of the far plane (4e-6, rt_kernels.h) covers chains up
// to sum c_l ~ 60 of it, and beyond, two real hits a rounding apart may come out in either order (rtow_mi355x_debug.h).
inline void exact_world_region(const RtFlatScene* s, uint32_t i, PrimBox& box, float4* ws) {
    const uint32_t x0 = i < s->n_spheres ? s->sph_xform[i] : s->rect_xform[i - s->n_spheres];
    double pts[4][3];
    int np = 1;
    double r = 0.0;
    if (i < s->n_spheres) {
        pts[0][0] = s->sph_cx[i], pts[0][1] = s->sph_cy[i], pts[0][2] = s->sph_cz[i];
        r = std::fabs((double)s->sph_r[i]);
    } else {
        const uint32_t j = i - s->n_spheres, ax = s->rect_axis[j];
        const float* mn = s->rect_min + 3 * (size_t)j;
        const float* mx = s->rect_max + 3 * (size_t)j;
        const int ua = ax == 0 ? 1 : 0, va = ax == 2 ? 1 : 2;
        np = 4;
        for (int c = 0; c < 4; ++c) {
            pts[c][ax] = mn[ax]; // the plane the hit test uses (hitable.rs:253)
            pts[c][ua] = (c & 1) ? mx[ua] : mn[ua];
            pts[c][va] = (c & 2) ? mx[va] : mn[va];
        }
    }
    double mag = r, S = 1.0, f32_map = 0.0; // f32_map: sum_l c_l M_l
    uint32_t n = 0;
    for (int c = 0; c < np; ++c)
        for (int k = 0; k < 3; ++k) mag = std::max(mag, std::fabs(pts[c][k]));
    for (uint32_t x = x0; x != RT_NO_XFORM; x = s->xf_parent[x], ++n) {
        const float* q = s->xf_param + 4 * (size_t)x;
        const double sn = q[0], cs = q[1], s2 = cs * cs + sn * sn;
        if (s->xf_type[x] == RT_XF_ROTATE_Y) S *= std::sqrt(s2);
        double level_mag = r; // M_l: the points' magnitude on both sides of this level
        for (int c = 0; c < np; ++c)
            for (int k = 0; k < 3; ++k) level_mag = std::max(level_mag, std::fabs(pts[c][k]) + r);
        for (int c = 0; c < np; ++c) {
            double* p = pts[c];
            if (s->xf_type[x] == RT_XF_TRANSLATE) {
                for (int k = 0; k < 3; ++k) p[k] += (double)q[k];
            } else {
                const double px = p[0], pz = p[2];
                p[0] = (cs * px + sn * pz) / s2, p[2] = (-sn * px + cs * pz) / s2;
            }
            for (int k = 0; k < 3; ++k) mag = std::max(mag, std::fabs(p[k])), level_mag = std::max(level_mag, std::fabs(p[k]) + r);
        }
        f32_map += (s->xf_type[x] == RT_XF_ROTATE_Y ? 12.0 : 1.0) * level_mag;
    }
    const double ulp = std::ldexp(1.0, -53);
    const double half[3] = {r / S * (1.0 + 4.0 * n * ulp), r, r / S * (1.0 + 4.0 * n * ulp)}; // (0 for a rectangle)
    const double e = 16.0 * (n + 1) * ulp * mag + 1.7321 * std::ldexp(f32_map, -24) / std::min(S, 1.0) * (1.0 + 1e-6);
    for (int k = 0; k < 3; ++k) {
        double lo = pts[0][k], hi = pts[0][k];
        for (int c = 1; c < np; ++c) lo = std::min(lo, pts[c][k]), hi = std::max(hi, pts[c][k]);
        box.mn[k] = std::min(box.mn[k], round_down(lo - half[k] - e));
        box.mx[k] = std::max(box.mx[k], round_up(hi + half[k] + e));
    }
    if (ws) { // the world sphere keeps its centre and grows to hold the ellipsoid
        const double dx = pts[0][0] - ws->x, dy = pts[0][1] - ws->y, dz = pts[0][2] - ws->z;
        const double need = std::sqrt(dx * dx + dy * dy + dz * dz) + std::max(half[0], half[1]) + 2.0 * e;
        if (need > (double)ws->w) ws->w = round_up(need);
    }
}

inline void world_bounds(const RtFlatScene* s, WorldBounds& w) {
    const uint32_t n_prims = s->n_spheres + s->n_rects;
    w.prim.assign(n_prims, PrimBox{});
    w.world_sphere.assign(s->n_spheres, make_float4(0.f, 0.f, 0.f, 0.f));
    w.pxf.assign(n_prims, RT_NO_XFORM);
    w.pmed.assign(n_prims, RT_NO_MEDIUM);
    for (uint32_t i = 0; i < n_prims; ++i) {
        const bool sph = i < s->n_spheres;
        const uint32_t r = i - s->n_spheres;
        w.pxf[i] = sph ? (s->sph_xform ? s->sph_xform[i] : RT_NO_XFORM) : (s->rect_xform ? s->rect_xform[r] : RT_NO_XFORM);
        w.pmed[i] = sph ? (s->sph_medium ? s->sph_medium[i] : RT_NO_MEDIUM) : (s->rect_medium ? s->rect_medium[r] : RT_NO_MEDIUM);
    }
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const float c[3] = {s->sph_cx[i], s->sph_cy[i], s->sph_cz[i]};
        const float r = std::fabs(s->sph_r[i]);
        for (int k = 0; k < 3; ++k) w.prim[i].mn[k] = c[k] - r, w.prim[i].mx[k] = c[k] + r;
        w.world_sphere[i] = make_float4(c[0], c[1], c[2], r);
    }
    for (uint32_t i = 0; i < s->n_rects; ++i) {
        const uint32_t ax = s->rect_axis[i];
        const float* mn = s->rect_min + 3 * (size_t)i;
        const float* mx = s->rect_max + 3 * (size_t)i;
        PrimBox& b = w.prim[s->n_spheres + i];
        for (int k = 0; k < 3; ++k) b.mn[k] = std::min(mn[k], mx[k]), b.mx[k] = std::max(mn[k], mx[k]);
        b.mn[ax] = mn[ax] - 0.0001f, b.mx[ax] = mn[ax] + 0.0001f; // the plane the hit test uses (hitable.rs:253)
    }
    // wrapped primitives: world-space bounds through the chain.  Two bounds, and the box is their hull:
    //  * the float construction (corners through every wrapper from the inside out, as RotateY::new does at hitable.rs:455-473; the
    //    centre of a sphere through the forward rotation) with its margins.  It is kept as a floor: on the scenes it was made for the
    //    tree and the list walk agree bit for bit, and a smaller box would cull more fp32 false positives;
    //  * the region the primitive covers under the chain's exact ray map (exact_world_region below).
    // What the exact map misses and fp32 hits is a false positive of the wrapper transform: a box may cull it (rtow_mi355x_debug.h).
    for (uint32_t i = 0; i < n_prims; ++i) {
        const uint32_t x0 = w.pxf[i];
        if (x0 == RT_NO_XFORM) continue;
        if (i < s->n_spheres) {
            // A sphere below Translate / RotateY wrappers is still a sphere: its world box is centre' +- r, not the
            // box of the rotated box that RotateY::new computes (22 % wider per axis at 15 degrees, and the cloud of
            // final_scene is 1 000 overlapping instanced spheres).  The exact test runs in object space on a ray
            // whose transform rounds at the magnitude of the WORLD coordinates, so the box gets that slack.
            double c[3] = {s->sph_cx[i], s->sph_cy[i], s->sph_cz[i]}, mag = std::fabs((double)s->sph_r[i]);
            for (uint32_t x = x0; x != RT_NO_XFORM; x = s->xf_parent[x]) {
                const float* q = s->xf_param + 4 * (size_t)x;
                for (int k = 0; k < 3; ++k) mag = std::max(mag, std::fabs(c[k]));
                if (s->xf_type[x] == RT_XF_TRANSLATE) {
                    for (int k = 0; k < 3; ++k) c[k] += (double)q[k];
                } else {
                    const double sn = q[0], cs = q[1], cx = c[0], cz = c[2];
                    c[0] = cs * cx + sn * cz, c[2] = -sn * cx + cs * cz;
                }
                for (int k = 0; k < 3; ++k) mag = std::max(mag, std::fabs(c[k]));
            }
            const double r = std::fabs((double)s->sph_r[i]), slack = 8e-6 * mag + 1e-30;
            for (int k = 0; k < 3; ++k) w.prim[i].mn[k] = (float)(c[k] - r - slack), w.prim[i].mx[k] = (float)(c[k] + r + slack);
            w.world_sphere[i] = make_float4((float)c[0], (float)c[1], (float)c[2], (float)(r + 2.0 * slack));
            exact_world_region(s, i, w.prim[i], &w.world_sphere[i]);
            continue;
        }
        PrimBox& b = w.prim[i];
        for (uint32_t x = x0; x != RT_NO_XFORM; x = s->xf_parent[x]) {
            const float* q = s->xf_param + 4 * (size_t)x;
            if (s->xf_type[x] == RT_XF_TRANSLATE) {
                for (int k = 0; k < 3; ++k) b.mn[k] += q[k], b.mx[k] += q[k];
            } else {
                const float sn = q[0], cs = q[1];
                float mn[3] = {FLT_MAX, b.mn[1], FLT_MAX}, mx[3] = {-FLT_MAX, b.mx[1], -FLT_MAX};
                for (int ci = 0; ci < 4; ++ci) {
                    const float x0c = (ci & 1) ? b.mx[0] : b.mn[0], z0c = (ci & 2) ? b.mx[2] : b.mn[2];
                    const float nx = cs * x0c + sn * z0c, nz = -sn * x0c + cs * z0c;
                    mn[0] = std::min(mn[0], nx), mx[0] = std::max(mx[0], nx);
                    mn[2] = std::min(mn[2], nz), mx[2] = std::max(mx[2], nz);
                }
                // the rotation itself rounds: widen by a few ulp of the coordinate magnitude
                for (int k = 0; k < 3; k += 2) {
                    const float e = 1e-6f * std::max(std::fabs(mn[k]), std::fabs(mx[k]));
                    b.mn[k] = mn[k] - e, b.mx[k] = mx[k] + e;
                }
            }
        }
        exact_world_region(s, i, b, nullptr);
    }
    // world entries: the primitives that are not a medium boundary, then the media (the box around their boundaries)
    w.ent.clear(), w.entry_ids.clear();
    for (uint32_t i = 0; i < n_prims; ++i)
        if (w.pmed[i] == RT_NO_MEDIUM) w.ent.push_back(w.prim[i]), w.entry_ids.push_back(i);
    for (uint32_t m = 0; m < s->n_media; ++m) {
        PrimBox mb;
        for (int k = 0; k < 3; ++k) mb.mn[k] = FLT_MAX, mb.mx[k] = -FLT_MAX;
        for (uint32_t i = 0; i < n_prims; ++i)
            if (w.pmed[i] == m)
                for (int k = 0; k < 3; ++k) mb.mn[k] = std::min(mb.mn[k], w.prim[i].mn[k]), mb.mx[k] = std::max(mb.mx[k], w.prim[i].mx[k]);
        w.ent.push_back(mb);
        w.entry_ids.push_back(n_prims + m);
    }
    // bounding spheres of the world entries (k_primary_lists): a sphere gets its world sphere, anything else the sphere
    // around its world-space box
    w.ent_bs.assign(w.ent.size(), make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t e = 0; e < w.ent.size(); ++e) {
        const uint32_t id = w.entry_ids[e];
        if (id < s->n_spheres) {
            w.ent_bs[e] = w.world_sphere[id];
        } else {
            const PrimBox& b = w.ent[e];
            const double hx = 0.5 * ((double)b.mx[0] - b.mn[0]), hy = 0.5 * ((double)b.mx[1] - b.mn[1]), hz = 0.5 * ((double)b.mx[2] - b.mn[2]);
            float4 bs = make_float4((float)(0.5 * ((double)b.mx[0] + b.mn[0])), (float)(0.5 * ((double)b.mx[1] + b.mn[1])),
                                    (float)(0.5 * ((double)b.mx[2] + b.mn[2])), (float)(std::sqrt(hx * hx + hy * hy + hz * hz) * 1.0001));
            // far from the origin the rounded centre moves by more than the 1e-4: the sphere holds the box's corners from where it is
            double far2 = 0.0;
            for (int c = 0; c < 8; ++c) {
                const double dx = ((c & 1) ? b.mx[0] : b.mn[0]) - (double)bs.x, dy = ((c & 2) ? b.mx[1] : b.mn[1]) - (double)bs.y,
                             dz = ((c & 4) ? b.mx[2] : b.mn[2]) - (double)bs.z;
                far2 = std::max(far2, dx * dx + dy * dy + dz * dz);
            }
            if (std::sqrt(far2) > (double)bs.w) bs.w = round_up(std::sqrt(far2) * (1.0 + 1e-15));
            w.ent_bs[e] = bs;
        }
    }
}

inline bool sphere_is_finite(const RtFlatScene* s, uint32_t i) {
    return std::isfinite(s->sph_cx[i]) && std::isfinite(s->sph_cy[i]) && std::isfinite(s->sph_cz[i]) && std::isfinite(s->sph_r[i]);
}

// The geometry half of validate_scene: what world_bounds() reads, and all rt_debug_world_bounds asks of a scene.
inline int validate_geometry(const RtFlatScene* s, std::string& msg) {
    if (s->n_spheres && (!s->sph_cx || !s->sph_cy || !s->sph_cz || !s->sph_r)) return msg = "rt_scene_upload: sphere arrays missing", RT_ERR_INVALID;
    if (s->n_rects && (!s->rect_axis || !s->rect_min || !s->rect_max)) return msg = "rt_scene_upload: rectangle arrays missing", RT_ERR_INVALID;
    if (s->n_xforms && (!s->xf_type || !s->xf_param || !s->xf_parent)) return msg = "rt_scene_upload: transform arrays missing", RT_ERR_INVALID;
    // non-finite geometry would reach the tree builder's sort comparators and bin casts (host-side UB)
    for (uint32_t i = 0; i < s->n_spheres; ++i)
        if (!sphere_is_finite(s, i)) return msg = "rt_scene_upload: sphere " + std::to_string(i) + " has a centre or radius that is not finite", RT_ERR_INVALID;
    for (uint32_t i = 0; i < 3u * s->n_rects; ++i)
        if (!std::isfinite(s->rect_min[i]) || !std::isfinite(s->rect_max[i]))
            return msg = "rt_scene_upload: rectangle " + std::to_string(i / 3u) + " has a bound that is not finite", RT_ERR_INVALID;
    for (uint32_t i = 0; i < s->n_rects; ++i)
        if (s->rect_axis[i] > RT_RECT_XY) return msg = "rt_scene_upload: unknown rectangle axis", RT_ERR_INVALID;
    for (uint32_t i = 0; i < 4u * s->n_xforms; ++i)
        if (!std::isfinite(s->xf_param[i]))
            return msg = "rt_scene_upload: transform " + std::to_string(i / 4u) + " has a parameter that is not finite", RT_ERR_INVALID;
    for (uint32_t i = 0; i < s->n_xforms; ++i) {
        if (s->xf_type[i] > RT_XF_ROTATE_Y) return msg = "rt_scene_upload: unknown transform type", RT_ERR_INVALID;
        if (s->xf_parent[i] != RT_NO_XFORM && s->xf_parent[i] >= i)
            return msg = "rt_scene_upload: transform parent must precede its child", RT_ERR_INVALID;
    }
    // (a parent precedes its child, so every chain ends; its length is xf_depth below: any number of nested wrappers, hitable.rs:404-520)
    for (uint32_t i = 0; i < s->n_spheres && s->sph_xform; ++i)
        if (s->sph_xform[i] != RT_NO_XFORM && s->sph_xform[i] >= s->n_xforms) return msg = "rt_scene_upload: bad sphere transform chain", RT_ERR_INVALID;
    for (uint32_t i = 0; i < s->n_rects && s->rect_xform; ++i)
        if (s->rect_xform[i] != RT_NO_XFORM && s->rect_xform[i] >= s->n_xforms) return msg = "rt_scene_upload: bad rectangle transform chain", RT_ERR_INVALID;
    std::vector<uint8_t> bounded(s->n_media, 0); // a medium is the box around its boundary primitives: it has some
    for (uint32_t i = 0; i < s->n_spheres && s->sph_medium; ++i) {
        if (s->sph_medium[i] == RT_NO_MEDIUM) continue;
        if (s->sph_medium[i] >= s->n_media) return msg = "rt_scene_upload: bad sphere medium tag", RT_ERR_INVALID;
        bounded[s->sph_medium[i]] = 1;
    }
    for (uint32_t i = 0; i < s->n_rects && s->rect_medium; ++i) {
        if (s->rect_medium[i] == RT_NO_MEDIUM) continue;
        if (s->rect_medium[i] >= s->n_media) return msg = "rt_scene_upload: bad rectangle medium tag", RT_ERR_INVALID;
        bounded[s->rect_medium[i]] = 1;
    }
    for (uint32_t m = 0; m < s->n_media; ++m)
        if (!bounded[m]) return msg = "rt_scene_upload: medium " + std::to_string(m) + " has no boundary primitives", RT_ERR_INVALID;
    return RT_OK;
}

// What rt_scene_upload refuses before it touches anything: a code and the message (RT_OK: the scene is valid).  The geometry half runs
// first; a scene that breaks one rule gets that rule's code and message whichever half holds it.
inline int validate_scene(const RtFlatScene* s, std::string& msg) {
    if (const int rc = validate_geometry(s, msg)) return rc;
    if (s->n_spheres && !s->sph_mat) return msg = "rt_scene_upload: sphere arrays missing", RT_ERR_INVALID;
    if (s->n_rects && !s->rect_mat) return msg = "rt_scene_upload: rectangle arrays missing", RT_ERR_INVALID;
    if (s->n_materials && (!s->mat_type || !s->mat_color || !s->mat_p0 || !s->mat_p1 || !s->mat_p2 || !s->mat_p3 ||
                           !s->mat_tex0 || !s->mat_tex1))
        return msg = "rt_scene_upload: material arrays missing", RT_ERR_INVALID;
    if (s->n_textures && (!s->tex_type || !s->tex_color0 || !s->tex_color1 || !s->tex_scale || !s->tex_aux))
        return msg = "rt_scene_upload: texture arrays missing", RT_ERR_INVALID;
    if (s->n_perlin && (!s->perlin_vec || !s->perlin_perm))
        return msg = "rt_scene_upload: perlin tables missing", RT_ERR_INVALID;
    if (s->n_images && (!s->img_w || !s->img_h || !s->img_offset || !s->texels))
        return msg = "rt_scene_upload: image arrays missing", RT_ERR_INVALID;
    for (uint32_t i = 0; i < s->n_spheres; ++i)
        if (s->sph_mat[i] >= s->n_materials)
            return msg = "rt_scene_upload: sphere " + std::to_string(i) + " has material index out of range", RT_ERR_INVALID;
    if (s->n_media > RT_MAX_MEDIA) return msg = "rt_scene_upload: more than RT_MAX_MEDIA media", RT_ERR_UNSUPPORTED;
    if (s->n_media && (!s->med_neg_inv_density || !s->med_mat))
        return msg = "rt_scene_upload: medium arrays missing", RT_ERR_INVALID;
    for (uint32_t m = 0; m < s->n_media; ++m) {
        if (s->med_xform && s->med_xform[m] != RT_NO_XFORM && s->med_xform[m] >= s->n_xforms)
            return msg = "rt_scene_upload: bad wrapper around medium " + std::to_string(m), RT_ERR_INVALID;
        if (s->med_mat[m] >= s->n_materials) return msg = "rt_scene_upload: medium material out of range", RT_ERR_INVALID;
        const uint32_t mt = s->mat_type[s->med_mat[m]];
        // a medium writes neither uv nor tang (hitable.rs:574-576): materials that read them see stale record state
        if (mt == RT_MAT_DISNEY_METAL) return msg = "rt_scene_upload: DisneyMetal as a phase function reads a stale HitRecord.tang", RT_ERR_UNSUPPORTED;
        if (mat_needs_tex0(mt) && s->mat_tex0[s->med_mat[m]] < s->n_textures && s->tex_type[s->mat_tex0[s->med_mat[m]]] == RT_TEX_IMAGE)
            return msg = "rt_scene_upload: an image texture on a medium reads a stale HitRecord.uv", RT_ERR_UNSUPPORTED;
    }
    for (uint32_t i = 0; i < s->n_rects; ++i) {
        if (s->rect_mat[i] >= s->n_materials)
            return msg = "rt_scene_upload: rectangle " + std::to_string(i) + " has material index out of range", RT_ERR_INVALID;
        // DisneyMetal reads rec.tang, which a rectangle never writes (hitable.rs:262-269): the reference then uses
        // whatever an earlier candidate left in the record — not reproducible outside its traversal order
        if (s->mat_type[s->rect_mat[i]] == RT_MAT_DISNEY_METAL)
            return msg = "rt_scene_upload: DisneyMetal on a rectangle reads a stale HitRecord.tang in the reference", RT_ERR_UNSUPPORTED;
    }
    for (uint32_t m = 0; m < s->n_materials; ++m) {
        uint32_t t = s->mat_type[m];
        if (t >= RT_MAT__COUNT) return msg = "rt_scene_upload: unknown material type", RT_ERR_INVALID;
        if (mat_needs_tex0(t) && s->mat_tex0[m] >= s->n_textures)
            return msg = "rt_scene_upload: material " + std::to_string(m) + " needs tex0", RT_ERR_INVALID;
        if (t == RT_MAT_ROUGH_PLASTIC && s->mat_tex1[m] >= s->n_textures)
            return msg = "rt_scene_upload: RoughPlastic material needs tex1", RT_ERR_INVALID;
    }
    for (uint32_t t = 0; t < s->n_textures; ++t) {
        uint32_t ty = s->tex_type[t];
        if (ty >= RT_TEX__COUNT) return msg = "rt_scene_upload: unknown texture type", RT_ERR_INVALID;
        if (ty == RT_TEX_PERLIN && s->tex_aux[t] >= s->n_perlin)
            return msg = "rt_scene_upload: Perlin texture references a missing table set", RT_ERR_INVALID;
        if (ty == RT_TEX_IMAGE && s->tex_aux[t] >= s->n_images)
            return msg = "rt_scene_upload: image texture references a missing image", RT_ERR_INVALID;
    }
    for (uint32_t k = 0; k < s->n_perlin * 3u * RT_PERLIN_POINTS; ++k)
        if (s->perlin_perm[k] >= RT_PERLIN_POINTS)
            return msg = "rt_scene_upload: perlin permutation entry out of range", RT_ERR_INVALID;
    for (uint32_t k = 0; k < s->n_images; ++k) {
        if (s->img_w[k] == 0 || s->img_h[k] == 0) return msg = "rt_scene_upload: empty image", RT_ERR_INVALID;
        if (s->img_offset[k] % 3u) return msg = "rt_scene_upload: image offset not a multiple of 3", RT_ERR_INVALID;
        if (s->img_offset[k] + 3ull * s->img_w[k] * s->img_h[k] > s->n_texel_floats) return msg = "rt_scene_upload: image exceeds texel pool", RT_ERR_INVALID;
    }
    if (s->sky_type > RT_SKY_ENV) return msg = "rt_scene_upload: unknown sky type", RT_ERR_INVALID;
    if (s->sky_type == RT_SKY_ENV && s->sky_image >= s->n_images)
        return msg = "rt_scene_upload: env sky references a missing image", RT_ERR_INVALID;
    return RT_OK;
}

// The spheres of a scene as the kernels read them: (c, r)
inline std::vector<float4> pack_spheres(const RtFlatScene* s) {
    std::vector<float4> geo(s->n_spheres);
    for (uint32_t i = 0; i < s->n_spheres; ++i) geo[i] = make_float4(s->sph_cx[i], s->sph_cy[i], s->sph_cz[i], s->sph_r[i]);
    return geo;
}

// The arrays of an RtFlatScene as the kernels read them (`opt`: the context's options).
struct PackedScene {
    std::vector<float4> geo, rgeo;     // spheres (c, r); rectangles (k, u0, u1, v0), (v1, axis) with (u, v) the uv axes of hitable.rs:262-263 etc.
    std::vector<uint32_t> smat;
    std::vector<MatRec> mats;
    std::vector<TexRec> texs;
    std::vector<float4> pvec;
    std::vector<unsigned short> pperm2;
    std::vector<ImgRec> imgs;
    bool all_u8 = false;               // the texel pool is RGBA8 (texels8), else float4 (texels)
    std::vector<float4> texels;
    std::vector<uint32_t> texels8;
    std::vector<float4> xparam;
    std::vector<uint2> xmeta;
    uint32_t n_xf_listed = 0;
    int pack(const RtFlatScene* s, const uint32_t* opt, std::string& msg) {
        geo = pack_spheres(s);
        smat.assign(s->sph_mat, s->sph_mat + s->n_spheres);
        mats.resize(s->n_materials);
        for (uint32_t m = 0; m < s->n_materials; ++m) {
            MatRec r{};
            r.type = s->mat_type[m];
            r.tex0 = s->mat_tex0[m];
            r.tex1 = s->mat_tex1[m];
            r.cr = s->mat_color[3 * m], r.cg = s->mat_color[3 * m + 1], r.cb = s->mat_color[3 * m + 2];
            r.p0 = s->mat_p0[m], r.p1 = s->mat_p1[m], r.p2 = s->mat_p2[m], r.p3 = s->mat_p3[m];
            mats[m] = r;
        }
        texs.resize(s->n_textures);
        for (uint32_t t = 0; t < s->n_textures; ++t) {
            TexRec r{};
            r.type = s->tex_type[t];
            r.aux = s->tex_aux[t];
            r.scale = s->tex_scale[t];
            r.c0r = s->tex_color0[3 * t], r.c0g = s->tex_color0[3 * t + 1], r.c0b = s->tex_color0[3 * t + 2];
            r.c1r = s->tex_color1[3 * t], r.c1g = s->tex_color1[3 * t + 1], r.c1b = s->tex_color1[3 * t + 2];
            texs[t] = r;
        }
        pvec.resize((size_t)s->n_perlin * 256);
        std::vector<uint8_t> pperm((size_t)s->n_perlin * 768);
        for (size_t k = 0; k < pvec.size(); ++k)
            pvec[k] = make_float4(s->perlin_vec[3 * k], s->perlin_vec[3 * k + 1], s->perlin_vec[3 * k + 2], 0.0f);
        for (size_t k = 0; k < pperm.size(); ++k) pperm[k] = (uint8_t)s->perlin_perm[k];
        pperm2.resize(pperm.size()); // entry i with its successor on the 256-ring (PerlinTables)
        for (size_t k = 0; k < pperm.size(); ++k)
            pperm2[k] = (unsigned short)(pperm[k] | (pperm[(k & ~(size_t)255) + ((k + 1) & 255)] << 8));
        imgs.resize(s->n_images);
        // The texel pool: RGBA8 when every component of every image is exactly k/255 (what image::open(..).to_rgb32f() makes of
        // an 8-bit file, texture.rs:176-177; image_value() divides k by 255 again and gets the same float), float4 otherwise.
        auto as_u8 = [](float t, uint32_t& k) {
            if (!(t >= 0.0f && t <= 1.0f)) return false;
            k = (uint32_t)std::lrintf(t * 255.0f);
            const float back = (float)k / 255.0f;
            return k <= 255u && std::memcmp(&back, &t, sizeof(float)) == 0;
        };
        all_u8 = s->n_images > 0 && opt[RT_OPT_TEXEL_POOL] != 1u;
        for (uint32_t k = 0; k < s->n_images && all_u8; ++k) {
            const float* src = s->texels + s->img_offset[k];
            const size_t nc = (size_t)s->img_w[k] * s->img_h[k] * 3u;
            uint32_t q;
            for (size_t c = 0; c < nc && all_u8; ++c) all_u8 = as_u8(src[c], q);
        }
        uint64_t n_texels = 0;
        for (uint32_t k = 0; k < s->n_images; ++k) n_texels = std::max<uint64_t>(n_texels, (s->img_offset[k] + 3ull * s->img_w[k] * s->img_h[k]) / 3u);
        texels.resize(all_u8 ? 0 : (size_t)n_texels);
        texels8.resize(all_u8 ? (size_t)n_texels : 0);
        for (uint32_t k = 0; k < s->n_images; ++k) {
            uint64_t off = s->img_offset[k] / 3u;
            imgs[k] = ImgRec{s->img_w[k], s->img_h[k], (uint32_t)off, (uint32_t)(off >> 32)};
            const float* src = s->texels + s->img_offset[k];
            const size_t np = (size_t)s->img_w[k] * s->img_h[k];
            for (size_t p = 0; p < np; ++p) {
                if (all_u8) {
                    uint32_t r = 0, g = 0, b = 0;
                    as_u8(src[3 * p], r), as_u8(src[3 * p + 1], g), as_u8(src[3 * p + 2], b);
                    texels8[off + p] = r | (g << 8) | (b << 16);
                } else {
                    texels[off + p] = make_float4(src[3 * p], src[3 * p + 1], src[3 * p + 2], 0.0f);
                }
            }
        }

        rgeo.resize((size_t)s->n_rects * 2);
        for (uint32_t i = 0; i < s->n_rects; ++i) {
            const uint32_t ax = s->rect_axis[i];
            const float* mn = s->rect_min + 3 * (size_t)i;
            const float* mx = s->rect_max + 3 * (size_t)i;
            const int ua = ax == 0 ? 1 : 0, va = ax == 2 ? 1 : 2;
            rgeo[2 * (size_t)i] = make_float4(mn[ax], mn[ua], mx[ua], mn[va]);
            rgeo[2 * (size_t)i + 1] = make_float4(mx[va], fbits(ax), 0.0f, 0.0f);
        }
        // instance wrappers: the listed long chains (the per-primitive innermost wrapper and the world-space bounds come from world_bounds())
        xparam.resize(s->n_xforms), xmeta.resize(s->n_xforms);
        // xf_meta[x] = (type, parent).  A chain of more than RT_MAX_CHAIN wrappers is listed once more behind the table, outermost wrapper
        // first, as (wrapper, chain length), and xf_param[x].w holds where — 0 for a short chain (rt_device.h: the kernels walk short
        // chains through the parent links into registers and long ones through the list).
        std::vector<uint32_t> xf_depth(s->n_xforms);
        std::vector<uint8_t> xf_is_innermost(s->n_xforms, 0); // only the wrapper a primitive or a medium names is ever looked up by a kernel
        for (uint32_t i = 0; i < s->n_spheres && s->sph_xform; ++i)
            if (s->sph_xform[i] != RT_NO_XFORM) xf_is_innermost[s->sph_xform[i]] = 1;
        for (uint32_t i = 0; i < s->n_rects && s->rect_xform; ++i)
            if (s->rect_xform[i] != RT_NO_XFORM) xf_is_innermost[s->rect_xform[i]] = 1;
        for (uint32_t m = 0; m < s->n_media && s->med_xform; ++m)
            if (s->med_xform[m] != RT_NO_XFORM && s->med_xform[m] < s->n_xforms) xf_is_innermost[s->med_xform[m]] = 1;
        for (uint32_t i = 0; i < s->n_xforms; ++i) {
            const uint32_t depth = xf_depth[i] = s->xf_parent[i] == RT_NO_XFORM ? 1u : xf_depth[s->xf_parent[i]] + 1u;
            xparam[i] = make_float4(s->xf_param[4 * i], s->xf_param[4 * i + 1], s->xf_param[4 * i + 2], 0.0f);
            xmeta[i] = make_uint2(s->xf_type[i], s->xf_parent[i]);
            if (depth > (uint32_t)RT_MAX_CHAIN && xf_is_innermost[i]) {
                if ((uint64_t)s->n_xforms + n_xf_listed + depth > 0x7FFFFFFFull) return msg = "rt_scene_upload: wrapper chains too long to list", RT_ERR_UNSUPPORTED;
                xparam[i].w = fbits(s->n_xforms + n_xf_listed);
                n_xf_listed += depth;
            }
        }
        xmeta.resize((size_t)s->n_xforms + n_xf_listed);
        for (uint32_t i = 0; i < s->n_xforms; ++i) {
            if (xf_depth[i] <= (uint32_t)RT_MAX_CHAIN || !xf_is_innermost[i]) continue;
            uint32_t p0, k = xf_depth[i];
            std::memcpy(&p0, &xparam[i].w, 4);
            for (uint32_t x = i; x != RT_NO_XFORM; x = s->xf_parent[x]) xmeta[p0 + --k] = make_uint2(x, xf_depth[i]);
        }
        return RT_OK;
    }
};

// What rt_set_motion and rt_set_quads need of the uploaded scene on the host: to bound the moved spheres again, and what the records and
// sort keys of planar primitives are made of with the static ones they are appended to.
struct Keep {
    std::vector<float4> geo;         // spheres (c0, r)
    std::vector<PrimBox> eboxes;     // world entries, unpadded
    std::vector<uint32_t> entry_ids;
    std::vector<float4> ent_bs;
    std::vector<uint8_t> bare;       // per sphere: no wrapper, not a medium boundary
    std::vector<MatRec> mats;
    std::vector<TexRec> texs;
    std::vector<float4> srec;        // 5 per world entry
    std::vector<uint8_t> raw_class;  // per world entry, before the ranking of the classes present
    uint32_t sky_type = 0;
    double world_mag = 0.0;          // largest coordinate magnitude of the world entries' bounds
};

// ---- planar primitives (rt_set_quads) --------------------------------------------------------------------------------------------
// The set-up of rtow_mi355x.h in f32 (this file is built with -ffp-contract=off: one rounding per operation), the box of every
// primitive's corners and its slack.  DESIGN.md "Planar primitives" derives the slack; in short, for a ray whose origin coordinates
// stay within RT_PLANAR_REACH W and a primitive with s = sin(u, v) >= 2^-10:
//   - the plane the kernels test is the f32 (normal, D): tilted against the exact one by <= 3.5 eps / s, i.e. off by <= 7 eps L / s over the figure;
//   - alpha, beta carry <= 9 eps |p| / (|u| s) of rounding and 3.5 eps / s of scale (w), i.e. <= 22 eps L / s in space for |p| <= 2 L;
//   - P = fl(o + fl(d t)) and the two dot products of t move the accepted point by <= 16 eps (M + reach) (3 + 2 x 3 sqrt(3) roundings).
// eps = 2^-24.  The constants are rounded up to 64 and 16; the slack is added in double, rounded outwards, BEFORE pad_prim_box.
struct PlanarHost {
    std::vector<float4> pq;     // 5 per primitive (planar_root)
    std::vector<PrimBox> boxes; // corners + slack
    std::vector<float> slack;
    std::vector<float> len;     // |cross(u, v)| in f32: a parallelogram's area (rt_set_lights)
    double world_mag = 0.0;     // W: the scene's and the set's largest coordinate magnitude
};
// (q->kind NULL: every primitive a quad, a light set's; q->mat is not read)
inline int planar_setup(const RtQuads* q, double world_mag, PlanarHost& out, std::string& err) {
    const uint32_t n = q->n;
    if (!q->q || !q->u || !q->v) return err = "NULL array", RT_ERR_INVALID;
    double W = world_mag;
    for (size_t k = 0; k < 3 * (size_t)n; ++k) {
        if (!std::isfinite(q->q[k]) || !std::isfinite(q->u[k]) || !std::isfinite(q->v[k])) return err = "primitive " + std::to_string(k / 3) + " has a component that is not finite", RT_ERR_INVALID;
        const double a = q->q[k], b = q->u[k], c = q->v[k];
        W = std::max(W, std::max(std::max(std::fabs(a), std::fabs(a + b)), std::max(std::fabs(a + c), std::fabs(a + b + c))));
    }
    out.world_mag = W;
    out.pq.assign(5 * (size_t)n, make_float4(0.f, 0.f, 0.f, 0.f));
    out.boxes.resize(n), out.slack.resize(n), out.len.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t kind = q->kind ? q->kind[i] : (uint32_t)RT_PLANAR_QUAD;
        if (kind > RT_PLANAR_TRIANGLE) return err = "primitive " + std::to_string(i) + " has a kind outside RtPlanarKind", RT_ERR_INVALID;
        const float* Q = q->q + 3 * (size_t)i;
        const float* u = q->u + 3 * (size_t)i;
        const float* v = q->v + 3 * (size_t)i;
        {   // conditioning, in double: |n|^2 >= 2^-20 |u|^2 |v|^2
            const double ud[3] = {u[0], u[1], u[2]}, vd[3] = {v[0], v[1], v[2]};
            const double nd[3] = {ud[1] * vd[2] - ud[2] * vd[1], ud[2] * vd[0] - ud[0] * vd[2], ud[0] * vd[1] - ud[1] * vd[0]};
            const double n2 = nd[0] * nd[0] + nd[1] * nd[1] + nd[2] * nd[2], u2 = ud[0] * ud[0] + ud[1] * ud[1] + ud[2] * ud[2], v2 = vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2];
            if (!(u2 > 0.0 && v2 > 0.0 && n2 >= RT_PLANAR_MIN_SIN2 * u2 * v2)) return err = "primitive " + std::to_string(i) + " is degenerate or ill-conditioned (|u x v|^2 < 2^-20 |u|^2 |v|^2)", RT_ERR_INVALID;
            const double L = std::sqrt(std::max(u2, v2)), sn = std::sqrt(n2 / (u2 * v2));
            double M = 0.0, lo[3], hi[3];
            for (int k = 0; k < 3; ++k) {
                const double c0 = Q[k], c1 = c0 + ud[k], c2 = c0 + vd[k], c3 = c0 + ud[k] + vd[k];
                lo[k] = std::min(std::min(c0, c1), c2), hi[k] = std::max(std::max(c0, c1), c2);
                if (kind == RT_PLANAR_QUAD) lo[k] = std::min(lo[k], c3), hi[k] = std::max(hi[k], c3);
                M = std::max(M, std::max(std::max(std::fabs(c0), std::fabs(c1)), std::max(std::fabs(c2), std::fabs(c3))));
            }
            const double slack = std::ldexp(64.0 * L / sn + 16.0 * (M + RT_PLANAR_REACH * W), -24) * (1.0 + 1e-9) + 1e-37;
            out.slack[i] = round_up(slack);
            for (int k = 0; k < 3; ++k) out.boxes[i].mn[k] = round_down(lo[k] - slack), out.boxes[i].mx[k] = round_up(hi[k] + slack);
        }
        // f32, in the order of the header
        const float nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
        const float nn = (nx * nx + ny * ny) + nz * nz;
        const float len = std::sqrt(nn);
        const float ux = nx / len, uy = ny / len, uz = nz / len;
        const float D = (ux * Q[0] + uy * Q[1]) + uz * Q[2];
        const float wx = nx / nn, wy = ny / nn, wz = nz / nn;
        if (!std::isfinite(ux) || !std::isfinite(uy) || !std::isfinite(uz) || !std::isfinite(D) || !std::isfinite(wx) || !std::isfinite(wy) || !std::isfinite(wz) || !(nn > 0.0f))
            return err = "primitive " + std::to_string(i) + ": the f32 plane set-up overflows or underflows", RT_ERR_INVALID;
        out.len[i] = len;
        out.pq[5 * (size_t)i + 0] = make_float4(ux, uy, uz, D);
        out.pq[5 * (size_t)i + 1] = make_float4(Q[0], Q[1], Q[2], fbits(kind));
        out.pq[5 * (size_t)i + 2] = make_float4(u[0], u[1], u[2], 0.0f);
        out.pq[5 * (size_t)i + 3] = make_float4(v[0], v[1], v[2], 0.0f);
        out.pq[5 * (size_t)i + 4] = make_float4(wx, wy, wz, 0.0f);
    }
    return RT_OK;
}

// ---- rt_scene_upload --------------------------------------------------------------------------------------------------------------
// Everything rt_scene_upload uploads or decides by.  What `keep` holds (sphere geometry, materials, textures, the world entries' boxes,
// ids and bounding spheres, the shading records) lies there only: the upload reads it from there and the context takes it by move.
struct PreparedScene {
    PackedScene pk;                  // (geo, mats, texs: in keep)
    std::vector<uint32_t> pxf, pmed; // per primitive: innermost wrapper, medium
    std::vector<float4> pgeo;        // spheres, then rectangles
    std::vector<uint32_t> med_prims; // media: boundary primitive lists
    std::vector<uint2> med_range;    // (first, count | kind << 24)
    std::vector<float> med_nid;
    std::vector<uint2> med_xf;       // (.x: the chain all boundary primitives share, .y: the wrapper around the medium)
    HostTree tree;
    std::vector<uint8_t> sclass;     // sort keys per world entry (keep.raw_class ranked)
    DevScene ds{};                   // the counts and key_miss; the upload fills in the pointers
    bool nest = false;               // what only the NEST instantiations evaluate (rt_device.h): a listed chain, the media of mask bit 31, a wrapper around a medium
    Keep keep;
};
inline int prepare_scene(const RtFlatScene* s, const uint32_t* opt, PreparedScene& p, std::string& msg) {
    p = PreparedScene{};
    PackedScene& pk = p.pk;
    {   // ---- validate, then pack
        int rc = validate_scene(s, msg);
        if (!rc) rc = pk.pack(s, opt, msg);
        if (rc) return rc;
    }
    const uint32_t n_prims = s->n_spheres + s->n_rects;
    // ---- world-space bounds of primitives and world entries (culling only; the same code answers rt_debug_world_bounds)
    WorldBounds wb;
    world_bounds(s, wb);
    const std::vector<uint32_t>& pxf = wb.pxf;
    const std::vector<uint32_t>& pmed = wb.pmed;
    // media: boundary primitive lists; world entries = primitives that are not a boundary, then the media
    const uint32_t n_entries = n_prims + s->n_media;
    std::vector<uint32_t>& med_prims = p.med_prims;
    std::vector<uint2>& med_range = p.med_range;
    std::vector<uint2>& med_xf = p.med_xf;
    med_range.assign(s->n_media, make_uint2(0u, 0u)), p.med_nid.assign(s->n_media, 0.0f);
    med_xf.assign(s->n_media, make_uint2(RT_NO_XFORM, RT_NO_XFORM));
    for (uint32_t m = 0; m < s->n_media; ++m) {
        med_range[m] = make_uint2((uint32_t)med_prims.size(), 0u);
        p.med_nid[m] = s->med_neg_inv_density[m];
        for (uint32_t i = 0; i < n_prims; ++i)
            if (pmed[i] == m) {
                // one wrapper chain for the whole boundary (a GBox under RotateY/Translate): medium_root moves the ray once
                if (med_range[m].y == 0) med_xf[m].x = pxf[i];
                else if (med_xf[m].x != pxf[i]) med_xf[m].x = RT_MED_XF_MIXED;
                if (s->med_xform && s->med_xform[m] != RT_NO_XFORM) { // the wrapper around the medium lies on the chain of every boundary primitive
                    uint32_t x = pxf[i];
                    while (x != RT_NO_XFORM && x != s->med_xform[m]) x = s->xf_parent[x];
                    if (x == RT_NO_XFORM) return msg = "rt_scene_upload: the wrapper around medium " + std::to_string(m) + " is not on the chain of its boundary primitive " + std::to_string(i), RT_ERR_INVALID;
                }
                med_prims.push_back(i);
                ++med_range[m].y;
            }
        // (validate_geometry: the medium has boundary primitives)
        if (s->med_xform) med_xf[m].y = s->med_xform[m];
        if (med_range[m].y > RT_MED_COUNT_MASK) return msg = "rt_scene_upload: medium " + std::to_string(m) + " has too many boundary primitives", RT_ERR_UNSUPPORTED;
        {   // boundaries whose two searches are answered from one evaluation of their primitives (medium_root, rt_kernels.h)
            bool all_rects = true;
            for (uint32_t k = 0; k < med_range[m].y; ++k) all_rects = all_rects && med_prims[med_range[m].x + k] >= s->n_spheres;
            uint32_t kind = 0u;
            if (med_xf[m].x != RT_MED_XF_MIXED && all_rects && med_range[m].y <= 6u) kind = RT_MED_KIND_RECTS;
            else if (med_xf[m].x != RT_MED_XF_MIXED && med_range[m].y == 1u && med_prims[med_range[m].x] < s->n_spheres) kind = RT_MED_KIND_SPHERE;
            if (opt[RT_OPT_MEDIUM_SEARCH] == 1u) kind = 0u; // test hook: the two searches as the reference makes them
            med_range[m].y |= kind << 24;
        }
    }
    // ---- tree
    build_tree(wb.ent, wb.entry_ids, p.tree);
    // ---- shading records and sort keys
    Keep& kp = p.keep;
    kp.raw_class.assign(n_entries, 0);
    // (at least one record: shade() issues the loads of record 0 for a miss too, see rt_device.h, so an empty scene
    // still needs 5 readable float4)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    kp.srec.assign((size_t)std::max<uint32_t>(n_entries, 1u) * 5, zero4);
    for (uint32_t i = 0; i < n_entries; ++i) {
        const bool is_med = i >= n_prims;
        const bool is_rect = !is_med && i >= s->n_spheres;
        const uint32_t m = is_med ? s->med_mat[i - n_prims] : (is_rect ? s->rect_mat[i - s->n_spheres] : s->sph_mat[i]);
        const float4* rg = is_rect ? &pk.rgeo[2 * (size_t)(i - s->n_spheres)] : nullptr;
        kp.raw_class[i] = shading_record(pk.mats[m], pk.texs, is_med ? make_float4(0.f, 0.f, 0.f, 1.f) : (is_rect ? rg[0] : pk.geo[i]), is_rect ? rg[1] : zero4,
                                         &kp.srec[5 * (size_t)i]);
    }
    p.sclass = kp.raw_class; // (rt_set_quads ranks the raw classes again with those of its primitives)
    DevScene& ds = p.ds;
    ds.key_miss = rank_classes(p.sclass, s->sky_type);
    ds.n_xforms = s->n_xforms;
    ds.n_media = s->n_media;
    ds.n_rects = s->n_rects;
    ds.n_prims = n_prims;
    ds.n_entries = (uint32_t)wb.ent.size();
    ds.n_med_prims = (uint32_t)med_prims.size();
    ds.n_xf_listed = pk.n_xf_listed;
    p.nest = pk.n_xf_listed > 0 || s->n_media > 32u;
    for (uint32_t m = 0; m < s->n_media && s->med_xform; ++m) p.nest = p.nest || s->med_xform[m] != RT_NO_XFORM;
    ds.n_spheres = s->n_spheres, ds.n_materials = s->n_materials, ds.n_textures = s->n_textures;
    ds.n_perlin = s->n_perlin, ds.n_images = s->n_images, ds.sky_type = s->sky_type, ds.sky_image = s->sky_image;
    p.pgeo = pk.geo;
    p.pgeo.insert(p.pgeo.end(), pk.rgeo.begin(), pk.rgeo.end());
    // ---- what rt_set_motion and rt_set_quads need of the scene on the host
    kp.bare.assign(s->n_spheres, 0);
    for (uint32_t i = 0; i < s->n_spheres; ++i) kp.bare[i] = pxf[i] == RT_NO_XFORM && pmed[i] == RT_NO_MEDIUM;
    kp.sky_type = s->sky_type;
    kp.world_mag = 0.0;
    for (const PrimBox& b : wb.ent)
        for (int k = 0; k < 3; ++k)
            if (std::isfinite(b.mn[k]) && std::isfinite(b.mx[k])) kp.world_mag = std::max(kp.world_mag, (double)std::max(std::fabs(b.mn[k]), std::fabs(b.mx[k])));
    kp.geo = std::move(pk.geo), kp.mats = std::move(pk.mats), kp.texs = std::move(pk.texs);
    kp.eboxes = std::move(wb.ent), kp.entry_ids = std::move(wb.entry_ids), kp.ent_bs = std::move(wb.ent_bs);
    p.pxf = std::move(wb.pxf), p.pmed = std::move(wb.pmed);
    return RT_OK;
}

// ---- rt_set_motion ----------------------------------------------------------------------------------------------------------------
inline int check_shutter(const RtMotion* m, std::string& msg) {
    if (!std::isfinite(m->shutter_open) || !std::isfinite(m->shutter_close) || m->shutter_open < 0.0f || m->shutter_close > 1.0f ||
        m->shutter_open > m->shutter_close)
        return msg = "rt_set_motion: the shutter must satisfy 0 <= shutter_open <= shutter_close <= 1", RT_ERR_INVALID;
    return RT_OK;
}
// Moving spheres.  Everything that bounds a listed sphere is built again over the region it sweeps; the static arrays stay where they
// are (clearing the motion only switches back to them).  The kernels form c(tm) = fl(c0 + fl(tm dc)), dc = fl(c1 - c0), tm in [0, 1]:
// the exact point c0 + tm dc lies on the segment from c0 to e1 = c0 + dc (e1 in double: it need not be the caller's c1 to the last
// bit), and the two roundings move a coordinate by at most half an ulp of |dc| and half an ulp of the larger of |c0|, |e1| — together
// below `slack` = 2^-22 of the coordinate magnitude (2 ulp).  The bounds take the union of the two end positions (exact for linear
// motion) and add that slack for the moved spheres, so none of the existing pads (2^-18 of the magnitude around a tree leaf, which
// is there for the slab arithmetic; the list cone's 0.1 % + 2^-21 of the magnitude) is asked to cover it:
//   tree leaf  = [min(c0, e1) - r - slack, max(c0, e1) + r + slack], then pad_prim_box as for every leaf;
//   ent_bs     = centre (c0 + e1) / 2, radius r + |e1 - c0| / 2 + the distance the rounded centre moved + sqrt(3) slack, rounded up;
//   grid       = build_sphere_grid's swept boxes (its own argument for the roundings, rt_grid.h).
struct PreparedMotion {
    std::vector<uint32_t> sphere;  // the moved spheres
    std::vector<float4> dc;        // per sphere: (displacement, 1), 0 for one that rests
    std::vector<PrimBox> eboxes;   // world entries over the swept regions, unpadded (pad_prim_box is applied on the way out, as the builder does)
    std::vector<float4> ent_bs;
    HostTree tree;
};
inline int prepare_motion(const Keep& kp, uint32_t n_sph, const RtMotion* motion, PreparedMotion& pm, std::string& msg) {
    pm = PreparedMotion{};
    const uint32_t nm = motion->n_moving;
    if (!motion->sphere || !motion->center1) return msg = "rt_set_motion: NULL array", RT_ERR_INVALID;
    if (check_shutter(motion, msg)) return RT_ERR_INVALID;
    for (uint32_t k = 0; k < nm; ++k) {
        const uint32_t i = motion->sphere[k];
        if (i >= n_sph) return msg = "rt_set_motion: sphere index " + std::to_string(i) + " out of range", RT_ERR_INVALID;
        if (k > 0 && i <= motion->sphere[k - 1]) return msg = "rt_set_motion: sphere indices must be strictly increasing", RT_ERR_INVALID;
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(motion->center1[3 * (size_t)k + c])) return msg = "rt_set_motion: non-finite center1 of sphere " + std::to_string(i), RT_ERR_INVALID;
        if (!kp.bare[i])
            return msg = "rt_set_motion: sphere " + std::to_string(i) + " lies below a Translate / RotateY wrapper or bounds a medium: only bare spheres move", RT_ERR_UNSUPPORTED;
    }
    // ---- displacements and swept bounds
    pm.sphere.assign(motion->sphere, motion->sphere + nm);
    std::vector<float4>& dc = pm.dc;
    dc.assign(std::max<uint32_t>(n_sph, 1u), make_float4(0.f, 0.f, 0.f, 0.f));
    std::vector<PrimBox>& eboxes = pm.eboxes = kp.eboxes;
    std::vector<float4>& ent_bs = pm.ent_bs = kp.ent_bs;
    std::vector<uint32_t> entry_of(n_sph, 0xFFFFFFFFu);
    for (size_t e = 0; e < kp.entry_ids.size(); ++e)
        if (kp.entry_ids[e] < n_sph) entry_of[kp.entry_ids[e]] = (uint32_t)e;
    for (uint32_t k = 0; k < nm; ++k) {
        const uint32_t i = motion->sphere[k];
        const float4 g = kp.geo[i];
        const float c0[3] = {g.x, g.y, g.z};
        float d[3];
        for (int c = 0; c < 3; ++c) d[c] = motion->center1[3 * (size_t)k + c] - c0[c]; // fl(c1 - c0), once
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(d[c])) return msg = "rt_set_motion: the displacement of sphere " + std::to_string(i) + " overflows", RT_ERR_INVALID;
        dc[i] = make_float4(d[0], d[1], d[2], 1.0f);
        const uint32_t e = entry_of[i]; // (a bare sphere is a world entry)
        const double r = std::fabs((double)g.w);
        double mid[3], half2 = 0.0, slack_max = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double a = c0[c], b = (double)c0[c] + (double)d[c];
            const double slack = std::ldexp(std::max(std::fabs(a), std::fabs(b)), -22) + 1e-37;
            slack_max = std::max(slack_max, slack);
            eboxes[e].mn[c] = round_down(std::min(a, b) - r - slack);
            eboxes[e].mx[c] = round_up(std::max(a, b) + r + slack);
            mid[c] = 0.5 * (a + b);
            half2 += 0.25 * (b - a) * (b - a);
        }
        float4 bs = make_float4((float)mid[0], (float)mid[1], (float)mid[2], 0.0f);
        const double mx = mid[0] - bs.x, my = mid[1] - bs.y, mz = mid[2] - bs.z;
        bs.w = round_up((r + std::sqrt(half2) + std::sqrt(mx * mx + my * my + mz * mz) + 1.7321 * slack_max) * (1.0 + 1e-12));
        ent_bs[e] = bs;
    }
    build_tree(eboxes, kp.entry_ids, pm.tree);
    return RT_OK;
}

// ---- rt_set_quads -----------------------------------------------------------------------------------------------------------------
// The scene's records, sort keys and tree with those of the set behind them (world entries n_prims + n_media + i).
struct PreparedQuads {
    PlanarHost ph;
    std::vector<float4> srec;
    std::vector<uint8_t> sclass;
    uint32_t key_miss = 0;
    uint32_t n_entries = 0; // tree leaves: the scene's world entries and the set
    HostTree tree;
};
inline int prepare_quads(const Keep& kp, uint32_t n_prims, uint32_t n_media, const RtQuads* quads, PreparedQuads& pq, std::string& msg) {
    pq = PreparedQuads{};
    const uint32_t n = quads->n, base = n_prims + n_media;
    if ((uint64_t)base + n > 32768u) return msg = "rt_set_quads: more than 32768 world entries with the set", RT_ERR_INVALID;
    if (!quads->kind || !quads->mat) return msg = "rt_set_quads: NULL array", RT_ERR_INVALID;
    PlanarHost& ph = pq.ph;
    if (const int rc = planar_setup(quads, kp.world_mag, ph, msg)) return msg = "rt_set_quads: " + msg, rc;
    for (uint32_t i = 0; i < n; ++i) {
        if (quads->mat[i] >= kp.mats.size()) return msg = "rt_set_quads: primitive " + std::to_string(i) + " has material index out of range", RT_ERR_INVALID;
        if (kp.mats[quads->mat[i]].type == RT_MAT_DISNEY_METAL)
            return msg = "rt_set_quads: DisneyMetal on a planar primitive reads a tangent it does not carry", RT_ERR_UNSUPPORTED;
    }
    // ---- records and sort keys: the static ones, then the set's; the classes present are ranked again (rt_scene_upload)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    pq.srec.assign((size_t)(base + n) * 5, zero4);
    std::copy(kp.srec.begin(), kp.srec.begin() + 5 * (size_t)base, pq.srec.begin());
    pq.sclass = kp.raw_class;
    pq.sclass.resize((size_t)base + n);
    for (uint32_t i = 0; i < n; ++i) pq.sclass[base + i] = shading_record(kp.mats[quads->mat[i]], kp.texs, zero4, zero4, &pq.srec[5 * (size_t)(base + i)]);
    pq.key_miss = rank_classes(pq.sclass, kp.sky_type);
    // ---- the tree over the scene's entries and the set
    std::vector<PrimBox> eboxes = kp.eboxes;
    std::vector<uint32_t> entry_ids = kp.entry_ids;
    for (uint32_t i = 0; i < n; ++i) eboxes.push_back(ph.boxes[i]), entry_ids.push_back(base + i);
    pq.n_entries = (uint32_t)eboxes.size();
    build_tree(eboxes, entry_ids, pq.tree);
    if (pq.tree.bvh4.id.size() >= 32768u || pq.tree.depth > RT_BVH_MAX_DEPTH) return msg = "rt_set_quads: the tree over the set has more nodes or levels than the kernels index", RT_ERR_INVALID;
    return RT_OK;
}

// ---- light importance sampling (rt_set_lights) -----------------------------------------------------------------------------------
// The table the LIGHTS instantiations of k_shade read, in ph.pq: per light the five float4 of a planar quad (planar_setup: the same
// conditioning test in double and the same f32 plane set-up as rt_set_quads) with area = sqrt(dot(n, n)), n = cross(u, v), in the free w of g[3].
inline int prepare_lights(const RtLights* lights, PlanarHost& ph, std::string& msg) {
    ph = PlanarHost{};
    const uint32_t n = lights->n;
    if (n > RT_MAX_LIGHTS) return msg = "rt_set_lights: more than RT_MAX_LIGHTS (16) lights", RT_ERR_INVALID;
    const RtQuads as_quads{n, lights->q, lights->u, lights->v, nullptr, nullptr};
    if (const int rc = planar_setup(&as_quads, 0.0, ph, msg)) return msg = "rt_set_lights: " + msg, rc;
    for (uint32_t i = 0; i < n; ++i) {
        const float area = ph.len[i];
        if (!std::isfinite(area) || !(area > 0.0f)) return msg = "rt_set_lights: light " + std::to_string(i) + ": the f32 area overflows or underflows", RT_ERR_INVALID;
        ph.pq[5 * (size_t)i + 3].w = area;
    }
    return RT_OK;
}

} // namespace rt
