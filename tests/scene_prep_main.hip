// The host-side scene preparation (csrc/rt_scene_prep.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_scene_prep_sanitize.py and run without a GPU (no HIP runtime call).  Every valid case prints
//   <name> <rc> <n_entries> <n_tree_nodes> <tree_depth> <n_xf_listed> <nest>
// (prepare_motion / prepare_quads / prepare_lights / build_sphere_grid cases: <name> <rc> and what they built), every refused input
//   refuse <rule> <rc>
// and whatever is prepared is checked for indices out of range before it is printed: a violation ends the program with status 1.
#include "rt_scene_prep.h"
#include "rtow_host.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace rt;

namespace {

int g_bad = 0;
#define EXPECT(cond, what)                                        \
    do {                                                          \
        if (!(cond)) std::printf("FAILED %s: %s\n", what, #cond), ++g_bad; \
    } while (0)

// A scene written array by array (one constant texture per material).
struct Flat {
    std::vector<float> cx, cy, cz, r, rmin, rmax, xparam, mnid, mcol, p0, p1, p2, p3, tc0, tc1, tscale, pvec, texels;
    std::vector<uint32_t> smat, sxf, smed, rmat, rxf, rmed, xparent, mmat, mxf, t0, t1, taux, img_w, img_h;
    std::vector<uint8_t> raxis, xtype, mtype, ttype;
    std::vector<uint16_t> pperm;
    std::vector<uint64_t> img_off;
    uint64_t n_texel_floats = 0;
    uint32_t material(uint32_t type, uint32_t tex_type = RT_TEX_CONSTANT, uint32_t aux = 0) {
        ttype.push_back((uint8_t)tex_type), tscale.push_back(1.0f), taux.push_back(aux);
        for (int k = 0; k < 3; ++k) tc0.push_back(0.5f), tc1.push_back(0.25f), mcol.push_back(0.75f);
        mtype.push_back((uint8_t)type), p0.push_back(0.5f), p1.push_back(0.5f), p2.push_back(0.0f), p3.push_back(0.0f);
        t0.push_back((uint32_t)ttype.size() - 1u), t1.push_back(RT_NO_TEX);
        return (uint32_t)mtype.size() - 1u;
    }
    uint32_t sphere(float x, float y, float z, float rad, uint32_t mat, uint32_t xf = RT_NO_XFORM, uint32_t med = RT_NO_MEDIUM) {
        cx.push_back(x), cy.push_back(y), cz.push_back(z), r.push_back(rad), smat.push_back(mat), sxf.push_back(xf), smed.push_back(med);
        return (uint32_t)cx.size() - 1u;
    }
    void rect(uint32_t axis, float x0, float y0, float z0, float x1, float y1, float z1, uint32_t mat, uint32_t xf = RT_NO_XFORM, uint32_t med = RT_NO_MEDIUM) {
        raxis.push_back((uint8_t)axis), rmat.push_back(mat), rxf.push_back(xf), rmed.push_back(med);
        rmin.insert(rmin.end(), {x0, y0, z0}), rmax.insert(rmax.end(), {x1, y1, z1});
    }
    void box(float x0, float y0, float z0, float x1, float y1, float z1, uint32_t mat, uint32_t xf, uint32_t med) { // (the six sides of a GBox)
        rect(RT_RECT_XY, x0, y0, z1, x1, y1, z1, mat, xf, med), rect(RT_RECT_XY, x0, y0, z0, x1, y1, z0, mat, xf, med);
        rect(RT_RECT_XZ, x0, y1, z0, x1, y1, z1, mat, xf, med), rect(RT_RECT_XZ, x0, y0, z0, x1, y0, z1, mat, xf, med);
        rect(RT_RECT_YZ, x1, y0, z0, x1, y1, z1, mat, xf, med), rect(RT_RECT_YZ, x0, y0, z0, x0, y1, z1, mat, xf, med);
    }
    uint32_t translate(float x, float y, float z, uint32_t parent) {
        xtype.push_back(RT_XF_TRANSLATE), xparent.push_back(parent), xparam.insert(xparam.end(), {x, y, z, 0.0f});
        return (uint32_t)xtype.size() - 1u;
    }
    uint32_t rotate_y(float degrees, uint32_t parent) {
        const float rad = degrees * 3.14159265f / 180.0f;
        xtype.push_back(RT_XF_ROTATE_Y), xparent.push_back(parent), xparam.insert(xparam.end(), {std::sin(rad), std::cos(rad), degrees, 0.0f});
        return (uint32_t)xtype.size() - 1u;
    }
    uint32_t medium(float density, uint32_t xf = RT_NO_XFORM) {
        mnid.push_back(-1.0f / density), mmat.push_back(material(RT_MAT_ISOTROPIC)), mxf.push_back(xf);
        return (uint32_t)mnid.size() - 1u;
    }
    void perlin_set() {
        for (uint32_t k = 0; k < 3u * RT_PERLIN_POINTS; ++k) pvec.push_back(0.577f), pperm.push_back((uint16_t)(k % RT_PERLIN_POINTS));
    }
    void image(uint32_t w, uint32_t h) {
        img_w.push_back(w), img_h.push_back(h), img_off.push_back(texels.size());
        texels.resize(texels.size() + 3u * (size_t)w * h, 0.5f);
        n_texel_floats = texels.size();
    }
    RtFlatScene flat() const {
        RtFlatScene f{};
        f.n_spheres = (uint32_t)cx.size(), f.sph_cx = cx.data(), f.sph_cy = cy.data(), f.sph_cz = cz.data(), f.sph_r = r.data(), f.sph_mat = smat.data();
        f.n_rects = (uint32_t)raxis.size(), f.rect_axis = raxis.data(), f.rect_min = rmin.data(), f.rect_max = rmax.data(), f.rect_mat = rmat.data();
        f.n_xforms = (uint32_t)xtype.size(), f.xf_type = xtype.data(), f.xf_param = xparam.data(), f.xf_parent = xparent.data();
        f.sph_xform = sxf.data(), f.rect_xform = rxf.data();
        f.n_media = (uint32_t)mnid.size(), f.med_neg_inv_density = mnid.data(), f.med_mat = mmat.data(), f.med_xform = mxf.data();
        f.sph_medium = smed.data(), f.rect_medium = rmed.data();
        f.n_materials = (uint32_t)mtype.size(), f.mat_type = mtype.data(), f.mat_color = mcol.data();
        f.mat_p0 = p0.data(), f.mat_p1 = p1.data(), f.mat_p2 = p2.data(), f.mat_p3 = p3.data(), f.mat_tex0 = t0.data(), f.mat_tex1 = t1.data();
        f.n_textures = (uint32_t)ttype.size(), f.tex_type = ttype.data(), f.tex_color0 = tc0.data(), f.tex_color1 = tc1.data();
        f.tex_scale = tscale.data(), f.tex_aux = taux.data();
        f.n_perlin = (uint32_t)(pperm.size() / (3u * RT_PERLIN_POINTS)), f.perlin_vec = pvec.data(), f.perlin_perm = pperm.data();
        f.n_images = (uint32_t)img_w.size(), f.img_w = img_w.data(), f.img_h = img_h.data(), f.img_offset = img_off.data();
        f.texels = texels.data(), f.n_texel_floats = n_texel_floats;
        f.sky_type = RT_SKY_GRADIENT;
        return f;
    }
};

// every child of the tree is a node of it, or a world entry the scene has
void check_tree(const HostTree& t, uint32_t n_ids, const char* what) {
    const int n_nodes = (int)t.bvh4.id.size();
    for (int k = 0; k < 6; ++k) EXPECT(t.bvh4.p[k].size() == t.bvh4.id.size(), what);
    for (const int4& c : t.bvh4.id)
        for (int v : {c.x, c.y, c.z, c.w}) {
            if (v == INT_MIN) continue;
            if (v >= 0) EXPECT(v < n_nodes, what);
            else EXPECT((uint32_t)~v < n_ids, what);
        }
}

// what the kernels index with, against what they index into
void check_scene(const RtFlatScene& f, const PreparedScene& p, const char* what) {
    const uint32_t n_prims = f.n_spheres + f.n_rects, n_ids = n_prims + f.n_media;
    EXPECT(p.pxf.size() == n_prims && p.pmed.size() == n_prims && p.pgeo.size() == f.n_spheres + 2u * (size_t)f.n_rects, what);
    EXPECT(p.keep.eboxes.size() == p.ds.n_entries && p.keep.entry_ids.size() == p.ds.n_entries && p.keep.ent_bs.size() == p.ds.n_entries, what);
    EXPECT(p.sclass.size() == n_ids && p.keep.raw_class.size() == n_ids && p.keep.srec.size() == 5u * (size_t)std::max(n_ids, 1u), what);
    for (uint32_t id : p.keep.entry_ids) EXPECT(id < n_ids, what);
    for (uint8_t c : p.keep.raw_class) EXPECT(c < RT_NCLASS, what);
    for (uint8_t k : p.sclass) EXPECT(k < RT_NCLASS, what);
    EXPECT(p.ds.key_miss < RT_NCLASS, what);
    EXPECT(p.med_range.size() == f.n_media && p.med_xf.size() == f.n_media && p.med_nid.size() == f.n_media, what);
    for (const uint2& rg : p.med_range) EXPECT((size_t)rg.x + (rg.y & RT_MED_COUNT_MASK) <= p.med_prims.size() && (rg.y & RT_MED_COUNT_MASK) > 0u, what);
    for (uint32_t i : p.med_prims) EXPECT(i < n_prims, what);
    EXPECT(p.pk.xparam.size() == f.n_xforms && p.pk.xmeta.size() == (size_t)f.n_xforms + p.pk.n_xf_listed, what);
    for (uint32_t x = 0; x < f.n_xforms; ++x) {
        uint32_t at;
        std::memcpy(&at, &p.pk.xparam[x].w, 4);
        if (!at) continue; // a short chain
        EXPECT(at >= f.n_xforms && at < p.pk.xmeta.size(), what);
        const uint32_t len = at < p.pk.xmeta.size() ? p.pk.xmeta[at].y : 0u;
        EXPECT((size_t)at + len <= p.pk.xmeta.size(), what);
        for (uint32_t k = 0; k < len && (size_t)at + k < p.pk.xmeta.size(); ++k) EXPECT(p.pk.xmeta[at + k].x < f.n_xforms && p.pk.xmeta[at + k].y == len, what);
    }
    for (const ImgRec& im : p.pk.imgs) {
        const uint64_t off = im.offset_lo | ((uint64_t)im.offset_hi << 32);
        EXPECT(off + (uint64_t)im.w * im.h <= (p.pk.all_u8 ? p.pk.texels8.size() : p.pk.texels.size()), what);
    }
    check_tree(p.tree, n_ids, what);
}

int run_scene(const char* name, const RtFlatScene& f, PreparedScene& p, uint32_t texel_pool = 0) {
    uint32_t opt[RT_OPT__COUNT] = {};
    opt[RT_OPT_TEXEL_POOL] = texel_pool;
    std::string msg;
    const int rc = prepare_scene(&f, opt, p, msg);
    if (rc) {
        std::printf("FAILED %s: %d %s\n", name, rc, msg.c_str()), ++g_bad;
        return rc;
    }
    check_scene(f, p, name);
    std::printf("%s %d %u %zu %u %u %d\n", name, rc, p.ds.n_entries, p.tree.bvh4.id.size(), p.tree.bvh4.depth, p.pk.n_xf_listed, (int)p.nest);
    return rc;
}

void refuse_scene(const char* rule, const RtFlatScene& f) {
    uint32_t opt[RT_OPT__COUNT] = {};
    PreparedScene p;
    std::string msg;
    const int rc = prepare_scene(&f, opt, p, msg);
    std::printf("refuse %s %d\n", rule, rc);
    EXPECT(rc == RT_OK || !msg.empty(), rule);
}

Flat plain_spheres(uint32_t n) {
    Flat s;
    const uint32_t m = s.material(RT_MAT_DIFFUSE);
    for (uint32_t i = 0; i < n; ++i) s.sphere((float)(i % 7u) * 2.5f, 0.5f, (float)(i / 7u) * 2.5f, 0.5f + 0.01f * (float)(i % 3u), m);
    return s;
}

} // namespace

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    {   // ---- the demo scenes, with the two images the scene code names
        std::vector<float> img(64 * 32 * 3, 0.5f);
        rth_register_image("res/earthmap.jpg", 64, 32, img.data());
        rth_register_image("res/newport_loft.jpg", 64, 32, img.data());
        const char* names[] = {"sphere_scene", "moving_sphere_scene", "quads_scene", "mesh_scene", "test_sphere", "simple_light_scene",
                               "cornell_box", "final_scene", "earth_env_scene", "pbr_sweep_scene"};
        for (const char* n : names) {
            RthScene* s = nullptr;
            if (rth_scene_build(n, 1.5f, &s) != 0 || !rth_scene_flat(s)) {
                std::printf("FAILED %s: %s\n", n, rth_last_error()), ++g_bad;
                continue;
            }
            PreparedScene p;
            run_scene(n, *rth_scene_flat(s), p);
            if (std::string(n) == "final_scene") run_scene("final_scene/float_texels", *rth_scene_flat(s), p, 1u);
            rth_scene_free(s);
        }
    }
    PreparedScene p;
    {   // ---- an empty scene
        const RtFlatScene f{};
        run_scene("empty", f, p);
    }
    {   // ---- 18 alternating Translate / RotateY wrappers around a sphere and a rectangle: a listed chain
        Flat s;
        const uint32_t m = s.material(RT_MAT_DIFFUSE);
        uint32_t x = RT_NO_XFORM;
        for (int k = 0; k < 18; ++k) x = (k & 1) ? s.rotate_y(7.0f + (float)k, x) : s.translate(0.25f * (float)k, -0.5f, 1.0f, x);
        s.sphere(0.0f, 1.0f, 0.0f, 1.0f, m, x);
        s.rect(RT_RECT_XZ, -1.0f, 0.0f, -1.0f, 1.0f, 0.0f, 1.0f, m, x);
        run_scene("chain18", s.flat(), p);
        EXPECT(p.pk.n_xf_listed == 18u && p.nest, "chain18");
    }
    {   // ---- 33 media, each inside one sphere: the 33rd is tested through mask bit 31
        Flat s;
        const uint32_t m = s.material(RT_MAT_DIELECTRIC);
        for (uint32_t k = 0; k < 33u; ++k) s.sphere(3.0f * (float)k, 0.0f, 0.0f, 1.0f, m, RT_NO_XFORM, s.medium(0.2f));
        run_scene("media33", s.flat(), p);
        EXPECT(p.nest && p.ds.n_entries == 33u, "media33");
        for (const uint2& rg : p.med_range) EXPECT((rg.y >> 24) == RT_MED_KIND_SPHERE, "media33");
    }
    {   // ---- a medium inside a box, the medium wrapped in a RotateY
        Flat s;
        const uint32_t m = s.material(RT_MAT_DIFFUSE);
        const uint32_t x = s.rotate_y(15.0f, RT_NO_XFORM);
        s.box(0.0f, 0.0f, 0.0f, 1.0f, 2.0f, 3.0f, m, x, s.medium(0.01f, x));
        s.sphere(0.0f, -100.0f, 0.0f, 100.0f, m);
        run_scene("rotated_medium", s.flat(), p);
        EXPECT(p.nest && p.ds.n_entries == 2u && (p.med_range[0].y >> 24) == RT_MED_KIND_RECTS && (p.med_range[0].y & RT_MED_COUNT_MASK) == 6u, "rotated_medium");
    }
    // ---- refused scenes: one broken rule each
    {
        Flat s = plain_spheres(3);
        s.cx[1] = nan;
        refuse_scene("nan_sphere_centre", s.flat());
    }
    {
        Flat s = plain_spheres(3);
        s.sxf[0] = s.translate(1.0f, 0.0f, 0.0f, s.translate(1.0f, 0.0f, 0.0f, RT_NO_XFORM));
        s.xparent[1] = 1u;
        refuse_scene("xf_parent_not_before_child", s.flat());
    }
    {
        Flat s = plain_spheres(3);
        s.smat[2] = 7u;
        refuse_scene("sphere_material_out_of_range", s.flat());
    }
    {
        Flat s = plain_spheres(3);
        s.perlin_set();
        s.smat[0] = s.material(RT_MAT_LAMBERT, RT_TEX_PERLIN, 0u);
        s.pperm[300] = 256u;
        refuse_scene("perlin_permutation_256", s.flat());
    }
    {
        Flat s = plain_spheres(3);
        s.image(4, 4);
        s.n_texel_floats -= 1u;
        refuse_scene("image_beyond_texel_pool", s.flat());
    }
    {
        Flat s = plain_spheres(3);
        s.medium(0.2f);
        refuse_scene("medium_without_boundary", s.flat());
    }
    {
        Flat s;
        const uint32_t m = s.material(RT_MAT_DIELECTRIC);
        const uint32_t med_mat = s.material(RT_MAT_ISOTROPIC);
        for (uint32_t k = 0; k <= RT_MAX_MEDIA; ++k) s.sphere((float)(k % 256u), (float)(k / 256u), 0.0f, 0.25f, m, RT_NO_XFORM, k);
        s.mnid.assign(RT_MAX_MEDIA + 1u, -5.0f), s.mmat.assign(RT_MAX_MEDIA + 1u, med_mat), s.mxf.assign(RT_MAX_MEDIA + 1u, RT_NO_XFORM);
        refuse_scene("too_many_media", s.flat());
    }
    {
        Flat s = plain_spheres(3);
        s.rect(RT_RECT_XY, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 0.0f, s.material(RT_MAT_DISNEY_METAL));
        refuse_scene("disney_metal_on_rectangle", s.flat());
    }

    // ---- the sets, over sphere_scene and over the empty scene
    RthScene* hs = nullptr;
    if (rth_scene_build("sphere_scene", 1.5f, &hs) != 0) {
        std::printf("FAILED sphere_scene: %s\n", rth_last_error());
        return 1;
    }
    const RtFlatScene sf = *rth_scene_flat(hs);
    PreparedScene sp, ep;
    {
        uint32_t opt[RT_OPT__COUNT] = {};
        std::string msg;
        const RtFlatScene ef{};
        if (prepare_scene(&sf, opt, sp, msg) || prepare_scene(&ef, opt, ep, msg)) {
            std::printf("FAILED sets: %s\n", msg.c_str());
            return 1;
        }
    }
    const uint32_t ns = sf.n_spheres;
    std::string msg;
    {   // ---- rt_set_motion: the first, the middle and the last sphere move
        const uint32_t idx[3] = {0u, ns / 2u, ns - 1u};
        float c1[9];
        for (int k = 0; k < 3; ++k) c1[3 * k] = sf.sph_cx[idx[k]] + 0.3f, c1[3 * k + 1] = sf.sph_cy[idx[k]] + 0.5f, c1[3 * k + 2] = sf.sph_cz[idx[k]] - 0.2f;
        const RtMotion mo{3u, idx, c1, 0.0f, 1.0f};
        PreparedMotion pm;
        int rc = prepare_motion(sp.keep, ns, &mo, pm, msg);
        EXPECT(pm.dc.size() == ns && pm.eboxes.size() == sp.keep.eboxes.size() && pm.ent_bs.size() == sp.keep.ent_bs.size() && pm.sphere.size() == 3u, "motion");
        check_tree(pm.tree, sf.n_spheres + sf.n_rects + sf.n_media, "motion");
        std::printf("motion %d %zu %zu %u\n", rc, pm.eboxes.size(), pm.tree.bvh4.id.size(), pm.tree.bvh4.depth);
        // build_sphere_grid over the same spheres, at rest and with these displacements
        HostGrid hg;
        build_sphere_grid(sp.keep.geo, 80u * 1024u, 0.0, hg);
        std::printf("grid %d %u %u %u %zu %zu\n", hg.ok ? 0 : 1, hg.gp.nx, hg.gp.ny, hg.gp.nz, hg.cells.size(), hg.refs.size());
        for (uint32_t rec : hg.cells) EXPECT((size_t)(rec >> RT_GRID_CNT_BITS) + (rec & RT_GRID_CNT_MASK) <= hg.refs.size(), "grid");
        for (unsigned short ref : hg.refs) EXPECT(ref < ns, "grid");
        build_sphere_grid(sp.keep.geo, 80u * 1024u, 0.0, hg, &pm.dc);
        std::printf("grid_motion %d %u %u %u %zu %zu\n", hg.ok ? 0 : 1, hg.gp.nx, hg.gp.ny, hg.gp.nz, hg.cells.size(), hg.refs.size());
        for (uint32_t rec : hg.cells) EXPECT((size_t)(rec >> RT_GRID_CNT_BITS) + (rec & RT_GRID_CNT_MASK) <= hg.refs.size(), "grid_motion");
        for (unsigned short ref : hg.refs) EXPECT(ref < ns, "grid_motion");

        const uint32_t beyond[1] = {ns};
        const RtMotion m1{1u, beyond, c1, 0.0f, 1.0f};
        std::printf("refuse motion_index_out_of_range %d\n", prepare_motion(sp.keep, ns, &m1, pm, msg));
        const uint32_t unsorted[2] = {5u, 5u};
        const RtMotion m2{2u, unsorted, c1, 0.0f, 1.0f};
        std::printf("refuse motion_indices_not_increasing %d\n", prepare_motion(sp.keep, ns, &m2, pm, msg));
        Flat w = plain_spheres(3);
        w.sxf[1] = w.translate(1.0f, 0.0f, 0.0f, RT_NO_XFORM);
        PreparedScene wp;
        const RtFlatScene wf = w.flat();
        run_scene("wrapped_sphere", wf, wp);
        const uint32_t wrapped[1] = {1u};
        const RtMotion m3{1u, wrapped, c1, 0.0f, 1.0f};
        std::printf("refuse moving_sphere_below_wrapper %d\n", prepare_motion(wp.keep, 3u, &m3, pm, msg));
    }
    {   // ---- rt_set_quads: four quads and a triangle
        const float q[15] = {0, 0, 0, 3, 0, 0, 0, 2, -4, -5, 1, 1, 2, 2, 2};
        const float u[15] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0.5f, 0, 0};
        const float v[15] = {0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0.5f, 0.25f};
        const uint8_t kind[5] = {RT_PLANAR_QUAD, RT_PLANAR_QUAD, RT_PLANAR_QUAD, RT_PLANAR_QUAD, RT_PLANAR_TRIANGLE};
        const uint32_t mat[5] = {0, 0, 0, 0, 0};
        const RtQuads qs{5u, q, u, v, kind, mat};
        PreparedQuads pq;
        int rc = prepare_quads(sp.keep, sf.n_spheres + sf.n_rects, sf.n_media, &qs, pq, msg);
        check_tree(pq.tree, sf.n_spheres + sf.n_rects + sf.n_media + 5u, "quads");
        EXPECT(pq.ph.pq.size() == 25u && pq.sclass.size() == pq.n_entries && pq.srec.size() == 5u * (size_t)pq.n_entries, "quads");
        std::printf("quads %d %u %zu %u\n", rc, pq.n_entries, pq.tree.bvh4.id.size(), pq.tree.bvh4.depth);
        // (the empty scene has no material: one of its own)
        Keep ek = ep.keep;
        ek.mats.push_back(sp.keep.mats[0]), ek.texs = sp.keep.texs;
        rc = prepare_quads(ek, 0u, 0u, &qs, pq, msg);
        check_tree(pq.tree, 5u, "quads_on_empty");
        std::printf("quads_on_empty %d %u %zu %u\n", rc, pq.n_entries, pq.tree.bvh4.id.size(), pq.tree.bvh4.depth);

        const float par[3] = {2, 0, 0};
        const RtQuads q1{1u, q, u, par, kind, mat};
        std::printf("refuse quad_u_parallel_to_v %d\n", prepare_quads(sp.keep, sf.n_spheres + sf.n_rects, sf.n_media, &q1, pq, msg));
        const uint8_t kind2[1] = {2};
        const RtQuads q2{1u, q, u, v, kind2, mat};
        std::printf("refuse planar_kind_2 %d\n", prepare_quads(sp.keep, sf.n_spheres + sf.n_rects, sf.n_media, &q2, pq, msg));
    }
    {   // ---- rt_set_lights: 1, 16 and 17 lights
        std::vector<float> q, u, v;
        for (int k = 0; k < 17; ++k) q.insert(q.end(), {(float)k, 5.0f, 0.0f}), u.insert(u.end(), {0.5f, 0.0f, 0.0f}), v.insert(v.end(), {0.0f, 0.0f, 0.5f + (float)k});
        for (uint32_t n : {1u, 16u, 17u}) {
            const RtLights ls{n, q.data(), u.data(), v.data()};
            PlanarHost ph;
            const int rc = prepare_lights(&ls, ph, msg);
            if (n <= RT_MAX_LIGHTS) {
                EXPECT(ph.pq.size() == 5u * (size_t)n, "lights");
                std::printf("lights%u %d %zu\n", n, rc, ph.pq.size());
            } else {
                std::printf("refuse 17_lights %d\n", rc);
            }
        }
    }
    rth_scene_free(hs);
    if (g_bad) std::printf("%d checks failed\n", g_bad);
    return g_bad ? 1 : 0;
}
