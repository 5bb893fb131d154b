// Sanitizer driver for the CPU-side producers (libmi355rt_host: scene loader, JSON, OBJ / WO3 / HDR readers, BVH build,
// PNG / PFM writers, the noise estimate), for the CPU oracle's entry points and for scene preparation, the HIP-free half of the device library
// (csrc/device/rt_prepare.cpp: validation, the BVH re-lay, the primitive records; the plan of a render call).  Built with -fsanitize=address,undefined by
// tools/sanitize_host.py; every case must return (OK or an error code) without a sanitizer report.
//   usage: driver <repo root> <scratch dir>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/mi355rt.h"
#include "../../raytracer-rust_amd/csrc/device/rt_prepare.h"

extern "C" int oracle_render(const mi355rt_scene*, const mi355rt_camera*, const mi355rt_settings*, const mi355rt_options*, int, int, uint32_t*, float*, void*);

static int g_fail = 0;
static void expect(bool ok, const std::string& what) { if (!ok) { std::printf("UNEXPECTED: %s\n", what.c_str()); ++g_fail; } }
static void put(const std::string& path, const std::string& bytes) { std::ofstream f(path, std::ios::binary); f.write(bytes.data(), (std::streamsize)bytes.size()); }
static std::string u64(uint64_t v) { return std::string(reinterpret_cast<const char*>(&v), 8); }
static std::string u32(uint32_t v) { return std::string(reinterpret_cast<const char*>(&v), 4); }
static std::string f32s(float v) { return std::string(reinterpret_cast<const char*>(&v), 4); }

static uint32_t g_last_prims = 0, g_last_sky = 0;
static int load(const std::string& path, bool want_ok, uint32_t w = 16, uint32_t h = 12, bool skip_unknown = false) {
    g_last_prims = g_last_sky = 0;
    mi355rt_load_overrides ov{}; ov.width = w; ov.height = h; ov.samples_per_pixel = 1; ov.max_depth = 3; ov.skip_unknown_primitives = skip_unknown;
    mi355rt_loaded_scene* s = nullptr;
    const int rc = mi355rt_scene_load_json(path.c_str(), &ov, &s);
    if (want_ok) expect(rc == MI355RT_OK, path + " should load: " + mi355rt_host_last_error());
    else expect(rc != MI355RT_OK, path + " should be refused");
    if (rc == MI355RT_OK) {
        g_last_prims = mi355rt_loaded_scene_get(s)->n_primitives; g_last_sky = mi355rt_loaded_scene_get(s)->sky_width;
        // push the loaded scene through the oracle too (tiny render): exercises its scene import and BVH build under ASan
        std::vector<uint32_t> px((size_t)w * h);
        mi355rt_options o{}; o.abi_version = MI355RT_ABI_VERSION; o.rng_mode = MI355RT_RNG_CTR;
        const int orc = oracle_render(mi355rt_loaded_scene_get(s), mi355rt_loaded_scene_camera(s), mi355rt_loaded_scene_settings(s), &o, 2, -1, px.data(), nullptr, nullptr);
        expect(orc == 0, path + ": oracle_render");
        mi355rt_scene_free(s);
    }
    return rc;
}

// Scene preparation on a loaded scene: the four shipped scenes must prepare; on semesterbild (one mesh, a sphere) the caller-built
// trees and records that must be refused -- with MI355RT_ERR_INVALID, never by reading outside the arrays -- and a fat leaf that must not.
static void prepare(const std::string& path, bool skip_unknown, bool malformed) {
    mi355rt_load_overrides ov{}; ov.width = 16; ov.height = 12; ov.samples_per_pixel = 1; ov.max_depth = 3; ov.skip_unknown_primitives = skip_unknown;
    mi355rt_loaded_scene* ls = nullptr;
    if (mi355rt_scene_load_json(path.c_str(), &ov, &ls) != MI355RT_OK) { expect(false, path + " should load for prepare_scene"); return; }
    const mi355rt_scene base = *mi355rt_loaded_scene_get(ls);
    mi355rt::PreparedScene ps;
    expect(mi355rt::prepare_scene(&base, ps) == MI355RT_OK, path + " should prepare: " + mi355rt::last_error());
    expect(ps.prims.size() == base.n_primitives && ps.nodes.size() >= base.n_nodes, path + ": prepared sizes");
    if (malformed && base.n_meshes >= 1 && base.meshes[0].triangle_count > 2 * mi355rt::NODE_MAX_LEAF) {
        // a private copy of everything a case changes, exactly as long as the scene says: a read past an end is a sanitizer report
        std::vector<mi355rt_primitive> prims(base.primitives, base.primitives + base.n_primitives);
        std::vector<mi355rt_material> mats(base.materials, base.materials + base.n_materials);
        std::vector<mi355rt_mesh> meshes(base.meshes, base.meshes + base.n_meshes);
        std::vector<mi355rt_bvh_node> nodes(base.nodes, base.nodes + base.n_nodes);
        std::vector<uint32_t> idx(base.tri_indices, base.tri_indices + base.n_tri_indices);
        auto attempt = [&](const char* what, int want, const mi355rt_scene* edited = nullptr) {
            mi355rt_scene sc = edited ? *edited : base;
            sc.primitives = prims.data(); sc.materials = mats.data(); sc.meshes = meshes.data(); sc.nodes = nodes.data(); sc.tri_indices = idx.data();
            mi355rt::PreparedScene out;
            const int rc = mi355rt::prepare_scene(&sc, out);
            expect(rc == want, std::string("prepare_scene, ") + what + ": returned " + std::to_string(rc) + " (" + mi355rt::last_error() + ")");
            return out.nodes.size();
        };
        const mi355rt_mesh mesh0 = meshes[0];
        mi355rt_bvh_node& root = nodes[mesh0.first_node];
        const mi355rt_bvh_node root0 = root;
        size_t leaf = mesh0.first_node; while (nodes[leaf].index_count == 0) ++leaf;                     // (a tree has leaves)
        const mi355rt_bvh_node leaf0 = nodes[leaf];
        expect(root0.index_count == 0, "the shipped mesh has an inner root");
        root.left = mesh0.node_count + 7;                  attempt("child index out of range", MI355RT_ERR_INVALID); root = root0;
        root.left = 0xFFFFFFFFu;                           attempt("child index 2^32 - 1", MI355RT_ERR_INVALID); root = root0;
        root.left = 0;                                     attempt("cycle", MI355RT_ERR_INVALID); root = root0;
        root.right = root.left;                            attempt("shared child", MI355RT_ERR_INVALID); root = root0;
        nodes[leaf].first_index = mesh0.index_count;       attempt("leaf index range past the mesh", MI355RT_ERR_INVALID); nodes[leaf] = leaf0;
        nodes[leaf].first_index = 0xFFFFFFFFu;             attempt("leaf index range wraps", MI355RT_ERR_INVALID); nodes[leaf] = leaf0;
        nodes[leaf].index_count = 0xFFFFFFFFu;             attempt("leaf count 2^32 - 1", MI355RT_ERR_INVALID); nodes[leaf] = leaf0;
        { const uint32_t k = mesh0.first_index + leaf0.first_index, old = idx[k]; idx[k] = 1000000u; attempt("leaf triangle id", MI355RT_ERR_INVALID); idx[k] = old; }
        meshes[0].node_count = 0;                          attempt("mesh with node_count 0", MI355RT_ERR_INVALID); meshes[0] = mesh0;
        meshes[0].node_count = base.n_nodes + 5;           attempt("mesh node range", MI355RT_ERR_INVALID); meshes[0] = mesh0;
        meshes[0].first_node = 0xFFFFFFFFu;                attempt("mesh node range wraps", MI355RT_ERR_INVALID); meshes[0] = mesh0;
        meshes[0].triangle_count = base.n_triangles + 1;   attempt("mesh triangle range", MI355RT_ERR_INVALID); meshes[0] = mesh0;
        meshes[0].index_count = base.n_tri_indices + 1;    attempt("mesh index range", MI355RT_ERR_INVALID); meshes[0] = mesh0;
        int spheres = 0, mesh_prims = 0;
        for (size_t i = 0; i < prims.size(); ++i) {
            const mi355rt_primitive p0 = prims[i];
            if (p0.kind == MI355RT_PRIM_SPHERE) { prims[i].data[3] = 9.9e-5f; attempt("sphere radius", MI355RT_ERR_INVALID); ++spheres; }
            if (p0.kind == MI355RT_PRIM_MESH) { prims[i].mesh = base.n_meshes; attempt("primitive mesh index", MI355RT_ERR_INVALID); ++mesh_prims; }
            prims[i] = p0;
        }
        expect(spheres >= 1 && mesh_prims >= 1, path + ": the sphere-radius and mesh-index cases need a sphere and a mesh primitive");
        { const mi355rt_primitive p0 = prims[0];
          prims[0].material = base.n_materials; attempt("primitive material index", MI355RT_ERR_INVALID); prims[0] = p0;
          prims[0].kind = 17;                   attempt("primitive kind", MI355RT_ERR_INVALID); prims[0] = p0; }
        { const mi355rt_material m0 = mats[0];
          mats[0].kind = 99;                    attempt("material kind", MI355RT_ERR_INVALID); mats[0] = m0;
          mats[0].kind = MI355RT_MAT_TEXTURE; mats[0].texture = base.n_textures; attempt("texture index", MI355RT_ERR_INVALID); mats[0] = m0; }
        { mi355rt_scene sky = base; sky.sky_rgb = nullptr; sky.sky_width = 4; sky.sky_height = 2; attempt("sky size without pixels", MI355RT_ERR_INVALID, &sky); }
        { const float px[24] = {}; mi355rt_scene sky = base; sky.sky_rgb = px; sky.sky_width = 4; sky.sky_height = 0; attempt("sky pixels with one dimension", MI355RT_ERR_INVALID, &sky); }
        attempt("the restored scene", MI355RT_OK);                                                            // (everything restored: the scene prepares again)
        expect(mi355rt::prepare_scene(nullptr, ps) == MI355RT_ERR_INVALID, "prepare_scene(null)");
        // a fat leaf: the whole first mesh under one leaf -> a root and a chain of ceil(n / NODE_MAX_LEAF) chunk leaves
        mi355rt_bvh_node fat = root0; fat.left = fat.right = 0; fat.first_index = 0; fat.index_count = mesh0.triangle_count;
        nodes.push_back(fat);
        meshes[0].first_node = (uint32_t)nodes.size() - 1; meshes[0].node_count = 1;
        meshes[0].first_index = (uint32_t)idx.size(); meshes[0].index_count = mesh0.triangle_count;
        for (uint32_t t = 0; t < mesh0.triangle_count; ++t) idx.push_back(t);
        mi355rt_scene grown = base; grown.n_nodes = (uint32_t)nodes.size(); grown.n_tri_indices = (uint32_t)idx.size();
        size_t others = 0; for (uint32_t m = 1; m < base.n_meshes; ++m) others += meshes[m].node_count;
        const size_t n = attempt("fat leaf", MI355RT_OK, &grown);
        expect(n == others + 1 + (mesh0.triangle_count + mi355rt::NODE_MAX_LEAF - 1) / mi355rt::NODE_MAX_LEAF, "fat leaf: a root and its chunk chain");
    } else if (malformed) expect(false, path + ": no mesh to deform");
    mi355rt_scene_free(ls);
}

// The plan of a render call (rt_prepare.cpp plan_render, halve_bands, render_band, row_tables) at the ends of what check_settings admits: 64-bit
// arithmetic with 32-bit results next to the 2^31 limits.  Every band of every plan is walked; the bands must tile the selection, a band's samples
// stay below 2^31, its shards cover it and its grid stays within the slots.
static void plan(const mi355rt_settings& st, const mi355rt_options* opt, uint32_t s0, uint32_t s1, uint32_t variant, uint32_t slots, const std::string& what) {
    using namespace mi355rt;
    expect(check_settings(&st) == MI355RT_OK, what + ": settings");
    uint32_t block_slots[KERNEL_VARIANTS]; for (uint32_t& v : block_slots) v = slots;
    for (int probe = 0; probe < (st.height > 100000u ? 1 : 2); ++probe) {                      // (16 M rows: the row probe's plan is skipped, a probe has 96 rows)
        const RenderPlanIn in{&st, opt, s0, s1, s0 != 0, variant, true, 3u, true, probe != 0, block_slots, probe ? 16u : 1u, probe ? 64u : 1u};
        RowSel sel; RenderPlan p;
        const int rc = plan_render(in, sel, p);
        const uint64_t ws = opt && opt->workspace_bytes ? opt->workspace_bytes : ~0ull;
        expect(rc == (ws / 12 < (uint64_t)s1 - s0 && !sel.rows.empty() ? MI355RT_ERR_INVALID : MI355RT_OK), what + ": plan_render returned " + std::to_string(rc) + " (" + last_error() + ")");
        if (rc != MI355RT_OK) continue;
        expect(p.total_pixels == (uint64_t)sel.rows.size() * st.width && (p.n_bands == 0u) == sel.rows.empty(), what + ": pixels");
        if (sel.rows.empty() || VARIANT_TABLE[p.variant].block_threads == 0u) continue;     // nothing to launch; a retired variant
        if (!probe && sel.rows.size() <= 100000u) {
            std::vector<float> cost(st.height); for (uint32_t y = 0; y < st.height; ++y) cost[y] = (float)(y % 7u);
            std::vector<uint32_t> tables;
            row_tables(sel.rows, cost, p.order_groups, tables);
            expect(tables.size() == 3 * sel.rows.size(), what + ": tables");
        }
        for (int halvings = 0; ; ++halvings) {
            // every band when they are few; otherwise the first and the last 100 000 (a one-pixel band of the largest image: 2^31 of them)
            uint64_t next = 0; bool ok = p.n_bands >= 1 && p.band_pixels >= 1;
            for (uint32_t b = 0; b < p.n_bands; ++b) {
                if (p.n_bands > 200000u && b == 100000u) { b = p.n_bands - 100000u; next = (uint64_t)b * p.band_pixels; }
                const RenderBand r = render_band(p, b);
                ok = ok && r.band_pixel0 == next && r.band_pixels >= 1 && r.band_pixels <= p.band_pixels && 
                     (probe || (r.band_samples == (uint64_t)r.band_pixels * p.spp && r.band_samples < (1u << 31))) && (uint64_t)WORK_SHARDS * r.shard_samples >= r.band_samples && r.grid >= 1 && r.grid <= p.resident && r.guided_div >= 1;
                next += r.band_pixels;
            }
            expect(ok && next == p.total_pixels, what + ": bands after " + std::to_string(halvings) + " halvings" + (probe ? " (row probe)" : ""));
            const uint64_t before = p.band_pixels;
            if (!halve_bands(p)) { expect(probe || before == 1, what + ": halving ends at one pixel"); break; }
            expect(!probe && p.band_pixels == (before + 1) / 2, what + ": halving");
        }
    }
}

static void plan_cases() {
    using namespace mi355rt;
    const uint32_t SPP_MAX = (1u << 30) - 1u, SIDE_MAX = (1u << 24) - 1u;
    const mi355rt_settings sizes[] = {{1, 1, 1, 1}, {1, 1, SPP_MAX, 0}, {SIDE_MAX, 128, 1, 5}, {128, SIDE_MAX, SPP_MAX, 5}, {46340, 46340, 4096, 30}, {SIDE_MAX, 1, 7, 1}, {33, 35, 3, 6}};
    for (const mi355rt_settings& st : sizes) {
        const std::string size = std::to_string(st.width) + "x" + std::to_string(st.height) + "x" + std::to_string(st.samples_per_pixel);
        for (uint64_t ws : {0ull, 1ull, 12ull, ~0ull}) {
            mi355rt_options o{}; o.abi_version = MI355RT_ABI_VERSION; o.rng_mode = MI355RT_RNG_CTR; o.workspace_bytes = ws; o.seed = ~0ull;
            for (uint32_t v = 0; v < KERNEL_VARIANTS; v += st.height > 100000u ? 13u : 1u) {   // (16 M rows: two variants, a lockstep and a wavefront kernel)
                o.flags = v & 1u ? MI355RT_FLAG_FIXED_AABB : 0u;
                plan(st, &o, 0, st.samples_per_pixel, v, v & 2u ? 0xFFFFFFFFu : 1u, "plan " + size + " ws " + std::to_string(ws) + " variant " + std::to_string(v));
            }
            plan(st, &o, SPP_MAX - 1u, SPP_MAX, KERNEL_LOCKSTEP_SIMPLE_QC, 1024u, "plan " + size + " ws " + std::to_string(ws) + ": one sample at a large s0");
            mi355rt_options row = o; row.row_begin = st.height - 1u; row.row_end = st.height;
            plan(st, &row, 0, st.samples_per_pixel, KERNEL_WAVEFRONT_MESHFREE, 512u, "plan " + size + " ws " + std::to_string(ws) + ": a window of one row");
            mi355rt_options none = o; none.strip_rows = st.height; none.n_parts = 2; none.part = 1;
            plan(st, &none, 0, st.samples_per_pixel, KERNEL_LOCKSTEP, 512u, "plan " + size + " ws " + std::to_string(ws) + ": a part that is dealt no strip");
        }
        plan(st, nullptr, 0, st.samples_per_pixel, KERNEL_WAVEFRONT_NOMETAL, 512u, "plan " + size + " without options");
    }
    const mi355rt_settings st{33, 35, 3, 6};
    mi355rt_options o{}; o.abi_version = MI355RT_ABI_VERSION; o.rng_mode = MI355RT_RNG_REF;
    uint32_t slots[KERNEL_VARIANTS] = {};
    RowSel sel; RenderPlan p;
    expect(plan_render(RenderPlanIn{&st, &o, 0, 3, false, KERNEL_LOCKSTEP, false, 0, true, false, slots, 1, 16}, sel, p) == MI355RT_OK && p.n_bands == 1 && p.order_groups == 0, "plan: the replay mode");
    expect(plan_render(RenderPlanIn{&st, &o, 1, 3, true, KERNEL_LOCKSTEP, false, 0, true, false, slots, 1, 16}, sel, p) == MI355RT_ERR_INVALID, "plan: progressive in the replay mode");
    o.flags = 2u; expect(plan_render(RenderPlanIn{&st, &o, 0, 3, false, KERNEL_LOCKSTEP, false, 0, true, false, slots, 1, 16}, sel, p) == MI355RT_ERR_INVALID, "plan: unknown flag bits");
    for (uint32_t d : {1u, 2u, 3u, 255u, 256u, SIDE_MAX, SPP_MAX, 0x80000000u, 0xFFFFFFFFu}) { uint32_t mul = 1, shift = 1; magic_div(d, mul, shift); expect(shift < 32u && (d > 1u) == (mul != 0u), "magic_div " + std::to_string(d)); }
}

static std::string scene_with(const std::string& prim) {
    return std::string("{\"bsdfs\":[{\"name\":\"m\",\"type\":\"lambert\",\"albedo\":[0.5,0.5,0.5]}],\"primitives\":[") + prim +
           "],\"camera\":{\"transform\":{\"position\":[0,0,5],\"look_at\":[0,0,0],\"up\":[0,1,0]},\"fov\":40,\"resolution\":[8,8]},\"renderer\":{\"spp\":1},\"integrator\":{\"max_bounces\":2}}";
}
static std::string mesh_prim(const std::string& file) { return "{\"type\":\"mesh\",\"file\":\"" + file + "\",\"bsdf\":\"m\",\"transform\":{}}"; }

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: driver <repo root> <scratch dir>\n"); return 2; }
    const std::string root = argv[1], tmp = argv[2];

    // ---- the shipped scenes ----
    load(root + "/data/scenes/tungsten/cornell-box/scene.json", true);
    load(root + "/data/scenes/tungsten/veach-mis/scene.json", true);
    load(root + "/data/scenes/semesterbild.json", true);
    load(root + "/data/scenes/tungsten/teapot/scene.json", true, 16, 12, true);
    load(root + "/data/scenes/tungsten/teapot/scene.json", false);            // infinite_sphere: an unknown primitive type is a load error
    load(root + "/no/such/file.json", false);

    // ---- scene preparation (what mi355rt_context_set_scene does before it touches a device) ----
    prepare(root + "/data/scenes/tungsten/cornell-box/scene.json", false, false);
    prepare(root + "/data/scenes/tungsten/veach-mis/scene.json", false, false);
    prepare(root + "/data/scenes/tungsten/teapot/scene.json", true, false);
    prepare(root + "/data/scenes/semesterbild.json", false, true);

    // ---- the plan of a render call (what mi355rt_context_render decides before it touches a device) ----
    plan_cases();

    // ---- malformed JSON ----
    const char* bad_json[] = {"", "{", "[", "{\"a\":}", "{\"a\":1,}", "nul", "{\"a\":1} x", "\"\\u12", "\"abc", "{\"a\":01}", "{\"a\":1.}", "{\"a\":.5}",
                              "{\"a\":1e}", "{\"a\":0x10}", "{\"a\":-}", "{\"a\":-inf}", "{\"a\":nan}", "{\"a\":\"\\q\"}", "{1:2}", "[1 2]"};
    for (size_t i = 0; i < sizeof bad_json / sizeof bad_json[0]; ++i) { const std::string p = tmp + "/bad" + std::to_string(i) + ".json"; put(p, bad_json[i]); load(p, false); }
    { std::string deep(200000, '['); put(tmp + "/deep.json", deep); load(tmp + "/deep.json", false); }
    { std::string deep; for (int i = 0; i < 100000; ++i) deep += "{\"a\":"; put(tmp + "/deep2.json", deep); load(tmp + "/deep2.json", false); }
    // well-formed JSON, wrong content
    put(tmp + "/empty_obj.json", "{}"); load(tmp + "/empty_obj.json", false);
    put(tmp + "/arr.json", "[1,2,3]"); load(tmp + "/arr.json", false);
    const char* bad_res[] = {"-1", "1.5", "1e3", "\"800\"", "[800,\"a\"]", "4294967296", "[1.5,2]", "{\"w\":1}"};
    for (size_t i = 0; i < sizeof bad_res / sizeof bad_res[0]; ++i) {
        std::string s = scene_with("");
        const std::string from = "\"resolution\":[8,8]";
        s.replace(s.find(from), from.size(), std::string("\"resolution\":") + bad_res[i]);
        const std::string p = tmp + "/res" + std::to_string(i) + ".json"; put(p, s);
        mi355rt_loaded_scene* ls = nullptr;
        expect(mi355rt_scene_load_json(p.c_str(), nullptr, &ls) != MI355RT_OK, std::string("resolution ") + bad_res[i] + " should be refused");
        if (ls) mi355rt_scene_free(ls);
    }
    { std::string s = scene_with(""); const std::string from = "\"spp\":1"; s.replace(s.find(from), from.size(), "\"spp\":2.5"); put(tmp + "/spp.json", s);
      mi355rt_loaded_scene* ls = nullptr; expect(mi355rt_scene_load_json((tmp + "/spp.json").c_str(), nullptr, &ls) != MI355RT_OK, "spp 2.5 should be refused"); if (ls) mi355rt_scene_free(ls); }
    put(tmp + "/ok_empty.json", scene_with("")); load(tmp + "/ok_empty.json", true);
    put(tmp + "/res3.json", [&] { std::string s = scene_with(""); const std::string from = "\"resolution\":[8,8]"; s.replace(s.find(from), from.size(), "\"resolution\":[1,2,3]"); return s; }());
    load(tmp + "/res3.json", false);                                           // Explicit([usize; 2]), parser.rs:69-72: three elements match no variant of the untagged enum

    // ---- OBJ ----
    struct Case { const char* name; std::string body; bool ok; };
    const std::string tri = "v 0 0 0\nv 1 0 0\nv 0 1 0\n";
    const Case objs[] = {
        {"good", tri + "f 1 2 3\n", true}, {"neg", tri + "f -3 -2 -1\n", true}, {"slashes", tri + "vt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3//1\n", true},
        {"quad", tri + "v 1 1 0\nf 1 2 4 3\n", true}, {"crlf", "v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 3\r\n", true},
        {"novert", "f 1 2 3\n", false}, {"zero", tri + "f 0 1 2\n", false}, {"oob", tri + "f 1 2 4\n", false}, {"negoob", tri + "f -4 -2 -1\n", false},
        {"huge", tri + "f 1 2 99999999999999999999\n", false}, {"word", tri + "f 1 x 3\n", false}, {"shortv", "v 1 2\nf 1 1 1\n", false},
        {"line", tri + "f 1 2\n", false}, {"nofaces", tri, false}, {"empty", "", false}, {"degenerate_only", tri + "f 1 1 1\n", false},
    };
    // A mesh that fails to load is reported and DROPPED, the scene itself loads (parser.rs:685-698): `ok` = the mesh survives.
    for (const Case& c : objs) {
        put(tmp + "/" + c.name + ".obj", c.body);
        put(tmp + "/obj_" + c.name + ".json", scene_with(mesh_prim(std::string(c.name) + ".obj")));
        load(tmp + "/obj_" + std::string(c.name) + ".json", true);
        expect(g_last_prims == (c.ok ? 1u : 0u), std::string("OBJ case ") + c.name + (c.ok ? " should yield a mesh" : " should drop the mesh"));
    }
    put(tmp + "/obj_missing.json", scene_with(mesh_prim("does_not_exist.obj"))); load(tmp + "/obj_missing.json", true);
    expect(g_last_prims == 0u, "missing OBJ should drop the mesh");

    // ---- WO3 ----
    auto vert = [&](float x, float y, float z) { return f32s(x) + f32s(y) + f32s(z) + f32s(0) + f32s(0) + f32s(1) + f32s(0) + f32s(0); };
    const std::string v3 = vert(0, 0, 0) + vert(1, 0, 0) + vert(0, 1, 0);
    const Case wo3s[] = {
        {"good", u64(3) + v3 + u64(1) + u32(0) + u32(1) + u32(2) + u32(0), true},
        {"empty", "", false}, {"short", "abcd", false}, {"hugenv", u64(1ull << 60), false}, {"truncv", u64(3) + vert(0, 0, 0), false},
        {"nohdr2", u64(3) + v3, false}, {"hugent", u64(3) + v3 + u64(1ull << 61), false}, {"trunci", u64(3) + v3 + u64(2) + u32(0) + u32(1) + u32(2), false},
        {"oobidx", u64(3) + v3 + u64(1) + u32(0) + u32(1) + u32(7) + u32(0), false},        // every triangle skipped -> empty mesh -> error
        {"nvwrap", u64(0x0800000000000001ull) + v3, false},                                     // nv * 32 wraps around 2^64
    };
    for (const Case& c : wo3s) {
        put(tmp + "/" + c.name + ".wo3", c.body);
        put(tmp + "/wo3_" + c.name + ".json", scene_with(mesh_prim(std::string(c.name) + ".wo3")));
        load(tmp + "/wo3_" + std::string(c.name) + ".json", true);
        expect(g_last_prims == (c.ok ? 1u : 0u), std::string("WO3 case ") + c.name + (c.ok ? " should yield a mesh" : " should drop the mesh"));
    }

    // ---- Radiance HDR (sky.texture): a load error keeps the default background, so every scene loads; the reader must not crash ----
    auto sky_scene = [&](const std::string& file) { std::string s = scene_with(""); s.insert(1, "\"sky\":{\"texture\":\"" + file + "\"},"); return s; };
    const std::string hdr_head = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n";
    const std::string px4 = std::string("\x80\x40\x20\x81", 4);
    const Case hdrs[] = {
        {"flat", hdr_head + "-Y 2 +X 2\n" + px4 + px4 + px4 + px4, true}, {"notrad", "P6\n1 1\n255\n", false}, {"nores", hdr_head, false},
        {"negdim", hdr_head + "-Y -2 +X 2\n", false}, {"hugedim", hdr_head + "-Y 2147483647 +X 2147483647\n", false}, {"bigdim", hdr_head + "-Y 16000 +X 16000\n", false},
        {"truncflat", hdr_head + "-Y 2 +X 2\n" + px4, false},
        {"rle", hdr_head + "-Y 1 +X 8\n" + std::string("\x02\x02\x00\x08", 4) + std::string("\x88\x10", 2) + std::string("\x88\x20", 2) + std::string("\x88\x30", 2) + std::string("\x88\x80", 2), true},
        {"rlelong", hdr_head + "-Y 1 +X 8\n" + std::string("\x02\x02\x00\x08", 4) + std::string("\xff\x10", 2) + std::string(40, '\x01'), false},  // run of 127 > width
        {"rlezero", hdr_head + "-Y 1 +X 8\n" + std::string("\x02\x02\x00\x08", 4) + std::string(40, '\x00'), false},                              // literal of length 0
        {"rletrunc", hdr_head + "-Y 1 +X 8\n" + std::string("\x02\x02\x00\x08", 4) + std::string("\x05\x01\x02", 3), false},                     // literal longer than the file
        {"orient", hdr_head + "+Y 2 +X 2\n" + px4 + px4 + px4 + px4, false},
    };
    for (const Case& c : hdrs) {
        put(tmp + "/" + c.name + ".hdr", c.body);
        put(tmp + "/hdr_" + c.name + ".json", sky_scene(std::string(c.name) + ".hdr"));
        load(tmp + "/hdr_" + std::string(c.name) + ".json", true);                    // `ok` = the skybox survives; the scene always loads
        expect((g_last_sky != 0u) == c.ok, std::string("HDR case ") + c.name + (c.ok ? " should yield a skybox" : " should fall back to the default background"));
    }

    // ---- BVH build: ties, NaNs, one triangle, many equal centroids ----
    {
        std::vector<mi355rt_triangle> t;
        for (int i = 0; i < 300; ++i) {
            mi355rt_triangle x{}; const float o = (float)(i % 7);
            x.v0[0] = o; x.v1[0] = o + 1; x.v2[1] = 1; x.normal[2] = 1;
            if (i % 41 == 0) x.v0[1] = std::nanf("");
            t.push_back(x);
        }
        for (uint32_t n : {1u, 4u, 5u, 300u}) {
            uint32_t nn = 0, ni = 0, md = 0;
            expect(mi355rt_bvh_build(t.data(), n, nullptr, &nn, nullptr, &ni, &md) == MI355RT_OK, "bvh_build count");
            std::vector<mi355rt_bvh_node> nodes(nn); std::vector<uint32_t> idx(ni);
            expect(mi355rt_bvh_build(t.data(), n, nodes.data(), &nn, idx.data(), &ni, &md) == MI355RT_OK, "bvh_build fill");
            uint32_t small_n = nn ? nn - 1 : 0;
            expect(nn == 0 || mi355rt_bvh_build(t.data(), n, nodes.data(), &small_n, idx.data(), &ni, &md) != MI355RT_OK, "bvh_build must refuse short arrays");
        }
        uint32_t nn = 0, ni = 0;
        expect(mi355rt_bvh_build(nullptr, 3, nullptr, &nn, nullptr, &ni, nullptr) != MI355RT_OK, "bvh_build null");
        expect(mi355rt_bvh_build(t.data(), 0, nullptr, &nn, nullptr, &ni, nullptr) != MI355RT_OK, "bvh_build empty");
    }

    // ---- writers ----
    {
        std::vector<uint32_t> px(7 * 5, 0x00FF8040u); std::vector<float> lin(7 * 5 * 3, 0.25f);
        expect(mi355rt_write_png((tmp + "/a.png").c_str(), px.data(), 7, 5) == MI355RT_OK, "write_png");
        expect(mi355rt_write_pfm((tmp + "/a.pfm").c_str(), lin.data(), 7, 5) == MI355RT_OK, "write_pfm");
        expect(mi355rt_write_exr((tmp + "/a.exr").c_str(), lin.data(), 7, 5) == MI355RT_OK, "write_exr");
        expect(mi355rt_write_exr((tmp + "/a.exr").c_str(), lin.data(), 0, 5) != MI355RT_OK, "write_exr of an empty image");
        expect(mi355rt_write_png((tmp + "/no/dir/a.png").c_str(), px.data(), 7, 5) != MI355RT_OK, "write_png to a missing directory");
        expect(mi355rt_write_png((tmp + "/z.png").c_str(), px.data(), 0, 5) != MI355RT_OK, "write_png of an empty image");
        expect(mi355rt_write_png(nullptr, px.data(), 7, 5) != MI355RT_OK, "write_png null path");
    }

    // ---- the noise estimate: exact buffer sizes (a read or write past rows * width * 4 floats / rows * width floats is a report), non-finite and huge sums ----
    {
        const uint32_t W = 13, R = 7; const size_t n = (size_t)W * R;
        mi355rt_noise_state* s = nullptr; mi355rt_noise_summary sum{};
        expect(mi355rt_noise_create(0, R, &s) == MI355RT_ERR_INVALID && !s, "noise_create width 0");
        expect(mi355rt_noise_create(1u << 16, 1u << 15, &s) == MI355RT_ERR_INVALID && !s, "noise_create 2^31 pixels");
        expect(mi355rt_noise_create(W, R, &s) == MI355RT_OK && s, "noise_create");
        std::vector<float> acc(n * 4, 0.0f), err(n, -1.0f);
        expect(mi355rt_noise_evaluate(s, nullptr, err.data(), &sum) == MI355RT_ERR_INVALID, "noise_evaluate before any chunk");
        for (uint32_t k = 1; k <= 5; ++k) {
            for (size_t p = 0; p < n; ++p) for (int c = 0; c < 3; ++c) acc[4 * p + c] += (float)((p * 7 + c * 3 + k * k) % 11) * 0.125f * (float)k;
            acc[4 * 3 + 1] = k > 2 ? INFINITY : acc[4 * 3 + 1]; acc[4 * 5] = k > 3 ? NAN : acc[4 * 5]; acc[4 * 6 + 2] = 3.0e38f; acc[4 * 8] = -(float)k;
            expect(mi355rt_noise_update(s, acc.data(), k * 3 + (k > 2 ? 5 : 0)) == MI355RT_OK, "noise_update");
            expect(mi355rt_noise_update(s, acc.data(), k * 3) == MI355RT_ERR_INVALID, "noise_update with samples_total not increasing");
            if (k >= 2) expect(mi355rt_noise_evaluate(s, nullptr, k & 1 ? err.data() : nullptr, &sum) == MI355RT_OK && sum.chunks == k && sum.pixels == n, "noise_evaluate");
        }
        expect(sum.nonfinite == 2 && std::isnan(err[3]) && std::isnan(err[5]) && err[0] >= 0.0f, "noise_evaluate: two non-finite pixels");
        mi355rt_noise_params pr = {0.5, 0.0, 2u, 0u, n};
        expect(mi355rt_noise_evaluate(s, &pr, err.data(), &sum) == MI355RT_OK && sum.converged == 1u, "noise_evaluate with floor 0");
        pr._pad = 7u; expect(mi355rt_noise_evaluate(s, &pr, err.data(), &sum) == MI355RT_ERR_INVALID, "noise_evaluate with a pad");
        expect(mi355rt_noise_reset(s) == MI355RT_OK && mi355rt_noise_evaluate(s, nullptr, nullptr, &sum) == MI355RT_ERR_INVALID, "noise_reset");
        mi355rt_noise_free(s); mi355rt_noise_free(nullptr);
    }
    std::printf(g_fail ? "sanitize driver: %d unexpected result(s)\n" : "sanitize driver: all cases behaved (%d unexpected)\n", g_fail);
    return g_fail ? 1 : 0;
}
