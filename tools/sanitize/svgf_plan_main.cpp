// svgf_plan_main.cpp -- a program of its own for tests/test_svgf_cpu.py: this main and raytracer-rust_amd/csrc/svgf/svgf_plan.cpp, plain g++ with
// -fsanitize=address,undefined, run directly.  It drives plan_accumulate, plan_filter and plan_scratch_bytes (the HIP-free half of
// libmi355rt_svgf.so) over valid calls, whose geometry it checks, and over the table of refusals, each of which must return MI355RT_ERR_INVALID
// with a text that starts with the call's name and names the argument.  The buffers it passes are never read.  Prints "ok <n> checks" or what failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../raytracer-rust_amd/csrc/svgf/svgf_plan.h"

using namespace mi355rt_svgf;

static int failures = 0, checked = 0;
static void expect(bool ok, const char* what, const std::string& why) { ++checked; if (!ok) { ++failures; std::printf("FAILED %s: %s\n", what, why.c_str()); } }

struct Acc { int dev; mi355rt_view cur, prev; bool has_prev; mi355rt_svgf_accumulate_params p; bool has_p; char *hc, *cc, *hp, *mp, *mmp, *ho, *mo, *vo; };
struct Fil { int dev; uint32_t W, H; mi355rt_svgf_filter_params p; bool has_p; char *hist, *var, *hits, *scr, *ol, *op; };

static int run(const Acc& a, AccumulatePlan& plan, std::string& why) {
    return plan_accumulate(a.dev, &a.cur, a.has_prev ? &a.prev : nullptr, a.has_p ? &a.p : nullptr, a.hc, a.cc, a.hp, a.mp, a.mmp, a.ho, a.mo, a.vo, plan, why);
}
static int run(const Fil& f, FilterPlan& plan, std::string& why) { return plan_filter(f.dev, f.W, f.H, f.has_p ? &f.p : nullptr, f.hist, f.var, f.hits, f.scr, f.ol, f.op, plan, why); }

int main() {
    alignas(64) static char buf[8192];                       // never read: every decision is taken from the arguments alone
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mi355rt_view v; std::memset(&v, 0, sizeof v);
    v.model = MI355RT_VIEW_PINHOLE; v.width = 70; v.height = 17;
    v.camera.forward[2] = 1.0f; v.camera.right[0] = 1.0f; v.camera.true_up[1] = 1.0f; v.camera.half_width = v.camera.half_height = 1.0f;
    const Acc ok{0, v, v, true, {32u, 0u, 0.9f, 0.05f, 4u, 5u, 0.05f, 0u}, true, buf, buf + 512, buf + 1024, buf + 1536, buf + 2048, buf + 2560, buf + 3072, buf + 3584};
    const Fil fok{0, 70u, 17u, {5u, 5u, 1.0f, 0.05f, 0u, 0u}, true, buf, buf + 512, buf + 1024, buf + 1536, buf + 2048, buf + 2560};
    std::string why;
    AccumulatePlan ap; FilterPlan fp;
    // ---- valid calls and their geometry (10 checks)
    expect(run(ok, ap, why) == MI355RT_OK && ap.k.tiles_x == 3u && ap.k.n_tiles == 9u && ap.grid == 9u && ap.k.has_prev == 1u && ap.k.min_temporal_f == 4.0f, "a valid accumulate", why);
    { Acc a = ok; a.has_p = false; expect(run(a, ap, why) == MI355RT_OK && ap.k.max_history_f == 32.0f && ap.k.normal_squarings == 5u, "accumulate, default params", why); }
    { Acc a = ok; a.has_prev = false; a.hp = a.mp = a.mmp = nullptr; expect(run(a, ap, why) == MI355RT_OK && ap.k.has_prev == 0u && ap.k.prev_width == 0u, "accumulate without prev", why); }
    expect(run(fok, fp, why) == MI355RT_OK && fp.tiles_x == 3u && fp.n_tiles == 9u && fp.grid == 9u && fp.grid_px == 5u && fp.staged && fp.sl2 == 1.0f, "a valid filter", why);
    { Fil f = fok; f.has_p = false; f.ol = nullptr; expect(run(f, fp, why) == MI355RT_OK && fp.levels == 5u && fp.staged, "filter, default params, packed alone", why); }
    { Fil f = fok; f.p.flags = MI355RT_SVGF_GATHERS_ONLY; f.p.levels = 0u; expect(run(f, fp, why) == MI355RT_OK && !fp.staged && fp.levels == 0u, "filter, gathers only", why); }
    { Fil f = fok; f.W = 1u << 20; f.H = (1u << 11) - 1u; expect(run(f, fp, why) == MI355RT_OK && fp.n_tiles == (1u << 15) * 256u && fp.grid == MAX_BLOCKS, "the largest frame", why); }
    { Fil f = fok; f.ol = f.hist; expect(run(f, fp, why) == MI355RT_OK, "filter with levels, d_out_linear == d_hist_in", why); }
    uint64_t bytes = 1;
    expect(plan_scratch_bytes(70u, 17u, &bytes, why) == MI355RT_OK && bytes == 70u * 17u * 64u, "scratch bytes", why);
    expect(plan_scratch_bytes(1u << 16, 1u << 15, &bytes, why) == MI355RT_ERR_INVALID && bytes == 0u && why.find("2^31") != std::string::npos, "scratch bytes of a frame too large", why);
    expect(plan_scratch_bytes(4u, 4u, nullptr, why) == MI355RT_ERR_INVALID && why.find("out_bytes") != std::string::npos, "scratch bytes without a result", why);
    // ---- the refusals of accumulate (41 checks)
    const std::vector<std::pair<const char*, std::function<void(Acc&)>>> refusals = {
        {"cur.model", [](Acc& a) { a.cur.model = 7; }}, {"prev.width", [](Acc& a) { a.prev.width = 0; }}, {"cur.height", [](Acc& a) { a.cur.height = 0; }},
        {"cur.camera", [&](Acc& a) { a.cur.camera.position[1] = nan; }}, {"prev.camera", [&](Acc& a) { a.prev.camera.half_height = inf; }},
        {"cur.width * cur.height", [](Acc& a) { a.cur.width = 1u << 16; a.cur.height = 1u << 15; }},
        {"params.max_history", [](Acc& a) { a.p.max_history = 0; }}, {"params.max_history", [](Acc& a) { a.p.max_history = 65536; }}, {"params.flags", [](Acc& a) { a.p.flags = 1; }},
        {"params.normal_min", [&](Acc& a) { a.p.normal_min = nan; }}, {"params.normal_min", [](Acc& a) { a.p.normal_min = 1.5f; }},
        {"params.plane_tolerance", [](Acc& a) { a.p.plane_tolerance = 0.0f; }}, {"params.plane_tolerance", [&](Acc& a) { a.p.plane_tolerance = inf; }},
        {"params.min_temporal", [](Acc& a) { a.p.min_temporal = 0; }}, {"params.min_temporal", [](Acc& a) { a.p.min_temporal = 33; }},
        {"params.normal_squarings", [](Acc& a) { a.p.normal_squarings = 9; }}, {"params.sigma_plane", [&](Acc& a) { a.p.sigma_plane = nan; }},
        {"params.sigma_plane", [](Acc& a) { a.p.sigma_plane = -1.0f; }}, {"params.reserved", [](Acc& a) { a.p.reserved = 1; }},
        {"d_hits_cur is null", [](Acc& a) { a.hc = nullptr; }}, {"d_color_cur is null", [](Acc& a) { a.cc = nullptr; }}, {"d_hist_out is null", [](Acc& a) { a.ho = nullptr; }},
        {"d_moments_out is null", [](Acc& a) { a.mo = nullptr; }}, {"d_variance_out is null", [](Acc& a) { a.vo = nullptr; }},
        {"d_hits_cur must be 16-byte", [](Acc& a) { a.hc += 8; }}, {"d_color_cur must be 4-byte", [](Acc& a) { a.cc += 2; }}, {"d_hist_out must be 16-byte", [](Acc& a) { a.ho += 4; }},
        {"d_moments_out must be 8-byte", [](Acc& a) { a.mo += 4; }}, {"d_variance_out must be 4-byte", [](Acc& a) { a.vo += 1; }},
        {"d_hits_prev is null", [](Acc& a) { a.hp = nullptr; }}, {"d_hist_prev is null", [](Acc& a) { a.mp = nullptr; }}, {"d_moments_prev is null", [](Acc& a) { a.mmp = nullptr; }},
        {"d_hits_prev must be 16-byte", [](Acc& a) { a.hp += 4; }}, {"d_hist_prev must be 16-byte", [](Acc& a) { a.mp += 8; }}, {"d_moments_prev must be 8-byte", [](Acc& a) { a.mmp += 4; }},
        {"d_hits_prev is given without prev", [](Acc& a) { a.has_prev = false; }}, {"d_hist_prev is given without prev", [](Acc& a) { a.has_prev = false; a.hp = nullptr; }},
        {"d_moments_prev is given without prev", [](Acc& a) { a.has_prev = false; a.hp = a.mp = nullptr; }},
        {"d_hist_out must not be d_hist_prev", [](Acc& a) { a.ho = a.mp; }}, {"d_moments_out must not be d_moments_prev", [](Acc& a) { a.mo = a.mmp; }},
        {"hip_device", [](Acc& a) { a.dev = -1; }},
    };
    for (const auto& r : refusals) {
        Acc a = ok; r.second(a);
        const int rc = run(a, ap, why);
        expect(rc == MI355RT_ERR_INVALID && why.find(r.first) != std::string::npos && why.rfind("accumulate: ", 0) == 0, r.first, why);
    }
    // ---- the refusals of filter (26 checks)
    const std::vector<std::pair<const char*, std::function<void(Fil&)>>> filter_refusals = {
        {"width is 0", [](Fil& f) { f.W = 0; }}, {"height is 0", [](Fil& f) { f.H = 0; }}, {"width * height", [](Fil& f) { f.W = 1u << 16; f.H = 1u << 15; }},
        {"params.levels", [](Fil& f) { f.p.levels = 9; }}, {"params.normal_squarings", [](Fil& f) { f.p.normal_squarings = 9; }},
        {"params.sigma_luminance", [](Fil& f) { f.p.sigma_luminance = 0.0f; }}, {"params.sigma_luminance", [&](Fil& f) { f.p.sigma_luminance = nan; }},
        {"params.sigma_luminance", [](Fil& f) { f.p.sigma_luminance = 1e30f; }}, {"params.sigma_luminance", [](Fil& f) { f.p.sigma_luminance = 1e-30f; }},
        {"params.sigma_plane", [&](Fil& f) { f.p.sigma_plane = inf; }}, {"params.flags", [](Fil& f) { f.p.flags = 2; }}, {"params.reserved", [](Fil& f) { f.p.reserved = 1; }},
        {"d_hist_in is null", [](Fil& f) { f.hist = nullptr; }}, {"d_variance_in is null", [](Fil& f) { f.var = nullptr; }}, {"d_hits is null", [](Fil& f) { f.hits = nullptr; }},
        {"d_scratch is null", [](Fil& f) { f.scr = nullptr; }}, {"both null", [](Fil& f) { f.ol = f.op = nullptr; }},
        {"d_hist_in must be 16-byte", [](Fil& f) { f.hist += 8; }}, {"d_variance_in must be 4-byte", [](Fil& f) { f.var += 2; }}, {"d_hits must be 16-byte", [](Fil& f) { f.hits += 4; }},
        {"d_scratch must be 16-byte", [](Fil& f) { f.scr += 8; }}, {"d_out_linear must be 4-byte", [](Fil& f) { f.ol += 1; }}, {"d_out_packed must be 4-byte", [](Fil& f) { f.op += 2; }},
        {"d_out_linear must not be d_hist_in", [](Fil& f) { f.p.levels = 0; f.ol = f.hist; }}, {"d_out_packed must not be d_hist_in", [](Fil& f) { f.p.levels = 0; f.op = f.hist; }},
        {"hip_device", [](Fil& f) { f.dev = -1; }},
    };
    for (const auto& r : filter_refusals) {
        Fil f = fok; r.second(f);
        const int rc = run(f, fp, why);
        expect(rc == MI355RT_ERR_INVALID && why.find(r.first) != std::string::npos && why.rfind("filter: ", 0) == 0, r.first, why);
    }
    for (size_t i = 0; i < sizeof buf; ++i) if (buf[i]) { ++failures; break; }
    std::printf("%s %d checks\n", failures ? "FAILED" : "ok", checked);
    return failures ? 1 : 0;
}
