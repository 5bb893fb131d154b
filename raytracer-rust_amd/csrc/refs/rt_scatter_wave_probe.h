// rt_scatter_wave_probe.h -- one scatter event per lane through the shipped pieces of the bounce, on whole waves whose lanes the caller chooses.
// Compiled into the tests' reference build only (included by rt_kernels_refs.hip behind rt_kernels.hip, the translation unit that defines
// unit_ball_cooperative; -DMI355RT_REFS): the product library and its kernel hash do not contain it.
//
// Every counter-mode kernel bounces a path through scatter_pre / unit_ball_cooperative / ball_finish / scatter_origin / ray_direction, called
// from shade_and_regenerate with the kernel's template arguments.  The product's per-record hook (k_debug_scatter -> surface_scatter) runs the
// sequential rejection loop instead and one combination of arguments that no counter-mode kernel launches.  Here a lane reads a record -- live
// or idle, material, face, incoming direction, hit point, normal, the path's draw address (k0, k1, x, sample, ray) -- and does what the bounce
// of shade_and_regenerate does with it, by calling those functions with the arguments of one FORM of the table below; nothing is restated.
// All 64 lanes of a wave reach unit_ball_cooperative in uniform control flow: idle lanes pass false and work for the owners, as in the kernels;
// their generator words are the record's own four words (the kernels let an idle lane's state hold anything).  No lane returns early.
// tests/test_gpu_scatter_wave.py builds the waves (owner counts and places, first accepted tries up to 16 and beyond, material mixes, records
// at the decision boundaries) and compares every output word with the oracle's sequential loop.
#pragma once

#include <vector>

#include "../device/rt_host.h"

namespace mi355rt {

struct WaveProbeIn { uint32_t material, flags; float rd[3], p[3], n[3]; uint32_t k0, k1, x, s, ray; };   // 16 words; flags: bit 0 front face, bit 8 live
struct WaveProbeOut { float scattered, o[3], d[3], atten[3], emitted[3], ball[3]; };                    // 16 words; what a lane did not produce is +0
static_assert(sizeof(WaveProbeIn) == 64 && sizeof(WaveProbeOut) == 64, "wave probe records");
constexpr uint32_t WAVE_PROBE_LIVE = 0x100u;

// IN_PLACE: the bounce of FORM_STATE_IN_PLACE (k_render_ctr_simple_qc) -- the ball for the live lanes, diffuse_finish and ray_direction by all lanes.
// RANGE: that kernel's range arithmetic (rt_math.h), as render_ctr_lockstep passes it.
template <uint32_t MATS, bool WIDE, bool FASTN, int TRY1, bool TERMINAL_DONE, bool STEP, bool IN_PLACE, uint32_t RANGE>
__global__ void __launch_bounds__(BLOCK_THREADS) k_probe_scatter_wave(const DevMat* __restrict__ mats, const WaveProbeIn* __restrict__ in, WaveProbeOut* __restrict__ out) {
    typedef RngCtrT<STEP> Rng;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;                        // (the entry pads the records to whole workgroups)
    const uint32_t lane = threadIdx.x & 63u;
    const WaveProbeIn r = in[i];
    const bool live = (r.flags & WAVE_PROBE_LIVE) != 0u;
    Hit h; h.t = 0.f; h.p = mk(r.p[0], r.p[1], r.p[2]); h.n = mk(r.n[0], r.n[1], r.n[2]);
    h.mat_ff = (live ? r.material : 0u) | ((r.flags & 1u) ? 0x80000000u : 0u);
    const f3 rd_in = mk(r.rd[0], r.rd[1], r.rd[2]);
    Rng rng;
    if (live) { rng.start(r.k0, r.k1, r.x, r.s); rng.set_ray(r.ray); }
    else { rng.w[0] = r.k0; rng.w[1] = r.k1; rng.w[2] = r.x; rng.w[3] = r.s; if constexpr (Rng::NW == 5) rng.w[4] = r.ray; }
    rng.template load_block0<WIDE>();
    uint32_t blk1[4] = {0u, 0u, 0u, 0u};
    if constexpr (TRY1 >= 1) Rng::template block<WIDE>(rng.w, 1u, blk1);
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) q0 = reinterpret_cast<const float4*>(mats + r.material)[0];
    h.q0 = q0;
    bool scattered = false, used_ball = false;
    f3 ball, org, dir, atten = mk(0.f, 0.f, 0.f), emitted = mk(0.f, 0.f, 0.f);
    if constexpr (IN_PLACE) {
        static_assert((MATS & ~MATS_LAMBERT) == 0u && TERMINAL_DONE, "the in-place bounce belongs to the Lambert-only kernel");
        atten = mk(q0.y, q0.z, q0.w);
        org = scatter_origin(h, EPS);
        rng.begin_scatter();
        ball = unit_ball_cooperative<WIDE, TRY1>(live, rng, lane, blk1);              // whole wave, uniform control flow
        dir = ray_direction<FASTN, RANGE>(diffuse_finish<FASTN, RANGE>(h, ball));
        scattered = live; used_ball = live;
    } else {
        uint32_t ball_use = BALL_NONE; float side = EPS, fuzz = 0.f; f3 raw = mk(0.f, 0.f, 1.f);
        if (live) scattered = scatter_pre<MATS, WIDE, FASTN, TERMINAL_DONE>(mats, nullptr, q0, h, rd_in, rng, side, raw, atten, emitted, ball_use, fuzz);
        used_ball = scattered && ball_use != BALL_NONE;
        ball = unit_ball_cooperative<WIDE, TRY1>(used_ball, rng, lane, blk1);         // whole wave, uniform control flow
        if (live && scattered) scattered = ball_finish<FASTN, RANGE>(ball_use, h, ball, fuzz, raw);   // (a fuzzed metal reflection may still be absorbed)
        org = scatter_origin(h, side);
        dir = ray_direction<FASTN, RANGE>(raw);
    }
    WaveProbeOut o{};
    if (live) {
        o.scattered = scattered ? 1.0f : 0.0f;
        if (scattered) { o.o[0] = org.x; o.o[1] = org.y; o.o[2] = org.z; o.d[0] = dir.x; o.d[1] = dir.y; o.d[2] = dir.z; o.atten[0] = atten.x; o.atten[1] = atten.y; o.atten[2] = atten.z; }
        o.emitted[0] = emitted.x; o.emitted[1] = emitted.y; o.emitted[2] = emitted.z;
        if (used_ball) { o.ball[0] = ball.x; o.ball[1] = ball.y; o.ball[2] = ball.z; }
    }
    out[i] = o;
}

// The forms the library launches: the template arguments at the call sites of shade_and_regenerate (render_ctr_lockstep, render_ctr_wavefront,
// render_ctr_state_machine) and the STEP each kernel is instantiated with.  Two kernels that resolve to the same arguments share one instantiation.
struct WaveForm { const char* name; uint32_t mats, wide, fastn, try1, terminal_done, step, in_place; const void* kernel; };
template <uint32_t MATS, bool WIDE, bool FASTN, int TRY1, bool TERMINAL_DONE, bool STEP, bool IN_PLACE = false, uint32_t RANGE = 0u>
static WaveForm wave_form(const char* name) {
    return WaveForm{name, MATS, WIDE, FASTN, (uint32_t)TRY1, TERMINAL_DONE, RngCtrT<STEP>::STEPPED, IN_PLACE,
                    reinterpret_cast<const void*>(&k_probe_scatter_wave<MATS, WIDE, FASTN, TRY1, TERMINAL_DONE, STEP, IN_PLACE, RANGE>)};
}
static const WaveForm WAVE_FORMS[] = {
    wave_form<MATS_LAMBERT, true, true, 1, true, step_form(STEP_SIMPLE_QC)>("k_render_sky_simple_qc"),
    wave_form<MATS_LAMBERT, true, true, 1, true, step_form(STEP_SIMPLE_QC), (MI355RT_QC_FORM & FORM_STATE_IN_PLACE) != 0u, MI355RT_QC_RANGE>("k_render_ctr_simple_qc"),
    wave_form<MATS_LAMBERT, true, true, 1, true, step_form(STEP_SIMPLE)>("k_render_ctr_simple"),
    wave_form<MATS_NO_SPECULAR, true, true, 0, true, step_form(STEP_NOSPEC)>("k_render_ctr_nospec"),
    wave_form<MATS_NO_SPECULAR, true, true, 0, true, step_form(STEP_WF_MESHFREE)>("k_render_ctr_wf_meshfree"),
    wave_form<MATS_ALL, true, true, 0, true, step_form(STEP_NOMESH)>("k_render_ctr_nomesh"),
    wave_form<MATS_ALL, true, true, 0, true, step_form(STEP_MESH)>("k_render_ctr_mesh"),
    wave_form<MATS_ALL, true, false, 0, true, step_form(STEP_WF)>("k_render_ctr_wf"),
    wave_form<MATS_ALL, true, false, 0, true, step_form(STEP_WF_FIXAABB)>("k_render_ctr_wf_fixaabb"),
    wave_form<MATS_NO_METAL, true, false, 0, true, step_form(STEP_WF_NOMETAL)>("k_render_ctr_wf_nometal"),
    wave_form<MATS_NO_METAL, true, false, 0, true, step_form(STEP_WF_NOMETAL_SHALLOW)>("k_render_ctr_wf_nometal_shallow"),
    wave_form<MATS_NO_METAL, true, false, 0, true, step_form(STEP_WF_NOMETAL_IDENT)>("k_render_ctr_wf_nometal_ident"),
    wave_form<MATS_ALL, false, false, 0, false, false>("k_render_ctr_sm"),
};
constexpr uint32_t WAVE_FORM_COUNT = sizeof(WAVE_FORMS) / sizeof(WAVE_FORMS[0]);

}  // namespace mi355rt

// Not in the public header; the reference build's diagnostic entries.
// mi355rt_debug_scatter_wave_form: what form `form` is -- words = {mats, wide, fastn, try1, terminal_done, stepped, in_place, number of forms}
// and the name of the kernel it belongs to (a static string) -- so that a test runs every distinct instantiation once and knows its material set.
extern "C" int mi355rt_debug_scatter_wave_form(uint32_t form, uint32_t* words, const char** name) {
    using namespace mi355rt;
    return guard([&]() -> int {
    if (form >= WAVE_FORM_COUNT || !words) return fail(MI355RT_ERR_INVALID, "debug_scatter_wave_form: form");
    const WaveForm& f = WAVE_FORMS[form];
    const uint32_t w[8] = {f.mats, f.wide, f.fastn, f.try1, f.terminal_done, f.step, f.in_place, WAVE_FORM_COUNT};
    for (int k = 0; k < 8; ++k) words[k] = w[k];
    if (name) *name = f.name;
    return MI355RT_OK;
    });
}
// mi355rt_debug_scatter_wave: host pointers.  materials = n_materials mi355rt_material; records = n WaveProbeIn, 64 to a wave in the order
// given; out = n WaveProbeOut.  A live record's material must be of a kind the form is compiled for (no texture: the probe binds none), and of
// no terminal kind where the form's caller finishes those.  The last workgroup is padded with idle lanes.  Synchronous; every buffer is freed
// before it returns.
extern "C" int mi355rt_debug_scatter_wave(uint32_t form, const void* materials, uint32_t n_materials, const void* records, uint32_t n, void* out, int device) {
    using namespace mi355rt;
    return guard([&]() -> int {
    if (form >= WAVE_FORM_COUNT || !materials || !n_materials || !records || !out || !n) return fail(MI355RT_ERR_INVALID, "debug_scatter_wave: form / null / empty");
    if (n > (1u << 24)) return fail(MI355RT_ERR_INVALID, "debug_scatter_wave: at most 2^24 records");
    const WaveForm& f = WAVE_FORMS[form];
    const DevMat* m = static_cast<const DevMat*>(materials);
    const WaveProbeIn* in = static_cast<const WaveProbeIn*>(records);
    const uint32_t terminal = MATS_TERMINAL;
    for (uint32_t i = 0; i < n; ++i) {
        if (!(in[i].flags & WAVE_PROBE_LIVE)) continue;
        if (in[i].material >= n_materials) return fail(MI355RT_ERR_INVALID, "debug_scatter_wave: material index");
        const uint32_t kind = m[in[i].material].kind;
        if (kind >= MI355RT_MAT_KIND_COUNT || kind == MI355RT_MAT_TEXTURE || !((f.mats >> kind) & 1u) || (f.terminal_done && ((terminal >> kind) & 1u)))
            return fail(MI355RT_ERR_INVALID, "debug_scatter_wave: a live lane's material kind is not one this form scatters");
    }
    const uint32_t padded = (n + BLOCK_THREADS - 1u) / BLOCK_THREADS * BLOCK_THREADS;
    std::vector<WaveProbeIn> host(padded);
    for (uint32_t i = 0; i < n; ++i) host[i] = in[i];
    for (uint32_t i = n; i < padded; ++i) { WaveProbeIn idle{}; idle.k0 = idle.k1 = idle.x = idle.s = idle.ray = 0xFFFFFFFFu; host[i] = idle; }
    HIP_TRY(hipSetDevice(device));
    DevBuf<WaveProbeIn> d_in; DevBuf<WaveProbeOut> d_out; DevBuf<DevMat> d_mats;
    int rc = d_in.ensure(padded);
    if (!rc) rc = d_out.ensure(padded);
    if (!rc) rc = d_mats.ensure(n_materials);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpy(d_in.p, host.data(), (size_t)padded * sizeof(WaveProbeIn), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) e = hipMemcpy(d_mats.p, m, (size_t)n_materials * sizeof(DevMat), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) {
        const DevMat* a0 = d_mats.p; const WaveProbeIn* a1 = d_in.p; WaveProbeOut* a2 = d_out.p;
        void* args[] = {&a0, &a1, &a2};
        (void)hipLaunchKernel(f.kernel, dim3(padded / BLOCK_THREADS), dim3(BLOCK_THREADS), args, 0, nullptr);
        e = hipGetLastError();
    }
    if (!rc && e == hipSuccess) e = hipMemcpy(out, d_out.p, (size_t)n * sizeof(WaveProbeOut), hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) rc = fail(MI355RT_ERR_HIP, std::string("debug_scatter_wave: ") + hipGetErrorString(e));
    d_in.release(); d_out.release(); d_mats.release();
    return rc;
    });
}
