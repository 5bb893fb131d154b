// rt_kernels.hip -- hand-written HIP kernels for gfx950 (MI355X) replacing the rayon per-pixel loop of
// jackra1n/raytracer-rust (render_scene -> trace_ray, src/renderer.rs:19-123).
//
// Kernels
//   k_render_ctr   persistent wave64 path tracer.  One lane = one path (one sample of one pixel).  A wave
//                  claims BATCH_SAMPLES consecutive sample indices with ONE global atomic and deals them
//                  to its lanes with ballot/mbcnt whenever lanes run dry (path regeneration), so lanes
//                  whose paths end early (miss, emitter, absorption) are refilled on the next iteration
//                  instead of idling until the longest path of the wave finishes.
//                  The top-level primitive list is walked with a wave-uniform index through the constant
//                  address space (scalar loads, records live in SGPRs); the per-mesh BVH is a threaded
//                  pre-order array walked per lane with dwordx4 loads -- the reference always descends
//                  left-then-right (bvh.rs:142-156), so escape links reproduce its visit order and its
//                  shrinking t_max exactly and no traversal stack is needed.
//                  Randomness: a counter-based generator (pcg4d since round 5; Philox4x32-10 / -7 selectable at build time,
//                  rt_rng.h) addressed by (image row key; x, sample, ray index, block): every draw is a pure function of
//                  the path, so any schedule / tiling / GPU count produces bit-identical radiance.
//                  Round 5: a wave keeps the camera rays of its next 64 samples IN STOCK (RayStock, LDS) and the mesh-free kernels
//                  are instantiated per material set AND per primitive-kind set (k_render_ctr_simple_qc).  k_render_ctr_simple_qc
//                  stocks the camera rays' first hits instead (HitStock), walked in refill passes of the loop.
//                  Those passes test only the primitives their one or two pixels can see (RenderParams.cam_mask_off: per-pixel masks built by set_scene).
//                  Output: three floats of radiance per path into the HBM workspace.
//   k_resolve      per pixel, sums its spp radiance values IN SAMPLE ORDER (renderer.rs:100), scales by
//                  1/spp (:103), sqrt-gamma, clamp, pack 0x00RRGGBB (:112-120, color.rs:87-93).
//   k_render_ref   validation mode: one lane per image row replays the reference's sequential
//                  StdRng::seed_from_u64(y) stream (renderer.rs:91) and folds radiance tail-first.
//   k_gather_strips  the multi-device exchange: de-interleaves the parts' strips into the image (rt_multi.cpp).
//   k_gather_accum   the same for the parts' running sums of a progressive multi-device render (rt_multi.cpp).
//
// Files (one translation unit; this file includes the rest): rt_math.h (vec3.rs helpers), rt_rng.h (pcg4d / Philox, ChaCha12 replay),
// rt_intersect.h (hit tests, BVH walk, finish_hit), rt_materials.h (scatter, camera, miss colour), here: the work cursor,
// shade_and_regenerate() and the lockstep kernels, then rt_mesh_variants.h (the state machine of the reference build), rt_wavefront.h
// (k_render_ctr_wf), and at the end k_resolve, k_render_ref, the debug kernels and the launchers.
//
// Numerics: compiled with -ffp-contract=off and correctly rounded f32 divide/sqrt; every expression
// keeps the reference's operation order (file:line cited per function), so results agree with the
// CPU oracle bit-for-bit wherever only + - * / sqrt are involved.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rt_device.h"
#include "../../../include/mi355rt.h"

#include "rt_math.h"
#include "rt_rng.h"
#include "rt_intersect.h"
#include "rt_materials.h"

namespace mi355rt {

DI uint32_t mbcnt64(uint64_t mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u)); }
DI uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// The hand-off of WAVE-PRIVATE LDS between the lanes of one wave (RayStock, HitStock: entries that one lane writes and another reads, or reads and another
// overwrites).  The hardware needs nothing for it: a wave's DS instructions execute in the order they were issued, for all of its lanes at once.  The
// compiler has to be told: to it every lane is a thread of its own, and without a fence it may move one thread's LDS accesses past each other wherever it
// can show that THAT thread's addresses differ.  This orders every LDS access of the wave in front of the call before every LDS access behind it -- a release
// fence, a wave barrier, an acquire fence, all of wavefront scope and for the local address space only (global loads and stores stay free to move).  It
// emits no instruction: wavefront-scope fences and the wave barrier are constraints on the compiler's schedule, nothing else.
// Call it wherever an entry changes hands; memory that each lane writes and reads back itself (HitStock's parking area) needs none.
// FENCED = false leaves the wave barrier alone.  The compiler moves no memory access across it either (to the optimiser it is a call that may read and write
// anything, to the scheduler an instruction with side effects), but it is no memory operation to the language.  deal_stocked uses this form: there the
// fences, on their own or around the barrier, make the compiler lay k_render_ctr_nomesh out differently, 0.8 ... 1.7 % slower (profiles/ab_defined_handoffs.txt).
template <bool FENCED = true>
DI void wave_lds_handoff() {
    if constexpr (FENCED) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    if constexpr (FENCED) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// ===================================================================================================
// Shared pieces of the two counter-mode kernels
// ===================================================================================================
// n / d for n < 2^31 with a host-computed magic pair (mul == 0 means d == 1): q = umulhi(n, mul) >> shift.
DI uint32_t fastdiv(uint32_t n, uint32_t mul, uint32_t shift) { return mul ? (__umulhi(n, mul) >> shift) : n; }

// Wave-uniform cursor over the band's sample indices.  A wave claims a run of consecutive indices with one
// global atomic and deals them to idle lanes with ballot + mbcnt.
//  * The band is cut into WORK_SHARDS contiguous ranges, each with its own counter on its own cache line.
//    A wave starts on the shard of its XCD (HW_REG_XCC_ID; used for speed only) and moves to the next shard
//    when one runs dry (work stealing), so one hot word never serialises all 6 k waves of the chip
//    (measured: a single counter saturates near 88 atomics/us and made short runs 30 % slower).
//  * Run length follows guided self-scheduling: (what was left in the shard at the wave's previous claim)
//    / guided_div, clamped to [run_min, run_max] -- long runs while there is plenty of work (few atomics,
//    coherent primary rays), short runs at the end so that all waves drain together.  This matters when one
//    image is split across 8 GPUs and a launch lasts only a few ms.
DI uint32_t xcc_id() { uint32_t v; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v)); return v & (WORK_SHARDS - 1u); }
// RMIN .. RMAX: the run lengths, compile-time (as kernel arguments they cost the Lambert-only kernel two more live scalar registers
// in its hot loop and 5.7 % of its time).  RMIN == RMAX: fixed runs, no guided division.
template <uint32_t RMIN, uint32_t RMAX>
struct WorkCursorT {
    uint32_t next = 0, end = 0; bool no_more = false;
    uint32_t shard = 0, dry = 0, seen = 0;      // current shard, consecutive dry shards, last counter value seen in it
    DI void init() { shard = xcc_id(); }
    DI bool exhausted() const { return no_more && next == end; }
    // One global atomic: the next run of the wave's shard (or of the next shard that still has work).  Wave-uniform.
    DI void claim(const RenderParams& P, uint32_t lane) {
        while (next == end && !no_more) {
            const uint32_t base = shard * P.shard_samples;
            const uint32_t len = min(P.shard_samples, P.band_samples > base ? P.band_samples - base : 0u);
            const uint32_t rem = len > seen ? len - seen : 0u;
            const uint32_t size = RMIN == RMAX ? RMAX : min(max(rem / P.guided_div, RMIN), RMAX);
            uint32_t start = 0;
            if (lane == 0) start = atomicAdd(P.batch_counter + shard * WORK_SHARD_STRIDE, size);
            start = __builtin_amdgcn_readfirstlane(start);
            if (start >= len) {                              // shard is dry: steal from the next one
                shard = (shard + 1u) & (WORK_SHARDS - 1u); seen = 0;
                if (++dry == WORK_SHARDS) no_more = true;
            } else { next = base + start; end = base + min(start + size, len); seen = start + size; dry = 0; }
        }
    }
    // Lanes with want == true get a sample index (returns true and sets sidx); others / surplus stay idle.
    DI bool deal(const RenderParams& P, bool want, uint32_t lane, uint32_t& sidx) {
        const uint64_t idle = __ballot(want);
        if (idle == 0ull) return false;
        claim(P, lane);
        const uint32_t take = min((uint32_t)__popcll(idle), end - next);
        bool got = false;
        if (take != 0u) {
            const uint32_t rank = mbcnt64(idle);
            if (want && rank < take) { sidx = next + rank; got = true; }
            next += take;
        }
        return got;
    }
    // The same, for a kernel that keeps camera rays IN STOCK (RayStock below): samples are dealt out of [next, stock_end), the part of the
    // wave's run whose rays `refill(first, count)` has prepared -- up to 64 at a time, by the whole wave, whenever the stock runs out
    // (also in the middle of a deal: the lanes the old stock could not serve are served from the new one in the same call).
    uint32_t stock_end = 0;                                  // next == stock_end: the stock is empty
    template <class Refill, class Take>
    DI bool deal_stocked(const RenderParams& P, bool want, uint32_t lane, uint32_t& sidx, Refill&& refill, Take&& take_entry) {
        uint64_t idle = __ballot(want);
        if (idle == 0ull) return false;
        uint32_t n_idle = (uint32_t)__popcll(idle);
        if (n_idle <= stock_end - next) {                    // the common case: the stock serves every idle lane
            if (want) { sidx = next + mbcnt64(idle); take_entry(sidx); }
            next += n_idle;
            return want;
        }
        bool got = false;                                    // the stock runs out in this deal (once per 64 samples)
        for (;;) {
            if (next == stock_end) {
                claim(P, lane);
                if (next == end) break;                      // no work left anywhere
                stock_end = next + min(64u, end - next);
                wave_lds_handoff<false>();                   // the entries that lanes took, in this call or an earlier one, are overwritten by other lanes ...
                refill(next, stock_end - next);
                wave_lds_handoff<false>();                   // ... and a lane takes an entry that another lane wrote (the barrier alone: see wave_lds_handoff)
            }
            const uint32_t take = min(n_idle, stock_end - next);
            const uint32_t rank = mbcnt64(idle);
            if (want && !got && rank < take) { sidx = next + rank; got = true; take_entry(sidx); }
            next += take;
            idle = __ballot(want && !got);
            if (idle == 0ull) break;
            n_idle = (uint32_t)__popcll(idle);
        }
        return got;
    }
    // The same for a kernel that keeps camera-ray FIRST HITS in stock (HitStock below): a ring of up to 64 ready entries, [ring_head, +ring_count) mod 64.
    // The refill pass walks the camera rays of the next samples of the run and appends the paths that go on; the deal hands out entries only.
    uint32_t ring_head = 0, ring_count = 0;
    // Wave-uniform: how many camera rays the refill pass walks now -- 0 while the ring holds LOW entries or more, or when no work is left.
    template <uint32_t LOW>
    DI uint32_t refill_size(const RenderParams& P, uint32_t lane) {
        if (ring_count >= LOW) return 0u;
        claim(P, lane);                                      // (no atomic while the run lasts)
        return min(64u - ring_count, end - next);
    }
    // Lanes with want == true get the ring slot of an entry (returns true); the others / surplus stay idle.
    DI bool deal_ring(bool want, uint32_t& slot) {
        const uint64_t idle = __ballot(want);
        const uint32_t take = min((uint32_t)__popcll(idle), ring_count);
        const uint32_t rank = mbcnt64(idle);
        slot = (ring_head + rank) & 63u;
        ring_head = (ring_head + take) & 63u; ring_count -= take;
        return want && rank < take;
    }
};
typedef WorkCursorT<BATCH_MIN, BATCH_MAX> WorkCursor;                    // lockstep kernels (and the reference build's mesh kernels)
typedef WorkCursorT<RUN_WAVEFRONT_MIN, RUN_WAVEFRONT> WorkCursorWf;          // wavefront kernel: fixed, aligned runs (rt_device.h)

// Decode a band-local sample index into (x, y, s) and key the path's RNG (renderer.rs:91-97).
template <class RNG>
DI void start_path(const RenderParams& P, uint32_t sidx, RNG& rng, uint32_t& px, uint32_t& py) {
    const uint32_t pix_local = fastdiv(sidx, P.spp_mul, P.spp_shift);
    const uint32_t s = sidx - pix_local * P.spp;
    const uint32_t pix = P.band_pixel0 + pix_local;
    const uint32_t jrow = fastdiv(pix, P.width_mul, P.width_shift);
    px = pix - jrow * P.width;
    py = P.rows[jrow];
    const uint64_t ykey = (uint64_t)py + (((uint64_t)P.seed_hi << 32) | (uint64_t)P.seed_lo);
    rng.start((uint32_t)ykey, (uint32_t)(ykey >> 32), px, s + P.sample0);
}

// Per-lane path state shared by both kernels.  STEP: the form of the generator's draw address (rt_rng.h), chosen per kernel.
template <bool STEP>
struct PathStateT {
    typedef RngCtrT<STEP> Rng;
    f3 ro, rd, thr;
    uint32_t sidx, ray_index;
    uint32_t px, py;               // only meaningful while `fresh`
    Rng rng;
};
typedef PathStateT<false> PathState;

// Camera rays IN STOCK (lockstep kernels, round 5).  A path that ends hands its lane to a fresh sample in the same iteration, so every iteration
// started a few paths -- 11 of 64 lanes on cornell, in 93 % of the iterations (profiles/r05/stamps_final_kernels.txt) -- and paid the whole
// price of starting one for them: the sample index decoded, its row looked up (a global load the arithmetic half then waited for), the path's
// generator base, the jitter block, u / v, Camera::get_ray: ~100 instructions at a sixth of the lanes.  Every one of those values is a pure function
// of the sample index.  So the wave prepares the rays of the next (up to) 64 samples of its run AT ONCE, with all lanes, whenever its stock runs out
// (WorkCursorT::deal_stocked), and keeps them in 2 KB of LDS: per sample the direction before its two normalisations (camera.rs:33-42; the shared
// tail of the iteration normalises it with the scattered rays, as before) and the generator base.  A lane that is dealt sample i reads entry i mod 64:
// two ds_read_b128.  Same arithmetic per path, same bits.  Entries change hands between lanes: wave_lds_handoff() around refill (deal_stocked).
struct RayStock {
    float4* dir; uint4* key;                                   // [64] each, this wave's
    template <bool FASTN, class RNG>
    DI void refill(const RenderParams& P, uint32_t first, uint32_t count, uint32_t lane) const {
        if (lane < count) {
            const uint32_t sidx = first + lane;
            RNG rng; uint32_t px, py;
            start_path(P, sidx, rng, px, py);
            rng.template load_block0<true>();                                                   // ray 0, block 0: the jitter (words 0 / 1)
            const float un = (float)px + rng.jitter_u(), vn = (float)py + rng.jitter_v();
            const float u = FASTN ? div_by_rn(un, P.width_f, P.inv_width_rn) : un / (float)P.width;       // renderer.rs:96
            const float v = FASTN ? div_by_rn(vn, P.height_f, P.inv_height_rn) : vn / (float)P.height;    // renderer.rs:97
            const f3 raw = camera_raw(P.cam, u, v);                                              // renderer.rs:99
            dir[sidx & 63u] = make_float4(raw.x, raw.y, raw.z, 0.f);
            if constexpr (RNG::NW == 4) key[sidx & 63u] = make_uint4(rng.w[0], rng.w[1], rng.w[2], rng.w[3]);   // (the draw address as the generator keeps it: opaque here)
        }
    }
    template <class PS>
    DI void take(const RenderParams& P, uint32_t sidx, f3& raw, PS& ps) const {
        const float4 d = dir[sidx & 63u];
        raw = mk(d.x, d.y, d.z);
        // (handing the key over only after the iteration's shared generator call -- a fresh path does not use that call's block -- so that the wave need not
        //  wait for this read in front of it was measured: four more live registers, cornell +0.5 %, the general kernels +0.5 ... 2 %)
        if constexpr (PS::Rng::NW == 4) { const uint4 k = key[sidx & 63u]; ps.rng.w[0] = k.x; ps.rng.w[1] = k.y; ps.rng.w[2] = k.z; ps.rng.w[3] = k.w; }
        else start_path(P, sidx, ps.rng, ps.px, ps.py);                                          // (the Philox builds address by (key, x, s): nothing to keep)
    }
};
// Camera-ray FIRST HITS in stock (k_render_ctr_simple_qc).  With RayStock a freshly dealt lane still spends one whole iteration on the camera ray: the
// second half of the iteration in which it is dealt (generator, cooperative unit-ball rounds, normalisations: about half of an iteration) only copies
// the stocked direction, and scatters the first hit one iteration later -- 11 of 61 live lanes, in 94 % of the iterations, do no shading work.
// Here the camera rays go through the loop's one walk site in a REFILL PASS of their own (render_ctr_lockstep): when the ring is empty, the wave
// parks its paths' rays in LDS, walks the camera rays of the next (up to 64 - ring_count) samples of its run with all lanes (coherent rays from one
// origin), finishes right there the paths whose camera ray misses or hits an emitter / a Null material, and appends the others as ready-to-scatter
// entries.  A lane that is dealt an entry scatters its first hit in the same iteration, as a continuing lane at ray 0.  Every value of an entry is the
// one the loop computed for that sample before (same functions, same order), so radiance and ray counts are the same bits.
// An entry is 64 bytes (four ds_read_b128): {h.p, sample index}, {h.n, mat_ff}, q0, the generator key at ray 0 (pcg4d: its four words; Philox: the
// key, x and s -- the ray word is 0; the words are the generator's own, stored and reloaded untouched).  The parking area holds ro and rd of the 64 lanes (24 bytes each) during a refill pass;
// the kernel compiled without the sky lookup has none and parks them in bytes 0-23 of the (then empty) ring's slots instead: render_ctr_lockstep, PARK_IN_RING.
// The forms of k_render_ctr_simple_qc that carry a path's state in place (FORM, a template argument of render_ctr_lockstep, shade_and_regenerate and
// HitStock::append; 0 everywhere else, which folds to the code as it was).  Each bit has a build define, MI355RT_QC_*, whose 0 builds the form before it.
//   FORM_HIT_IN_PLACE    a dealt lane reads its ring entry into the Hit it scatters: the one the walk wrote for the continuing lanes (no `hs = h`).
//   FORM_STATE_IN_PLACE  the bounce writes the next origin and throughput over the old ones as soon as the hit is known, for all lanes and outside
//                        any lane mask, so that the hit point and the albedo are dead before the generator runs and nothing is copied at the loop's bottom.
//   FORM_TERM_SELECT     the terminal classification selects `term` by the comparison results: no defaults, no nested regions, one store region.
//                        The shortest listing of all and slower on the GPU (+0.06 ms per step on cornell): its define stays at 0.
// The first two ship together: cornell -1.35 % (DESIGN.md 4.1 "Path state carried in place", profiles/bench_state_in_place_vs_parent.txt).
//   FORM_EMPTY_PASS      a refill pass whose camera-mask words are all 0 -- no camera ray of its pixels can hit anything -- builds no camera ray and walks
//                        nothing (render_ctr_lockstep, `walk_cam`).  It still parks the rays and runs append(): no lane walked, so every `hit` is false and
//                        append() stores 1 * miss for every camera path, as it does for any miss.  A form that gives the empty pass a store or an exit of its
//                        own moves the loop's scalar allocation (profiles/isa_diff_empty_pass_vs_parent.txt); this one leaves it where it was.
//                        Cornell -0.85 % (DESIGN.md 4.1 "Nothing for pixels that see nothing", profiles/bench_empty_pass_vs_parent.txt).
enum : uint32_t { FORM_HIT_IN_PLACE = 1u, FORM_STATE_IN_PLACE = 2u, FORM_TERM_SELECT = 4u, FORM_EMPTY_PASS = 8u };
// A path's terminal radiance by selects (FORM_TERM_SELECT): the miss colour where nothing was hit, the emitter's colour, 0 for a Null material;
// returns whether the path ends here.  `q0` is read only where `hit` says it was written.
DI bool terminal_select(const RenderParams& P, bool hit, const float4& q0, f3& term) {
    const bool emis = hit && __float_as_uint(q0.x) == MI355RT_MAT_EMISSIVE;
    term = mk(hit ? (emis ? q0.y : 0.f) : P.miss[0], hit ? (emis ? q0.z : 0.f) : P.miss[1], hit ? (emis ? q0.w : 0.f) : P.miss[2]);
    return !hit || emis || __float_as_uint(q0.x) == MI355RT_MAT_NULL;
}
struct HitStock {
    float4* e;                                                 // [64][4] this wave's ring of entries
    float4* park_a; float2* park_b;                            // [64] each: {ro, rd.x}, {rd.y, rd.z}; lane i writes and reads back element i only: no hand-off (null with PARK_IN_RING)
    // Before the walk: the camera ray of sample `sidx` into (ro, rd) -- what RayStock::refill and the loop's shared tail computed -- and its key
    // into the entry at `slot` (the entry's other words are written after the walk).  The slot is one that another lane was dealt earlier, and append()
    // reads the key from another lane: the caller puts a wave_lds_handoff() in front of the camera() calls and one behind them.
    // `here` is 0: a wave-uniform index that the caller makes from the pass's first sample index (below 2^31, rt_device.h), so that the camera record is read (scalar loads) where the pass
    // uses it.  Read as P.cam it is a launch constant, and with the stepped generator the compiler kept its first 32 bytes in eight scalar registers
    // across the whole loop and spilled the loop's own masks for them (13 spilled SGPRs, 23 v_readlane; like this 3 and 9, the plain form 6 and 10).
    template <class RNG, uint32_t RANGE = 0u>
    DI void camera(const RenderParams& P, uint32_t sidx, uint32_t slot, f3& ro, f3& rd, uint32_t here) const {
        RNG rng; uint32_t px, py;
        start_path(P, sidx, rng, px, py);
        rng.template load_block0<true>();                                                   // ray 0, block 0: the jitter (words 0 / 1)
        const float un = (float)px + rng.jitter_u(), vn = (float)py + rng.jitter_v();
        const float u = div_by_rn(un, P.width_f, P.inv_width_rn);                           // renderer.rs:96
        const float v = div_by_rn(vn, P.height_f, P.inv_height_rn);                         // renderer.rs:97
        const DevCamera& cam = (&P.cam)[here];
        ro = mk(cam.position[0], cam.position[1], cam.position[2]);
        rd = ray_direction<true, RANGE>(camera_raw(cam, u, v));                                  // renderer.rs:99
        e[4u * slot + 3u] = make_float4(__uint_as_float(rng.w[0]), __uint_as_float(rng.w[1]), __uint_as_float(rng.w[2]), __uint_as_float(rng.w[3]));
    }
    // After the walk (lanes with cam == true walked sample first + lane from `tail` + lane): finish the paths that end at their camera ray, exactly as
    // shade_and_regenerate classifies a path at ray 0 (throughput 1), and append the others to the ring in sample order.  Returns how many were appended.
    // NOSKY: see shade_and_regenerate; `rd` is then not read.
    template <bool NOSKY = false, uint32_t FORM = 0u>
    DI uint32_t append(const RenderParams& P, uint32_t lane, uint32_t first, uint32_t tail, bool cam, bool hit, const Hit& h, f3 rd) const {
        struct Rad { float x, y, z; };
        bool keep = false;
        if constexpr (NOSKY && (FORM & FORM_TERM_SELECT) != 0u) {
            f3 term; const bool fin = terminal_select(P, hit, h.q0, term);
            if (cam && fin) { const f3 L = mk(1.f, 1.f, 1.f) * term; reinterpret_cast<Rad*>(P.radiance)[first + lane] = Rad{L.x, L.y, L.z}; }
            keep = cam && !fin;
        } else
        if (cam) {
            f3 term = mk(0.f, 0.f, 0.f); bool fin = false;
            if (!hit) { if constexpr (NOSKY) term = mk(P.miss[0], P.miss[1], P.miss[2]); else term = miss_colour(P.sky, P.sky_w, P.sky_h, P.miss, rd); fin = true; }      // renderer.rs:38-63
            else {
                const uint32_t kind = __float_as_uint(h.q0.x);
                if (kind == MI355RT_MAT_EMISSIVE) { term = mk(h.q0.y, h.q0.z, h.q0.w); fin = true; }
                else if (kind == MI355RT_MAT_NULL) fin = true;
            }
            if (fin) { const f3 L = mk(1.f, 1.f, 1.f) * term; reinterpret_cast<Rad*>(P.radiance)[first + lane] = Rad{L.x, L.y, L.z}; }
            keep = !fin;
        }
        const uint64_t km = __ballot(keep);
        if (keep) {
            const float4 key = e[4u * ((tail + lane) & 63u) + 3u];
            wave_lds_handoff();                                                             // every lane has read its key before any lane writes an entry
            float4* d = e + 4u * ((tail + mbcnt64(km)) & 63u);
            d[0] = make_float4(h.p.x, h.p.y, h.p.z, __uint_as_float(first + lane));
            d[1] = make_float4(h.n.x, h.n.y, h.n.z, __uint_as_float(h.mat_ff));
            d[2] = h.q0;
            d[3] = key;
        }
        return (uint32_t)__popcll(km);
    }
};
#ifndef MI355RT_PREHIT_LOW
#define MI355RT_PREHIT_LOW 1                                   // refill when fewer entries are left: only when the ring is empty (cornell, against the parent: 1 -3.8 %, 4 -1.9 %, 8 -1.6 %, 16 -1.0 %, 32 +5 %; a partial refill walks fewer camera rays for the same cost)
#endif
struct NoStock {};

// random_in_unit_sphere (vec3.rs:54-61) for the whole wave at once, counter mode.  Try 0 comes from the event's
// block 0 (already in rng.b0).  Lanes whose try 0 failed become OWNERS of a retry request; then every lane of
// the wave -- busy or not -- is a WORKER: with n owners, G = 2^floor(log2(64 / n)) workers serve each owner and
// evaluate its tries jbase .. jbase+G-1 in parallel (the owner's counters arrive through ds_bpermute; a draw is a
// pure function of (key, x, s, ray, try), so any lane can compute it).  The owner takes the FIRST accepted try of
// its segment of the ballot, i.e. exactly the try the sequential loop would have stopped at.  Typically two
// rounds instead of E[max over 64 lanes of a geometric(0.52)] ~ 7.7 iterations of a mostly idle wave.
// Must be called in wave-uniform control flow.
// Stepped draw address (RngCtrT<true>): try j enters the generator's rounds as W_3 + j * A.  The owner keeps the word of its NEXT try, `wnext`, instead
// of the try's number and advances it by A << lg when a round fails; wnext travels in the place of W_3, so a round moves four words per worker, not
// five.  A worker adds sub * A for its place sub < 64 in the group: a 24-bit multiply (A < 2^24, sub < 2^6: the product is exact in 32 bits), the only
// place where one may be used -- everywhere else j is unbounded and takes the full multiply (RngCtrT::block) or a running word.
DI int lane_shfl(int v, uint32_t src_lane) { return __builtin_amdgcn_ds_bpermute((int)(src_lane << 2), v); }
DI float lane_shfl(float v, uint32_t src_lane) { return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), __float_as_int(v))); }
template <bool WIDE = false, int TRY1 = 0, class RNG>
DI f3 unit_ball_cooperative(bool diffuse, const RNG& rng, uint32_t lane, const uint32_t* b1 = nullptr) {
    constexpr bool STEPPED = RNG::STEPPED;
    f3 p = mk(u32_to_range11(rng.b0[1]), u32_to_range11(rng.b0[2]), u32_to_range11(rng.b0[3]));   // try 0
    bool need = diffuse && !(len2(p) < 1.0f);
    uint32_t jbase = 1;                                                            // plain form: the number of the owner's next try
    if constexpr (TRY1 >= 1) {                                                     // try 1 was drawn in the lane itself, next to the event's block
        const f3 p1 = mk(u32_to_range11(b1[1]), u32_to_range11(b1[2]), u32_to_range11(b1[3]));
        if (need && len2(p1) < 1.0f) { p = p1; need = false; }
        jbase = 2;                                                                 // (tries 1 AND 2 in the lane: the same kernel spills, 14.8 -> 17.9 ms)
    }
    if constexpr (TRY1 >= 2) {
        if (__ballot(need) != 0ull) {
            uint32_t b2[4]; RNG::template block<WIDE>(rng.w, 2u, b2);
            const f3 p2 = mk(u32_to_range11(b2[1]), u32_to_range11(b2[2]), u32_to_range11(b2[3]));
            if (need && len2(p2) < 1.0f) { p = p2; need = false; }
        }
        jbase = 3;
    }
    uint32_t wnext = 0u;                                                           // stepped form: the last word of the owner's next try, W_3 + jbase * A
    if constexpr (STEPPED) wnext = rng.w[3] + jbase * LCG_A;                       // (jbase is a constant here)
    for (;;) {
        const uint64_t m = __ballot(need);
        if (m == 0ull) break;
        const uint32_t n = (uint32_t)__popcll(m);
        const uint32_t lg = 6u - (n <= 1u ? 0u : 32u - (uint32_t)__builtin_clz(n - 1u));   // G = 2^lg = largest power of two <= 64 / n workers per owner
        const uint32_t r = mbcnt64(m);                                             // owners below this lane
        // table: lane t holds the lane id of owner number t (a full permutation keeps every lane enabled)
        const int tab = __builtin_amdgcn_ds_permute((int)((need ? r : n + (lane - r)) << 2), (int)lane);
        const uint32_t orank = lane >> lg;
        const bool worker = orank < n;
        const uint32_t olane = (uint32_t)lane_shfl(tab, worker ? orank : 0u);
        uint32_t w[4];
        if constexpr (STEPPED) {
            const uint32_t o0 = (uint32_t)lane_shfl((int)rng.w[0], olane), o1 = (uint32_t)lane_shfl((int)rng.w[1], olane), o2 = (uint32_t)lane_shfl((int)rng.w[2], olane);
            const uint32_t o3 = (uint32_t)lane_shfl((int)wnext, olane);
            RNG::block_at(o0, o1, o2, o3 + __umul24(lane & ((1u << lg) - 1u), LCG_A), w);   // sub < 64, A < 2^24
        } else {
        uint32_t ow[RNG::NW];                                                      // the owner's draw address (rt_rng.h)
#pragma unroll
        for (int i = 0; i < RNG::NW; ++i) ow[i] = (uint32_t)lane_shfl((int)rng.w[i], olane);
        const uint32_t oj = (uint32_t)lane_shfl((int)jbase, olane);
        RNG::template block<WIDE>(ow, oj + (lane & ((1u << lg) - 1u)), w);
        }
        const f3 q = mk(u32_to_range11(w[1]), u32_to_range11(w[2]), u32_to_range11(w[3]));
        const uint64_t acc = __ballot(worker && (len2(q) < 1.0f));
        const uint32_t seg_lo = r << lg;                                           // my segment of the ballot (owners only)
        const uint64_t segmask = (lg == 6u) ? ~0ull : ((1ull << (1u << lg)) - 1ull);
        const uint64_t seg = need ? ((acc >> seg_lo) & segmask) : 0ull;
        const bool found = seg != 0ull;
        const uint32_t src = found ? seg_lo + (uint32_t)__builtin_ctzll(seg) : lane;
        const float qx = lane_shfl(q.x, src), qy = lane_shfl(q.y, src), qz = lane_shfl(q.z, src);
        if constexpr (STEPPED) {
            if (need && found) { p = mk(qx, qy, qz); need = false; }
            wnext += LCG_A << lg;                                                  // (every lane: the word matters only to an owner that still needs a try)
        } else {
        if (need) { if (found) { p = mk(qx, qy, qz); need = false; } else jbase += (1u << lg); }
        }
    }
    return p;
}

// The shading half of one trace_ray level (renderer.rs:26-36) plus path regeneration, for every lane of the
// wave at once.  On entry `live` lanes carry a finished intersection (`hit`, `h`); on exit `live` lanes carry
// the next ray to trace.  Order: finish paths that end without scattering (miss / emitter / null) ->
// deal fresh samples to idle lanes -> ONE generator call for all lanes -> camera ray (fresh) or BSDF (continuing).
// Must be called by the whole wave in uniform control flow (it ballots): lanes that are busy elsewhere
// pass live = false and can_take = false and are left untouched.
// Returns false when no lane is live afterwards and no work is left to deal.
// DEFAULTS: give the per-lane temporaries default values.  The lockstep kernels run without (every value is read only on the
// path that wrote it, and the defaults cost ~30 v_mov per iteration: cornell -1.5 %), and since round 3 so does the wavefront
// kernel (rt_wavefront.h); the reference build's state machine keeps them (its other lanes'
// state must not be touched).  WIDE: the generator's multiplies as 64-bit products (rt_rng.h).  DROP_PRIO: lower the wave's priority to 0 once the
// fresh samples are dealt (the caller raised it for the memory-bound half of the iteration).  Q0_IN_HIT: see struct Hit.
// FASTN: see normalized() (rt_math.h).  TRY1: try 1 of the unit-ball draw comes from a second generator block drawn in the lane itself, right after the
// event's block, so the cooperative rounds start at try 2 and a second round is needed in 44 % of the iterations instead of all: cornell -0.9 %
// on the Lambert-only kernel; every other kernel pays for the three more live registers with spills (+1.5 ... +23 %: profiles/r03_ab_inlane_try1.txt).
// REKEY (wavefront kernel: a path's generator state is not carried in its slot): the state is derived from the sample index HERE, once, for continuing
// and freshly dealt lanes together, right in front of the event's block -- instead of by the caller when the slot is loaded (live through the hit record,
// the material read and the radiance store) and a second time where fresh samples are dealt.
// NOSKY: this instantiation is never launched with a sky texture (launch_render_ctr sees to it): a miss returns P.miss, three scalar registers.  Compiled in,
// the lookup of miss_colour() sits in the loop whether or not a scene has a sky -- its polynomial constants in vector registers across the whole
// iteration, and `sky == nullptr ? &P.miss : texel` as a pointer select with a per-lane load from the kernel-argument segment behind every miss.
// FORM: see FORM_HIT_IN_PLACE (HitStock; k_render_ctr_simple_qc only).  `h` is written only there: by the lanes that are dealt a ring entry.
template <uint32_t MATS, bool DEFAULTS = true, bool WIDE = !DEFAULTS, bool DROP_PRIO = false, bool Q0_IN_HIT = false, bool FASTN = false, int TRY1 = 0, bool REKEY = false, bool NOSKY = false, uint32_t FORM = 0u, uint32_t RANGE = 0u, class WC, class PS, class STOCK = NoStock>
DI bool shade_and_regenerate(const RenderParams& P, WC& wc, uint32_t lane, bool& live, bool can_take, bool hit, Hit& h,
                             PS& ps, uint32_t& n_paths, uint32_t& n_rays, Prof& prof, const STOCK& stock = STOCK()) {
    typedef typename PS::Rng Rng;                                                            // RngCtrT<STEP>: the kernel's form of the draw address
    constexpr bool STOCKED = std::is_same<STOCK, RayStock>::value;                           // camera rays come out of the wave's stock (lockstep kernels)
    constexpr bool PREHIT = std::is_same<STOCK, HitStock>::value;                            // ... or their first hits (k_render_ctr_simple_qc)
    constexpr bool HIT_IN_PLACE = (FORM & FORM_HIT_IN_PLACE) != 0u, STATE_IN_PLACE = (FORM & FORM_STATE_IN_PLACE) != 0u, TERM_SELECT = (FORM & FORM_TERM_SELECT) != 0u;
    static_assert(!(STOCKED || PREHIT) || (!DEFAULTS && !REKEY), "the stock serves the lockstep form");
    static_assert(!PREHIT || (MATS & ~MATS_LAMBERT) == 0u, "an entry holds no incoming direction: the Lambert bounce does not read it");
    static_assert(FORM == 0u || (PREHIT && Q0_IN_HIT && NOSKY && TRY1 == 1), "the in-place forms belong to k_render_ctr_simple_qc");
    static_assert(RANGE == 0u || (PREHIT && NOSKY && FASTN), "range arithmetic belongs to k_render_ctr_simple_qc");
    struct Rad { float x, y, z; };                                                        // 12 bytes per path: global_store_dwordx3
    Rad* __restrict__ radiance = reinterpret_cast<Rad*>(P.radiance);
    float4 q0;                                                                            // first 16 bytes of the hit material; read by lanes that loaded it
    if (DEFAULTS) q0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (TERM_SELECT) {
        f3 term; const bool fin = terminal_select(P, hit, h.q0, term);
        q0 = h.q0;
        if (live && fin) { const f3 L = ps.thr * term; radiance[ps.sidx] = Rad{L.x, L.y, L.z}; live = false; }
    } else
    if (live) {
        f3 term = mk(0.f, 0.f, 0.f); bool fin = false;
        if (!hit) { if constexpr (NOSKY) term = mk(P.miss[0], P.miss[1], P.miss[2]); else term = miss_colour(P.sky, P.sky_w, P.sky_h, P.miss, ps.rd); fin = true; }   // renderer.rs:38-63
        else {
            if constexpr (Q0_IN_HIT) q0 = h.q0;                                              // (finish_hit read it with the hit record)
            else q0 = reinterpret_cast<const float4*>(P.mats + (h.mat_ff & 0x7FFFFFFFu))[0];
            const uint32_t kind = __float_as_uint(q0.x);
            if (kind == MI355RT_MAT_EMISSIVE) { term = mk(q0.y, q0.z, q0.w); fin = true; }   // scatter -> None, emitted = colour
            else if (kind == MI355RT_MAT_NULL) fin = true;
        }
        if (fin) { const f3 L = ps.thr * term; radiance[ps.sidx] = Rad{L.x, L.y, L.z}; live = false; }
    }
    prof.mark(2);
    bool fresh = false;
    f3 stocked_raw = mk(0.f, 0.f, 1.f);
    Hit hs;                                                                                // PREHIT: the hit a lane scatters (a dealt lane's comes from the ring)
    if constexpr (PREHIT) {
        if constexpr (!HIT_IN_PLACE) hs = h;                                               // (in place: a dealt lane's h is dead, its ring entry goes there)
        uint32_t slot;
        if (wc.deal_ring(can_take && !live, slot)) {                                       // a continuing path at ray 0 from here on
            const float4* e = stock.e + 4u * slot;
            const float4 e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
            Hit& hd = HIT_IN_PLACE ? h : hs;
            hd.p = mk(e0.x, e0.y, e0.z); ps.sidx = __float_as_uint(e0.w);
            hd.n = mk(e1.x, e1.y, e1.z); hd.mat_ff = __float_as_uint(e1.w);
            q0 = e2;
            ps.rng.w[0] = __float_as_uint(e3.x); ps.rng.w[1] = __float_as_uint(e3.y); ps.rng.w[2] = __float_as_uint(e3.z); ps.rng.w[3] = __float_as_uint(e3.w);
            if constexpr (Rng::NW == 5) ps.rng.w[4] = 0u;                                  // (Philox: the ray word)
            ps.thr = mk(1.f, 1.f, 1.f); ps.ray_index = 0; live = true;
        }
    } else
    if constexpr (STOCKED) {
        if (wc.deal_stocked(P, can_take && !live, lane, ps.sidx, [&](uint32_t first, uint32_t count) { stock.template refill<FASTN, Rng>(P, first, count, lane); },
                            [&](uint32_t sidx) { stock.take(P, sidx, stocked_raw, ps); })) { fresh = true; live = true; ++n_paths; }
    } else
    if (wc.deal(P, can_take && !live, lane, ps.sidx)) { if constexpr (!REKEY) start_path(P, ps.sidx, ps.rng, ps.px, ps.py); fresh = true; live = true; ++n_paths; }
    if constexpr (DROP_PRIO) __builtin_amdgcn_s_setprio(0);                               // the lockstep kernels' arithmetic half (see render_ctr_lockstep)
    if constexpr (STATE_IN_PLACE) {
        // No lane is live behind the deal only when the ring was empty, and the loop comes here with an empty ring only when refill_size() found no
        // work left to claim (it refills whenever the ring is empty: MI355RT_PREHIT_LOW == 1).  So this is the end of the wave, not a third way back
        // to the loop's head with the state as it was -- the edge that kept the next state out of the registers of the old one.
        static_assert(MI355RT_PREHIT_LOW == 1, "an empty ring behind the deal means that no work is left");
        if (__ballot(live) == 0ull) return false;
    } else
    if (__ballot(live) == 0ull) return !wc.exhausted();
    uint32_t ball_use = BALL_NONE; bool scattered = false;
    f3 raw, atten, emitted; float side, fuzz = 0.f;  // written by the branch a lane takes below, read only on that lane's own path
    if constexpr (STATE_IN_PLACE) {
        // k_render_ctr_simple_qc: every live lane carries a hit on a Lambert surface (the terminal kinds are finished, a dealt lane is a continuing path
        // at ray 0), so the bounce is one straight line and its state is written IN PLACE: the next throughput thr * albedo (material.rs:47-71) and the next
        // origin p + n * EPS over the old ones, by all lanes and outside any lane mask (an idle lane's state may hold anything), before the generator runs.
        // The hit point, the albedo and the old state are dead from there on; only the normal lives on to the new direction.  The same operations on the
        // same operands as the form before it (scatter_pre / ball_finish / scatter_origin with MATS_LAMBERT), in another order.
        ps.thr = ps.thr * mk(q0.y, q0.z, q0.w);
        ps.ro = scatter_origin(PREHIT && !HIT_IN_PLACE ? hs : h, EPS);
        ++ps.ray_index;
        ps.rng.next_event();
        ps.rng.template load_block0<WIDE>();
        uint32_t blk1[4]; Rng::template block<WIDE>(ps.rng.w, 1u, blk1);
        ps.rng.begin_scatter();
        prof.mark(5);
        prof.classes(live, false, __float_as_uint(q0.x));
        const f3 ball = unit_ball_cooperative<WIDE, TRY1>(live, ps.rng, lane, blk1);          // whole wave, uniform control flow
        if (live && ps.ray_index == P.max_depth) {                                            // next level has depth == 0 (renderer.rs:20-22)
            const f3 L = ps.thr * mk(0.f, 0.f, 0.f);
            radiance[ps.sidx] = Rad{L.x, L.y, L.z}; live = false;
        }
        // (RANGE: every lane runs the two normalisations, idle ones included, and the range forms ballot all of them.  An idle lane holds the leftovers of
        //  its last path -- a unit normal and try 0 of a draw in [-1, 1)^3: ordinary vectors -- so it sends the wave to the guarded path only as an active
        //  lane would, for a sum below 1e-4 or a NaN.  Lanes idle only while the wave drains; the A/B is of the whole frame, drain included.)
        ps.rd = ray_direction<FASTN, RANGE>(diffuse_finish<FASTN, RANGE>(PREHIT && !HIT_IN_PLACE ? hs : h, ball));
        if (live) ++n_rays;
    } else
    if constexpr (DEFAULTS) {
        raw = mk(0.f, 0.f, 1.f); atten = mk(0.f, 0.f, 0.f); emitted = mk(0.f, 0.f, 0.f); side = EPS;
        if (live) {
            if (!fresh) ps.rng.next_event();
            ps.rng.template load_block0<WIDE>();
            if (fresh) {
                const float u = ((float)ps.px + ps.rng.jitter_u()) / (float)P.width;         // renderer.rs:96
                const float v = ((float)ps.py + ps.rng.jitter_v()) / (float)P.height;        // renderer.rs:97
                raw = camera_raw(P.cam, u, v);                                               // renderer.rs:99; normalised below with the scattered rays
                ps.ro = mk(P.cam.position[0], P.cam.position[1], P.cam.position[2]);
                ps.thr = mk(1.f, 1.f, 1.f); ps.ray_index = 0;
                if (P.max_depth == 0u) { radiance[ps.sidx] = Rad{0.f, 0.f, 0.f}; live = false; }   // depth == 0 -> BLACK
            } else {
                scattered = scatter_pre<MATS, WIDE>(P.mats, P.textures, q0, h, ps.rd, ps.rng, side, raw, atten, emitted, ball_use, fuzz);
            }
        }
        prof.mark(5);
        const f3 ball = unit_ball_cooperative<WIDE>(scattered && ball_use != BALL_NONE, ps.rng, lane);   // whole wave, uniform control flow
        if (live && !fresh) {
            if (scattered) scattered = ball_finish(ball_use, h, ball, fuzz, raw);            // (a fuzzed metal reflection may still be absorbed)
            if (scattered) {
                ps.thr = ps.thr * atten; ps.ro = scatter_origin(h, side); ++ps.ray_index;
                if (ps.ray_index == P.max_depth) {                                           // next level has depth == 0 (renderer.rs:20-22)
                    const f3 L = ps.thr * mk(0.f, 0.f, 0.f);
                    radiance[ps.sidx] = Rad{L.x, L.y, L.z}; live = false;
                }
            } else {                                                                         // absorbed: scatter -> None (renderer.rs:35)
                const f3 L = ps.thr * emitted;
                radiance[ps.sidx] = Rad{L.x, L.y, L.z}; live = false;
            }
        }
        if (live) { ps.rd = ray_direction(raw); ++n_rays; }                                  // fresh and scattered lanes together
    } else {
        // Lockstep kernels: every lane of the wave passes through here in every iteration, so a lane that is not live afterwards
        // is idle until it is dealt a fresh path (which sets all of its state) or for good -- its path state may hold anything.
        // The branches therefore only PRODUCE the next state (fresh values, nothing carried through them) and the state is
        // overwritten for all lanes at the end: no conditional updates of loop-carried registers, no copies to merge them.
        f3 n_ro, n_thr; uint32_t n_ri;
        if constexpr (REKEY) { if (live) { start_path(P, ps.sidx, ps.rng, ps.px, ps.py); ps.rng.set_ray(fresh ? 0u : ps.ray_index + 1u); } }
        else if (!fresh) ps.rng.next_event();
        ps.rng.template load_block0<WIDE>();
        uint32_t blk1[4] = {0u, 0u, 0u, 0u};
        if constexpr (TRY1 >= 1) Rng::template block<WIDE>(ps.rng.w, 1u, blk1);
        if (live) {
            if (fresh) {
                // (FASTN: div_bounded with the host's RN(1/width) -- the dividend is 0 or in [2^-24, 2^24), the divisor an image dimension in [1, 2^24);
                //  with the reciprocal computed in the kernel the compiler hoisted it into four vector registers that the loop then spilled)
                if constexpr (STOCKED) raw = stocked_raw;                                    // RayStock::refill computed it, with all lanes at once
                else {
                const float un = (float)ps.px + ps.rng.jitter_u(), vn = (float)ps.py + ps.rng.jitter_v();
                const float u = FASTN ? div_by_rn(un, P.width_f, P.inv_width_rn) : un / (float)P.width;       // renderer.rs:96
                const float v = FASTN ? div_by_rn(vn, P.height_f, P.inv_height_rn) : vn / (float)P.height;    // renderer.rs:97
                raw = camera_raw(P.cam, u, v);                                               // renderer.rs:99; normalised below with the scattered rays
                }
                n_ro = mk(P.cam.position[0], P.cam.position[1], P.cam.position[2]);
                n_thr = mk(1.f, 1.f, 1.f); n_ri = 0;
                if (P.max_depth == 0u) { radiance[ps.sidx] = Rad{0.f, 0.f, 0.f}; live = false; }   // depth == 0 -> BLACK
            } else {
                scattered = scatter_pre<MATS, WIDE, FASTN, /* TERMINAL_DONE */ true>(P.mats, P.textures, q0, PREHIT && !HIT_IN_PLACE ? hs : h, ps.rd, ps.rng, side, raw, atten, emitted, ball_use, fuzz);
            }
        }
        prof.mark(5);
        prof.classes(live && !fresh, live && fresh, __float_as_uint(q0.x));
        const f3 ball = unit_ball_cooperative<WIDE, TRY1>(scattered && ball_use != BALL_NONE, ps.rng, lane, blk1);   // whole wave, uniform control flow
        if (live && !fresh) {
            if (scattered) scattered = ball_finish<FASTN, RANGE>(ball_use, PREHIT && !HIT_IN_PLACE ? hs : h, ball, fuzz, raw);     // (a fuzzed metal reflection may still be absorbed)
            if (scattered) {
                n_thr = ps.thr * atten; n_ro = scatter_origin(PREHIT && !HIT_IN_PLACE ? hs : h, side); n_ri = ps.ray_index + 1u;
                if (n_ri == P.max_depth) {                                                   // next level has depth == 0 (renderer.rs:20-22)
                    const f3 L = n_thr * mk(0.f, 0.f, 0.f);
                    radiance[ps.sidx] = Rad{L.x, L.y, L.z}; live = false;
                }
            } else {                                                                         // absorbed: scatter -> None (renderer.rs:35)
                const f3 L = ps.thr * emitted;
                radiance[ps.sidx] = Rad{L.x, L.y, L.z}; live = false;
            }
        }
        ps.ro = n_ro; ps.thr = n_thr; ps.ray_index = n_ri;
        ps.rd = ray_direction<FASTN, RANGE>(raw);                                                 // fresh and scattered lanes together
        if (live) ++n_rays;
    }
    prof.mark(3);
    return true;
}

// Register budget per kernel, as waves per SIMD (A/B: tools/ab.py).  The lockstep kernel is VALU-issue bound
// and gains from 7 waves/SIMD (72 VGPRs) even with a few spills; the state-machine kernel keeps its hot BVH state in
// registers and loses when capped.
#define MI355RT_TRAV_BIAS 2                                 // (reference build's state machine)
#define MI355RT_OCC_LOCKSTEP 6                               // general mesh-free kernel, veach-mis 64 spp.  Round 1: 4 -> 6.46 ms, 5 -> 6.03, 6 -> 5.79,
                                                            // 7 -> 5.73.  After the instruction diet: 7 -> 4.94, 6 -> 4.88, and with the cube hit point
                                                            // carried (3 more registers): 7 -> 5.03 (spills), 6 -> 4.81, 5 -> 5.04
#define MI355RT_OCC_LS __attribute__((amdgpu_waves_per_eu(MI355RT_OCC_LOCKSTEP, MI355RT_OCC_LOCKSTEP)))
#define MI355RT_OCC_SIMPLE __attribute__((amdgpu_waves_per_eu(7, 7)))   // k_render_ctr_simple, k_render_ctr_nospec, k_render_sky_simple_qc: 72 VGPRs
// k_render_ctr_simple_qc, compiled without the sky lookup (NOSKY), step by step; each define's 0 builds the form before it (A/B:
// profiles/bench_nosky_eight_waves_vs_parent.txt).  8 waves per SIMD need 64 VGPRs and the rays parked in the ring (16 KB of LDS per workgroup).
#ifndef MI355RT_NOSKY_RECIP_FIRST
#define MI355RT_NOSKY_RECIP_FIRST 1
#endif
#ifndef MI355RT_NOSKY_PARK_IN_RING
#define MI355RT_NOSKY_PARK_IN_RING 1
#endif
#ifndef MI355RT_NOSKY_WAVES
#define MI355RT_NOSKY_WAVES 8
#endif
// ... and carrying a path's state in place (FORM_*, above HitStock; A/B: profiles/bench_state_in_place_vs_parent.txt), step by step in the same way.
// build.QC_FORM0_DEFINES builds the three at 0 for the tests (tests/test_gpu_state_in_place.py); the third is the one that did not pay.
#ifndef MI355RT_QC_HIT_IN_PLACE
#define MI355RT_QC_HIT_IN_PLACE 1
#endif
#ifndef MI355RT_QC_STATE_IN_PLACE
#define MI355RT_QC_STATE_IN_PLACE 1
#endif
#ifndef MI355RT_QC_TERM_SELECT
#define MI355RT_QC_TERM_SELECT 0
#endif
#ifndef MI355RT_QC_EMPTY_PASS
#define MI355RT_QC_EMPTY_PASS 1                              // the fourth bit of FORM; 0 (build.QC_FORM0_DEFINES, build.EMPTY_PASS_OFF_DEFINES) builds the camera pass as it was
#endif
#define MI355RT_QC_FORM ((MI355RT_QC_HIT_IN_PLACE != 0 ? FORM_HIT_IN_PLACE : 0u) | (MI355RT_QC_STATE_IN_PLACE != 0 ? FORM_STATE_IN_PLACE : 0u) | (MI355RT_QC_TERM_SELECT != 0 ? FORM_TERM_SELECT : 0u) | (MI355RT_QC_EMPTY_PASS != 0 ? FORM_EMPTY_PASS : 0u))
#define MI355RT_OCC_NOSKY __attribute__((amdgpu_waves_per_eu(MI355RT_NOSKY_WAVES, MI355RT_NOSKY_WAVES)))
#define MI355RT_OCC_SMK __attribute__((amdgpu_waves_per_eu(4, 4)))      // (reference build's state machine)

// ===================================================================================================
// k_render_ctr<HAS_MESH> -- persistent, path-regenerating wave64 path tracer, lockstep form: every live lane
// traces one full ray per loop iteration.  Used for scenes whose top level has no mesh (cornell, veach-mis):
// all lanes walk the same primitive list, so the iteration is divergence-free up to the hit tests.
// ===================================================================================================
// The lockstep kernels' forms (each measured against its alternative; docs/kernels/lockstep_round3.md): the candidate carries the cube's object-space hit
// point (also in the general kernel: pays at 80 VGPRs); the short reciprocal / square root / division of rt_math.h; in the Lambert-only kernel ONE try of the
// unit-ball draw in the lane itself before the cooperative rounds (0 tries: +1.9 %, 2 tries: +-0 with pcg4d, +23 % with Philox: profiles/r05/ab_counter_generator.txt).
// PREHIT: the wave stocks its camera rays' first hits (HitStock), walked in refill passes through the loop's one walk site.
// STEP: the generator's draw address in LCG-stepped form (rt_rng.h); per kernel, see the entry points below.
// NOSKY: never launched with a sky texture (shade_and_regenerate); with it the cube's reciprocals run first (recip3) and the refill pass parks the paths'
// rays inside the ring (below), each behind its build define so that the form before it can still be built for an A/B.
template <bool HAS_MESH, uint32_t MATS, uint32_t KINDS = PRIMS_ALL, bool PREHIT = false, bool BOUNDED = false, bool STEP = false, bool NOSKY = false, uint32_t FORM = 0u>
DI void render_ctr_lockstep(const RenderParams& P) {
    constexpr bool SIMPLE = (MATS & ~MATS_LAMBERT) == 0u;
    constexpr bool RECIP_FIRST = NOSKY && BOUNDED && (MI355RT_NOSKY_RECIP_FIRST != 0);
    // The refill pass parks the paths' rays INSIDE the ring: a refill happens only when the ring is empty, camera() writes bytes 48-63 of a slot and nothing
    // else until append(), so lane i keeps its 24 bytes in bytes 0-23 of slot i and takes them back right behind the walk, in front of append() -- which,
    // without a sky, does not read the camera ray's direction.  16 KB of LDS per workgroup instead of 22: the eighth workgroup of a CU fits.
    constexpr bool PARK_IN_RING = NOSKY && PREHIT && (MI355RT_NOSKY_PARK_IN_RING != 0);
    static_assert(!PARK_IN_RING || MI355RT_PREHIT_LOW == 1, "rays are parked in the ring's slots: a refill must find the ring empty");
    // An empty refill pass skips camera() and the walk (FORM_EMPTY_PASS, above HitStock).  Only without the sky lookup: there a miss is the constant P.miss.
    constexpr bool EMPTY_PASS = NOSKY && PREHIT && (FORM & FORM_EMPTY_PASS) != 0u;
    // Range arithmetic (rt_math.h): the kernel the cornell A/B measured it on.  k_render_sky_simple_qc keeps the guarded forms until a workload of its own says otherwise.
    constexpr uint32_t RANGE = (NOSKY && PREHIT && BOUNDED) ? MI355RT_QC_RANGE : 0u;
    // The mesh-free kernels are compiled for lists that hold something and for paths that may take a step: the host sends an empty list or max_depth == 0 to
    // k_render_ctr_mesh, the plain loop (rt_api.cpp render_samples).  Both are launch constants, and the compiler had turned `n_prims != 0` and `max_depth == 0`
    // into lane masks tested in every iteration (the masks spilled: four v_readlane, two mask operations, two branches): cornell -1.9 %.
    // (k_render_ctr_nomesh -1.2 %; k_render_ctr_nospec pays for the different allocation with 6 more scratch instructions, +0.4 %: it keeps the tests.)
    if constexpr (!HAS_MESH && MATS != MATS_NO_SPECULAR) { __builtin_assume(P.n_prims != 0u); __builtin_assume(P.max_depth != 0u); }
    cprim_t prims = (cprim_t)(P.prims);
    const uint32_t lane = threadIdx.x & 63u;
    WorkCursor wc; wc.init();
    std::conditional_t<PREHIT, HitStock, RayStock> stock;
    if constexpr (PREHIT) {                                                                    // HitStock: 64 entries of 64 B + 1.5 KB of parked rays per wave
        __shared__ __attribute__((aligned(16))) float4 s_ring[4u * BLOCK_THREADS];             // (22 KB per workgroup: 7 workgroups fit in 160 KB; PARK_IN_RING: 16 KB, 8 fit)
        stock.e = s_ring + 4u * (threadIdx.x & ~63u);
        if constexpr (PARK_IN_RING) { stock.park_a = nullptr; stock.park_b = nullptr; }
        else {
        __shared__ __attribute__((aligned(16))) float4 s_park_a[BLOCK_THREADS];
        __shared__ __attribute__((aligned(16))) float2 s_park_b[BLOCK_THREADS];
        stock.park_a = s_park_a + (threadIdx.x & ~63u); stock.park_b = s_park_b + (threadIdx.x & ~63u);
        }
    } else {
    __shared__ __attribute__((aligned(16))) float4 s_stock_dir[BLOCK_THREADS];                // RayStock: 64 entries per wave
    __shared__ __attribute__((aligned(16))) uint4 s_stock_key[BLOCK_THREADS];
    stock.dir = s_stock_dir + (threadIdx.x & ~63u); stock.key = s_stock_key + (threadIdx.x & ~63u);
    }
    PathStateT<STEP> ps; ps.ro = mk(0, 0, 0); ps.rd = mk(0, 0, 1); ps.thr = mk(1, 1, 1); ps.sidx = 0; ps.ray_index = 0; ps.px = ps.py = 0;
    ps.rng.clear();
    bool live = false;
    uint32_t n_paths = 0, n_rays = 0;
    Prof prof; prof.begin();
#ifdef MI355RT_STAMPS
    const unsigned long long t_wave0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long t_dry = 0ull; uint32_t drain_iters = 0, live_at_dry = 0;
#endif
    for (;;) {
        Hit h; bool hit = false;                           // h is read only where `hit` says it was written: no default values to copy around
        // Wave priority by phase (round 3; profiles/r03_ab_lockstep_priority.txt): the half of an iteration that waits on memory -- the
        // list walk's primitive reads, the material read, the radiance store and the work cursor's atomic -- runs at priority 1, the
        // arithmetic half (generator, BSDF, the cooperative unit-ball draw, the next ray) at 0, so a SIMD's issue slots go first to the
        // wave whose loads can then be in flight under the others' arithmetic.  cornell 16.49 -> 15.82 ms, veach-mis on these kernels -1.7 %;
        // priority 2 or 3 measure the same; keeping it through the generator call (15.96) or only over the walk (16.10-16.17) gains less.
        // (Round 5, after the scalar diet: all four schemes -- 1/0, none, inverted, 3/0 -- are within 0.2 % of each other; the list walk no longer waits.
        //  profiles/r05/ab_scalar_diet.txt r05_q13.)
        __builtin_amdgcn_s_setprio(1);
        uint32_t n_cam = 0u;                               // PREHIT: camera rays walked in this iteration (a refill pass; wave-uniform)
        uint32_t pmask = ~0u;                              // PREHIT: the primitives this walk tests (walk_list); all of them in a bounce iteration
        bool walk_cam = true;                              // EMPTY_PASS: false in a refill pass whose pixels' camera rays can hit nothing (wave-uniform)
        if constexpr (PREHIT) {
            n_cam = wc.template refill_size<MI355RT_PREHIT_LOW>(P, lane);
            if (n_cam != 0u) {                             // park the paths' rays; lane i takes the camera ray of sample next + i
                // The pass's samples are consecutive: at spp >= 64 they belong to one pixel or to two neighbours in processing order, and the walk tests
                // only what those pixels' camera rays can hit (two scalar loads; the table is indexed like the band's pixels).  More pixels: everything.
                if (P.cam_mask_off != 0u) {
                    const uint32_t pix0 = fastdiv(wc.next, P.spp_mul, P.spp_shift), pix1 = fastdiv(wc.next + n_cam - 1u, P.spp_mul, P.spp_shift);
                    const __attribute__((address_space(4))) uint32_t* cm = (const __attribute__((address_space(4))) uint32_t*)(P.rows) + P.cam_mask_off + P.band_pixel0;
                    if (pix1 - pix0 <= 1u) { pmask = cm[pix0] | cm[pix1]; if constexpr (EMPTY_PASS) walk_cam = pmask != 0u; }
                }
                wave_lds_handoff();                        // (camera() writes into slots whose entries other lanes were dealt)
                if constexpr (PARK_IN_RING) { stock.e[4u * lane] = make_float4(ps.ro.x, ps.ro.y, ps.ro.z, ps.rd.x); *reinterpret_cast<float2*>(stock.e + 4u * lane + 1u) = make_float2(ps.rd.y, ps.rd.z); }
                else { stock.park_a[lane] = make_float4(ps.ro.x, ps.ro.y, ps.ro.z, ps.rd.x); stock.park_b[lane] = make_float2(ps.rd.y, ps.rd.z); }
                if (lane < n_cam && walk_cam) stock.template camera<RngCtrT<STEP>, RANGE>(P, wc.next + lane, (wc.ring_head + wc.ring_count + lane) & 63u, ps.ro, ps.rd, /* here = 0: sample indices stay below 2^31 (band_samples) */ wc.next >> 31);
            }
        }
        if (n_cam != 0u ? lane < n_cam && walk_cam : live) hit = hit_scene<HAS_MESH, true, KINDS, BOUNDED, RECIP_FIRST, RANGE>(prims, P.n_prims, P.nodes, P.tris, ps.ro, ps.rd, h, pmask);     // renderer.rs:24
        prof.mark(1);
        if constexpr (PREHIT) {
            if (n_cam != 0u) {                             // finish or stock the camera paths, take the parked rays back, and walk them next
                const bool cam = lane < n_cam;
                if (cam) { ++n_paths; ++n_rays; }
                wave_lds_handoff();                        // camera() wrote the keys, append() reads them from other lanes ...
                if constexpr (PARK_IN_RING) {              // ... and writes its entries over the parked rays: every lane takes its own back first
                    const float4 a = stock.e[4u * lane]; const float2 b = *reinterpret_cast<const float2*>(stock.e + 4u * lane + 1u);
                    ps.ro = mk(a.x, a.y, a.z); ps.rd = mk(a.w, b.x, b.y);
                    wave_lds_handoff();
                }
                wc.ring_count += stock.template append<NOSKY, FORM>(P, lane, wc.next, wc.ring_head + wc.ring_count, cam, hit, h, ps.rd);
                wave_lds_handoff();                        // ... and deal_ring() hands the entries it wrote to whichever lanes are idle
                wc.next += n_cam;
                if constexpr (!PARK_IN_RING) {
                const float4 a = stock.park_a[lane]; const float2 b = stock.park_b[lane];
                ps.ro = mk(a.x, a.y, a.z); ps.rd = mk(a.w, b.x, b.y);
                }
                prof.mark(2);
                continue;
            }
        }
        if (!shade_and_regenerate<MATS, false, true, true, !HAS_MESH, /* FASTN */ true, /* TRY1 */ SIMPLE ? 1 : 0, /* REKEY */ false, NOSKY, FORM, RANGE>(P, wc, lane, live, true, hit, h, ps, n_paths, n_rays, prof, stock)) break;
        prof.mark(4);
#ifdef MI355RT_STAMPS
        if (wc.exhausted()) {                              // all work dealt: from here on the wave only drains its own paths
            if (t_dry == 0ull) { t_dry = __builtin_amdgcn_s_memrealtime(); live_at_dry = (uint32_t)__popcll(__ballot(live)); }
            ++drain_iters;
        }
#endif
    }
#ifdef MI355RT_STAMPS
    if (lane == 0 && P.stats) { for (int i = 0; i < 6; ++i) atomicAdd(&P.stats[2 + i], prof.acc[i]); for (int i = 0; i < 10; ++i) atomicAdd(&P.stats[24 + i], prof.cls[i]); }
    if (P.wave_times) {
        const unsigned long long t_wave1 = __builtin_amdgcn_s_memrealtime();
        const uint32_t wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        const uint32_t np = wave_sum(n_paths);
        if (lane == 0) {
            unsigned long long* w = P.wave_times + WAVE_TIME_WORDS * (size_t)wid;
            w[0] = t_wave0; w[1] = t_wave1; w[2] = np; w[3] = t_dry ? t_dry : t_wave1; w[4] = drain_iters; w[5] = live_at_dry;
        }
    }
#endif
    const uint32_t wp = wave_sum(n_paths), wr = wave_sum(n_rays);
    if (lane == 0 && P.stats) { atomicAdd(&P.stats[0], (unsigned long long)wp); atomicAdd(&P.stats[1], (unsigned long long)wr); }
}

// Entry points: one body, instantiated per scene class so that each gets its own register budget.
//   k_render_ctr_nomesh     any materials, no mesh in the list                      (any other mesh-free list)                        6 waves/SIMD
//   k_render_ctr_simple     Lambertian/Emissive/Null only, no mesh                  (-3 % vs nomesh on cornell)                       7 waves/SIMD
//   k_render_ctr_simple_qc  the same for lists of quads and cubes only, no sky      (cornell: another -1.1 %; without the sky lookup) 8 waves/SIMD
//   k_render_sky_simple_qc  its twin for scenes with a sky texture                  (the body with the lookup)                        7 waves/SIMD
//   k_render_ctr_nospec     no metal, no dielectric, no mesh                        (-2.5 % vs nomesh on veach-mis; the probe kernel) 7 waves/SIMD
//   k_render_ctr_mesh       lockstep with the per-lane BVH walk inlined             (diagnostic knob; the two degenerate renders: an empty list, max_depth 0)
// Which kernels keep the generator's draw address in LCG-stepped form (rt_rng.h, RngCtrT<true>): one bit per kernel.  The form saves the generator's
// four-multiply LCG step in every block after a path's first, and moves the register allocation of every kernel it touches; a kernel keeps it only where
// its figures stay inside tests/test_isa_budget.py with no more SGPR spills and no more v_readlane / v_writelane in its loop than the plain form has
// (profiles/isa_diff_stepped_generator_vs_parent.txt), and where it measures faster on the kernel's workload (profiles/bench_stepped_generator_vs_parent.txt).
// A kernel whose bit is clear compiles to the instructions it had before the form existed.  -DMI355RT_STEP_MASK=... builds the other choices for A/B.
enum : uint32_t { STEP_SIMPLE_QC = 1u, STEP_SIMPLE = 2u, STEP_NOSPEC = 4u, STEP_NOMESH = 8u, STEP_MESH = 16u, STEP_WF = 32u, STEP_WF_NOMETAL = 64u,
                  STEP_WF_NOMETAL_SHALLOW = 128u, STEP_WF_NOMETAL_IDENT = 256u, STEP_WF_MESHFREE = 512u, STEP_WF_FIXAABB = 1024u };
#ifndef MI355RT_STEP_MASK
#define MI355RT_STEP_MASK (STEP_SIMPLE_QC)
#endif
constexpr bool step_form(uint32_t kernel_bit) { return ((uint32_t)(MI355RT_STEP_MASK) & kernel_bit) != 0u; }
__global__ void __launch_bounds__(BLOCK_THREADS) MI355RT_OCC_LS k_render_ctr_nomesh(const RenderParams P) { render_ctr_lockstep<false, MATS_ALL, PRIMS_ALL, false, false, step_form(STEP_NOMESH)>(P); }
__global__ void __launch_bounds__(BLOCK_THREADS) MI355RT_OCC_SIMPLE k_render_ctr_simple(const RenderParams P) { render_ctr_lockstep<false, MATS_LAMBERT, PRIMS_ALL, false, false, step_form(STEP_SIMPLE)>(P); }
// ... and the Lambert-only kernel for lists of quads and cubes (round 5: cornell -1.1 %, profiles/r05/ab_scalar_diet.txt r05_q16), with its camera rays'
// first hits in stock (HitStock: cornell -3.7 %, profiles/ab_stocked_first_hits.txt)
// Variant 14 has two entry points.  k_render_ctr_simple_qc is compiled WITHOUT the sky lookup and serves the scenes without a sky texture (cornell);
// k_render_sky_simple_qc is the body with the lookup, for the scenes that carry one.  launch_render_ctr picks by RenderParams.sky.
__global__ void __launch_bounds__(BLOCK_THREADS) MI355RT_OCC_NOSKY k_render_ctr_simple_qc(const RenderParams P) { render_ctr_lockstep<false, MATS_LAMBERT, PRIMS_QUAD_CUBE, /* PREHIT */ true, /* BOUNDED */ true, step_form(STEP_SIMPLE_QC), /* NOSKY */ true, MI355RT_QC_FORM>(P); }
__global__ void __launch_bounds__(BLOCK_THREADS) MI355RT_OCC_SIMPLE k_render_sky_simple_qc(const RenderParams P) { render_ctr_lockstep<false, MATS_LAMBERT, PRIMS_QUAD_CUBE, /* PREHIT */ true, /* BOUNDED */ true, step_form(STEP_SIMPLE_QC)>(P); }
__global__ void __launch_bounds__(BLOCK_THREADS) MI355RT_OCC_SIMPLE k_render_ctr_nospec(const RenderParams P) { render_ctr_lockstep<false, MATS_NO_SPECULAR, PRIMS_ALL, false, false, step_form(STEP_NOSPEC)>(P); }
__global__ void __launch_bounds__(BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(6, 6))) k_render_ctr_mesh(const RenderParams P) { render_ctr_lockstep<true, MATS_ALL, PRIMS_ALL, false, false, step_form(STEP_MESH)>(P); }

}  // namespace mi355rt

// Round 1's form of the mesh path -- the in-wave state machine -- is retired from the product library: it is compiled only into the
// tests' reference build (-DMI355RT_REFS, build.build_device_variant("refs")), where it serves as a bit-identity reference for the
// wavefront kernel.  k_render_ctr_mesh above stays in the product library: the plain
// per-lane loop is the simplest statement of the BVH walk and what the diagnostic knob "kernel" = 1 selects.
#ifdef MI355RT_REFS
#include "rt_mesh_variants.h"   // k_render_ctr_sm (uses the shared pieces above)
#endif
#include "rt_wavefront.h"       // k_render_ctr_wf

namespace mi355rt {

// ===================================================================================================
// k_resolve -- ordered per-pixel sum, 1/spp, sqrt gamma, pack (renderer.rs:100-120), without LDS.
// One pixel's samples are contiguous in HBM (spp * 16 B apart from the next pixel's) and must be added in sample order.
// A 16-lane DPP row owns one pixel; lane s of the row loads sample
// c + s (64 lanes = 4 pixels x 16 samples = four fully coalesced 256-byte segments), and the sequential sum
// ((acc + x0) + x1) + ... + x15 runs ALONG the row: T = row_shr:1(T) + x, fifteen times.  Lane k's value is final after
// step k and every later step recomputes exactly the same sum (its left neighbour no longer changes), so no select is
// needed; lane 0 reads 0 from outside the row (bound_ctrl) and 0 + (acc + x0) is exact (a running sum that started at
// +0 is never -0).  Samples past spp enter as +0, which leaves a sum unchanged.  No LDS, 14 VGPRs: enough waves in
// flight to keep the HBM read stream busy (6.4 TB/s; the LDS-transpose version it replaces reached 3.3).
// ===================================================================================================
#ifndef MI355RT_RESOLVE_SKIP
#define MI355RT_RESOLVE_SKIP 1                               // 0 builds k_resolve as it was: ResolveParams.cam_mask is not looked at
#endif
DI float dpp_row_shr1_zero(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true)); }
DI float dpp_row_ror1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xF, 0xF, true)); }
__global__ void __launch_bounds__(256) k_resolve(const ResolveParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t s = lane & 15u;
    const uint32_t p = wave * 4u + (lane >> 4);                  // this row's pixel within the band
    const bool valid = p < P.band_pixels;
    size_t o = (size_t)P.band_pixel0 + p;                        // the pixel's number in processing order ...
    if (P.out_row && valid) {                                    // ... and where it belongs in the output (rows are processed dearest first, rt_api.cpp)
        const uint32_t jp = fastdiv((uint32_t)o, P.width_mul, P.width_shift);
        o = (size_t)P.out_row[jp] * P.width + ((uint32_t)o - jp * P.width);
    }
    const float* __restrict__ rad = P.radiance + 3u * (size_t)(valid ? p : 0u) * P.spp;     // 3 floats per sample
    float4* __restrict__ accum = reinterpret_cast<float4*>(P.accum);
    f3 acc = mk(0.f, 0.f, 0.f);                                  // meaningful in lane 0 of the row
    if (accum && P.accum_load && valid) { const float4 a = accum[o]; acc = mk(a.x, a.y, a.z); }
    // A pixel that no camera ray can leave with a hit (its camera-mask word is 0, rt_prepare.cpp build_camera_masks): each of its samples is the
    // constant the render kernel stored, so the row feeds that constant to the same chain and reads nothing.  The same instructions on the same values.
    constexpr bool RESOLVE_SKIP = MI355RT_RESOLVE_SKIP != 0;
    bool empty = false;
    if constexpr (RESOLVE_SKIP) { if (P.cam_mask && valid) empty = P.cam_mask[p] == 0u; }
    for (uint32_t c = 0; c < P.spp; c += 16u) {
        f3 x = mk(0.f, 0.f, 0.f);
        if (valid && c + s < P.spp) {
            const float* q = rad + 3u * (c + s);
            if (RESOLVE_SKIP && empty) x = mk(1.f, 1.f, 1.f) * mk(P.miss[0], P.miss[1], P.miss[2]);      // what the render kernel stored there (HitStock::append, a miss at throughput 1)
            else x = mk(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2));
        }
        if (s == 0u) x = acc + x;                                 // renderer.rs:100 goes on where the previous 16 samples stopped
        f3 t = x;
#pragma unroll
        for (int k = 0; k < 15; ++k) t = mk(dpp_row_shr1_zero(t.x) + x.x, dpp_row_shr1_zero(t.y) + x.y, dpp_row_shr1_zero(t.z) + x.z);
        acc = mk(dpp_row_ror1(t.x), dpp_row_ror1(t.y), dpp_row_ror1(t.z));   // lane 0 <- lane 15: the sum so far
    }
    if (!valid || s != 0u) return;
    const f3 pixel = acc * P.inv_spp;                            // renderer.rs:103
    if (accum) accum[o] = make_float4(acc.x, acc.y, acc.z, 0.0f);
    if (P.out_linear) { P.out_linear[3 * o] = pixel.x; P.out_linear[3 * o + 1] = pixel.y; P.out_linear[3 * o + 2] = pixel.z; }
    P.out_packed[o] = color_to_u32(sqrt3(pixel));                // renderer.rs:112-120
}

// ===================================================================================================
// k_render_ref -- validation: replay of the reference's per-row sequential stream, one lane per row
// ===================================================================================================
__global__ void __launch_bounds__(64) k_render_ref(const RefParams P) {
    cprim_t prims = (cprim_t)(P.prims);
    // One row per WAVE, carried by lane 0: rows consume their streams at data-dependent rates, so 64 rows in one wave
    // would run in lockstep through 64 different control flows; one active lane per wave has no divergence and the
    // rows spread over all CUs (the chip is otherwise idle in this validation mode).
    if ((threadIdx.x & 63u) != 0u) return;
    const uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= P.n_rows) return;
    const uint32_t y = P.rows[j];
    RngRef rng;
    rng.seed_from_u64((uint64_t)y + (((uint64_t)P.seed_hi << 32) | (uint64_t)P.seed_lo));      // renderer.rs:91
    float* __restrict__ stack = P.fold_stack + (size_t)j * P.max_depth * 3;
    const float inv_spp = 1.0f / (float)P.spp;                                                  // renderer.rs:85
    unsigned long long n_rays = 0;
    for (uint32_t x = 0; x < P.width; ++x) {                                                    // renderer.rs:93
        f3 acc = mk(0.f, 0.f, 0.f);
        for (uint32_t s = 0; s < P.spp; ++s) {                                                  // renderer.rs:95
            const float u = ((float)x + rng.jitter_u()) / (float)P.width;
            const float v = ((float)y + rng.jitter_v()) / (float)P.height;
            f3 ro, rd; camera_ray(P.cam, u, v, ro, rd);
            f3 term = mk(0.f, 0.f, 0.f);
            uint32_t depth = 0;
            for (;;) {
                if (depth == P.max_depth) break;
                ++n_rays;
                Hit h;
                if (!hit_scene<true>(prims, P.n_prims, P.nodes, P.tris, ro, rd, h)) { term = miss_colour(P.sky, P.sky_w, P.sky_h, P.miss, rd); break; }
                f3 no, nd, atten, emitted;
                const float4 q0 = reinterpret_cast<const float4*>(P.mats + (h.mat_ff & 0x7FFFFFFFu))[0];
                if (!surface_scatter(P.mats, P.textures, q0, h, rd, rng, no, nd, atten, emitted)) { term = emitted; break; }
                stack[3 * depth] = atten.x; stack[3 * depth + 1] = atten.y; stack[3 * depth + 2] = atten.z;
                ro = no; rd = nd; ++depth;
            }
            f3 L = term;                                                                        // fold tail-first: emitted + atten * scattered (renderer.rs:33)
            for (uint32_t d = depth; d-- > 0;) L = mk(0.f, 0.f, 0.f) + mk(stack[3 * d], stack[3 * d + 1], stack[3 * d + 2]) * L;
            acc = acc + L;                                                                      // renderer.rs:100-101
        }
        const f3 pixel = acc * inv_spp;                                                         // renderer.rs:103
        const size_t o = (size_t)j * P.width + x;
        if (P.out_linear) { P.out_linear[3 * o] = pixel.x; P.out_linear[3 * o + 1] = pixel.y; P.out_linear[3 * o + 2] = pixel.z; }
        P.out_packed[o] = color_to_u32(sqrt3(pixel));
    }
    if (P.stats) { atomicAdd(&P.stats[0], (unsigned long long)P.width * P.spp); atomicAdd(&P.stats[1], n_rays); }
}

// ===================================================================================================
// k_gather_strips -- the exchange of mi355rt_multi_context_render (rt_multi.cpp): the parts' rows arrive (peer copies) back to back in
// one staging area of the destination device, and output row r of the packed (width words) and linear (3 * width words) images is
// staging row src_row[r].  A pure copy of a few MB: a workgroup takes one row at a time (grid-stride over rows), so the row, its table
// entry (a scalar load) and the alignment test are uniform; a row whose source and destination both start on 16 bytes moves as dwordx4
// (cdna_hip_programming Guideline 13) plus a tail of < 4 words, any other row (width not a multiple of 4) as dwords.
// ===================================================================================================
DI void gather_row(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n) {
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0u) {
        const uint32_t nq = n >> 2;
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);
        uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t i = threadIdx.x; i < nq; i += blockDim.x) d4[i] = s4[i];
        const uint32_t t = (nq << 2) + threadIdx.x;
        if (t < n) dst[t] = src[t];                                   // (threadIdx.x < 4 <= blockDim.x)
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    }
}
__global__ void __launch_bounds__(256) k_gather_strips(const GatherParams P) {
    const __attribute__((address_space(4))) uint32_t* table = (const __attribute__((address_space(4))) uint32_t*)P.src_row;   // uniform reads -> s_load
    for (uint32_t r = blockIdx.x; r < P.n_rows; r += gridDim.x) {
        const size_t s = table[r];
        gather_row(P.src_packed + s * P.width, P.dst_packed + (size_t)r * P.width, P.width);
        if (P.dst_linear) gather_row(P.src_linear + s * 3u * P.width, P.dst_linear + (size_t)r * 3u * P.width, 3u * P.width);
    }
}

// k_gather_accum -- the running sums of mi355rt_multi_context_render_progressive (rt_multi.cpp), assembled like the images above: every
// part's float4 sums arrive (peer copies) back to back in a staging area of the destination device, and output row r is staging row
// src_row[r] (k_gather_strips' table).  A row is `width` float4 = 16 * width bytes, so every row of either side starts on 16 bytes (both
// buffers are 16-byte aligned, the caller's as in mi355rt_context_render_progressive): dwordx4 loads and stores only, no tail.  A workgroup
// takes one row at a time (grid-stride), the table entry is a uniform scalar load.
__global__ void __launch_bounds__(256) k_gather_accum(const GatherAccumParams P) {
    const __attribute__((address_space(4))) uint32_t* table = (const __attribute__((address_space(4))) uint32_t*)P.src_row;   // uniform reads -> s_load
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(P.src);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(P.dst);
    for (uint32_t r = blockIdx.x; r < P.n_rows; r += gridDim.x) {
        const uint4* __restrict__ s4 = src + (size_t)table[r] * P.width;
        uint4* __restrict__ d4 = dst + (size_t)r * P.width;
        for (uint32_t i = threadIdx.x; i < P.width; i += blockDim.x) d4[i] = s4[i];
    }
}

// ===================================================================================================
// Diagnostic kernels: one Material::scatter / one HittableList::hit per lane through the device functions above
// (tests/test_kat_functions.py compares them with independent numpy float32 known answers).
// ===================================================================================================
__global__ void __launch_bounds__(64) k_debug_scatter(const DevMat* __restrict__ mats, const DevTexture* __restrict__ texs, const DebugScatterIn* __restrict__ in, DebugScatterOut* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DebugScatterIn r = in[i];
    Hit h; h.t = 0.f; h.p = mk(r.p[0], r.p[1], r.p[2]); h.n = mk(r.n[0], r.n[1], r.n[2]);
    h.mat_ff = r.material | (r.front_face ? 0x80000000u : 0u);
    RngCtrT<true> rng; rng.start(r.k0, r.k1, r.x, r.s); rng.set_ray(r.ray); rng.load_block0();     // (the stepped form: any ray number, any try number)
    const float4 q0 = reinterpret_cast<const float4*>(mats + r.material)[0];
    f3 no = mk(0, 0, 0), nd = mk(0, 0, 0), atten = mk(0, 0, 0), emitted = mk(0, 0, 0);
    const bool ok = surface_scatter(mats, texs, q0, h, mk(r.rd[0], r.rd[1], r.rd[2]), rng, no, nd, atten, emitted);
    DebugScatterOut o{};
    o.scattered = ok ? 1.0f : 0.0f;
    o.o[0] = no.x; o.o[1] = no.y; o.o[2] = no.z; o.d[0] = nd.x; o.d[1] = nd.y; o.d[2] = nd.z;
    o.atten[0] = atten.x; o.atten[1] = atten.y; o.atten[2] = atten.z; o.emitted[0] = emitted.x; o.emitted[1] = emitted.y; o.emitted[2] = emitted.z;
    out[i] = o;
}
__global__ void __launch_bounds__(64) k_debug_hit(const DevPrim* prims_, uint32_t n_prims, const DevNode* __restrict__ nodes, const DevTri* __restrict__ tris,
                                                  const DebugHitIn* __restrict__ in, DebugHitOut* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DebugHitIn r = in[i];
    const f3 ro = mk(r.o[0], r.o[1], r.o[2]), rd = normalized(mk(r.d[0], r.d[1], r.d[2]));       // Ray::new, ray.rs:12-17
    Hit h;
    const bool hit = hit_scene<true>((cprim_t)prims_, n_prims, nodes, tris, ro, rd, h);
    DebugHitOut o{};
    o.hit = hit ? 1.0f : 0.0f;
    if (hit) {
        o.p[0] = h.p.x; o.p[1] = h.p.y; o.p[2] = h.p.z; o.n[0] = h.n.x; o.n[1] = h.n.y; o.n[2] = h.n.z; o.t = h.t;
        o.material = (float)(h.mat_ff & 0x7FFFFFFFu); o.front_face = (h.mat_ff >> 31) ? 1.0f : 0.0f;
    }
    out[i] = o;
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int launch_debug_scatter(const DevMat* mats, const DevTexture* textures, const DebugScatterIn* in, DebugScatterOut* out, uint32_t n, void* stream) {
    hipLaunchKernelGGL(k_debug_scatter, dim3((n + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, mats, textures, in, out, n);
    return (int)hipGetLastError();
}
int launch_debug_hit(const DevPrim* prims, uint32_t n_prims, const DevNode* nodes, const DevTri* tris, const DebugHitIn* in, DebugHitOut* out, uint32_t n, void* stream) {
    hipLaunchKernelGGL(k_debug_hit, dim3((n + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, prims, n_prims, nodes, tris, in, out, n);
    return (int)hipGetLastError();
}
// The counter-mode kernels by variant (rt_device.h, VARIANT_TABLE); null where this build holds none: the reference build's state machine
// outside -DMI355RT_REFS, the retired numbers always.
#define KFN(k) reinterpret_cast<const void*>(k)
#ifdef MI355RT_REFS
#define REFS_KFN(k) KFN(k)
#else
#define REFS_KFN(k) nullptr
#endif
static const void* const render_ctr_kernel[KERNEL_VARIANTS] = {
    KFN(k_render_ctr_nomesh), KFN(k_render_ctr_mesh), REFS_KFN(k_render_ctr_sm), KFN(k_render_ctr_simple), REFS_KFN(k_render_ctr_sm_fixaabb),
    nullptr, nullptr, KFN(k_render_ctr_wf), KFN(k_render_ctr_wf_fixaabb), KFN(k_render_ctr_nospec), KFN(k_render_ctr_wf_nometal),
    KFN(k_render_ctr_wf_meshfree), KFN(k_render_ctr_wf_nometal_ident), KFN(k_render_ctr_wf_nometal_shallow), KFN(k_render_ctr_simple_qc)};
#undef KFN
#undef REFS_KFN
bool render_ctr_variant_built(uint32_t variant) { return variant < KERNEL_VARIANTS && render_ctr_kernel[variant]; }
// The entry point of `variant` for a scene with (ENTRY_SKY) or without (ENTRY_PLAIN) a sky texture: one kernel for both everywhere but at variant 14.
static const void* render_ctr_entry(uint32_t variant, uint32_t entry) {
    return variant_entry(variant, entry == ENTRY_SKY) == ENTRY_SKY ? reinterpret_cast<const void*>(k_render_sky_simple_qc) : render_ctr_kernel[variant];
}
int launch_render_ctr(const RenderParams& p, uint32_t variant, uint32_t grid_blocks, void* stream) {
    if (!render_ctr_variant_built(variant)) return -1;
    void* args[] = {const_cast<RenderParams*>(&p)};
    // (by the pointer the kernel would read: the entry compiled without the lookup never sees a texture)
    (void)hipLaunchKernel(render_ctr_entry(variant, p.sky ? ENTRY_SKY : ENTRY_PLAIN), dim3(grid_blocks), dim3(VARIANT_TABLE[variant].block_threads), args, 0, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int launch_resolve(const ResolveParams& p, void* stream) {
    const uint32_t blocks = (p.band_pixels + 15u) / 16u;         // 4 waves x 4 pixels per block
    hipLaunchKernelGGL(k_resolve, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
int launch_gather_strips(const GatherParams& p, void* stream) {
    if (p.n_rows == 0) return 0;
    const uint32_t blocks = p.n_rows < 2048u ? p.n_rows : 2048u;   // one row per workgroup at a time; more rows are strided over
    hipLaunchKernelGGL(k_gather_strips, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
int launch_gather_accum(const GatherAccumParams& p, void* stream) {
    if (p.n_rows == 0) return 0;
    const uint32_t blocks = p.n_rows < 2048u ? p.n_rows : 2048u;   // as launch_gather_strips
    hipLaunchKernelGGL(k_gather_accum, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
int launch_render_ref(const RefParams& p, void* stream) {
    hipLaunchKernelGGL(k_render_ref, dim3(p.n_rows), dim3(64), 0, (hipStream_t)stream, p);      // one wave per row
    return (int)hipGetLastError();
}
int query_render_ctr_occupancy(uint32_t variant, uint32_t entry, int* blocks_per_cu, int* vgprs, int* sgprs) {
    if (!render_ctr_variant_built(variant)) return -1;
    const void* fn = render_ctr_entry(variant, entry);
    int nb = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, (int)VARIANT_TABLE[variant].block_threads, 0);
    if (e != hipSuccess) return (int)e;
    hipFuncAttributes fa;
    e = hipFuncGetAttributes(&fa, fn);
    if (e != hipSuccess) return (int)e;
    *blocks_per_cu = nb; *vgprs = fa.numRegs; *sgprs = 0;
    return 0;
}

}  // namespace mi355rt
