/*
 * mi355rt.h -- C ABI of the MI355X-native render loop.
 *
 * This is the drop-in boundary for ONE call of the reference:
 *
 *     let buffer = render_scene(&scene, &camera, &render_settings);      // src/main.rs:57
 *     pub fn render_scene(scene: &Scene, camera: &Camera,
 *                         render_settings: &RenderSettings) -> Vec<u32>  // src/renderer.rs:67
 *
 * The reference has no FFI of its own, so the entry points below are
 * what a `#[repr(C)]` / `extern "C"` binding added at src/main.rs:57 would bind (the stub is in
 * INTEGRATION.md).  Every struct is plain-old-data, little-endian f32/u32, no pointers inside
 * arrays, and the caller owns every buffer it passes in.
 *
 * Conventions
 *   - return value 0 = OK, negative = error; nothing aborts, nothing throws across the ABI (every
 *     entry point of both libraries runs inside an exception barrier: a failed host allocation is
 *     MI355RT_ERR_OOM, any other C++ exception MI355RT_ERR_HIP / _IO with its text);
 *     mi355rt_last_error() returns a thread-local message for the last failure.
 *   - output layout == render_scene's Vec<u32>: width*height, row-major, row 0 = top,
 *     0x00RRGGBB (src/color.rs:87-93).
 *   - matrices are column-major 4x4 as glam::Mat4 stores them (x_axis, y_axis, z_axis, w_axis).
 *   - the top-level primitive array is walked in array order, exactly as
 *     HittableList::hit walks `objects` (src/hittable.rs:45-58): order changes tie-breaks.
 *   - the libraries read NO environment variables: everything that selects behaviour is in the structs below.
 */
#ifndef MI355RT_H
#define MI355RT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355RT_ABI_VERSION 5u   /* 2: mi355rt_scene.textures, MI355RT_MAT_TEXTURE; 3: mi355rt_context_check exported, quads must carry a (near-)unit normal;
                                    4: mi355rt_context_set_share exported; MI355RT_RNG_CTR draws from pcg4d (other numbers than versions 1-3, same distribution);
                                    5: mi355rt_multi_context_* exported.  No struct changed in 5: options.abi_version 4 is still accepted.
                                    Added within version 5 (no struct changed, the number stays): mi355rt_multi_context_render_progressive and
                                    mi355rt_render_progressive_multi -- a caller that needs them probes for the symbols (dlsym), not the number.
                                    Likewise the ray queries: mi355rt_context_trace_rays, mi355rt_context_first_hits, mi355rt_trace_rays;
                                    and the denoiser: mi355rt_denoise_scratch_bytes, mi355rt_context_denoise, mi355rt_denoise;
                                    and the occlusion queries: mi355rt_context_occluded, mi355rt_occluded, mi355rt_context_ambient_occlusion;
                                    and the radiance queries: mi355rt_radiance_scratch_bytes, mi355rt_context_trace_radiance, mi355rt_trace_radiance;
                                    and the camera views: mi355rt_view_scratch_bytes, mi355rt_context_view_rays, mi355rt_context_render_view;
                                    and the surface probes: mi355rt_context_probe_rays, mi355rt_context_probe_radiance;
                                    and, in the host library, the noise estimate: mi355rt_noise_create, mi355rt_noise_free, mi355rt_noise_reset,
                                    mi355rt_noise_update, mi355rt_noise_evaluate;
                                    and, in the device library, the same estimate on device memory: mi355rt_noise_device_create, mi355rt_noise_device_destroy,
                                    mi355rt_noise_device_reset, mi355rt_noise_device_update, mi355rt_noise_device_evaluate. */

/* ---- error codes ------------------------------------------------------------------------- */
#define MI355RT_OK               0
#define MI355RT_ERR_INVALID     -1   /* malformed scene / settings / options                    */
#define MI355RT_ERR_NO_DEVICE   -2   /* no usable HIP device (there is NO CPU fallback)          */
#define MI355RT_ERR_HIP         -3   /* a HIP runtime call or a kernel failed                    */
#define MI355RT_ERR_OOM         -4   /* host or device allocation failed                         */
#define MI355RT_ERR_IO          -5   /* file could not be read / parsed (host-side loaders)      */
#define MI355RT_ERR_UNSUPPORTED -6   /* feature flagged in the ABI but not built                   */

/* ---- camera: src/camera.rs:4-11 (the fields of `Camera`, computed by Camera::new on the host) */
typedef struct mi355rt_camera {
    float position[3];
    float forward[3];
    float right[3];
    float true_up[3];
    float half_width;
    float half_height;
} mi355rt_camera;

/* ---- render settings: src/tungsten/parser.rs:191-197 (`RenderSettings`) ---------------------- */
typedef struct mi355rt_settings {
    uint32_t width;
    uint32_t height;
    uint32_t samples_per_pixel;
    uint32_t max_depth;
} mi355rt_settings;

/* ---- materials: the eight `impl Material` types (src/material.rs, src/tungsten/materials.rs) - */
enum {
    MI355RT_MAT_LAMBERT_SOLID   = 0, /* material.rs:47-71, AlbedoKind::Solid     albedo           */
    MI355RT_MAT_LAMBERT_CHECKER = 1, /* material.rs:47-71, AlbedoKind::Checked   albedo=on, aux=off, p0=inv_scale */
    MI355RT_MAT_METAL           = 2, /* material.rs:87-110                       albedo, p0=fuzz  */
    MI355RT_MAT_DIELECTRIC      = 3, /* material.rs:122-162                      p0=refractive_index */
    MI355RT_MAT_EMISSIVE        = 4, /* material.rs:169-192                      albedo=color     */
    MI355RT_MAT_PLASTIC         = 5, /* tungsten/materials.rs:29-65              albedo, p0=ior   */
    MI355RT_MAT_ROUGH_GGX       = 6, /* tungsten/materials.rs:306-377 (Ggx)      albedo, p0=roughness, eta, k */
    MI355RT_MAT_ROUGH_BECKMANN  = 7, /* tungsten/materials.rs:306-377 (Beckmann) albedo, p0=roughness, eta, k */
    MI355RT_MAT_NULL            = 8, /* material.rs:229-252 (never scatters, never emits)         */
    MI355RT_MAT_TEXTURE         = 9, /* tungsten/parser.rs:199-243 TextureMaterial: Lambert bounce, albedo * texel looked up by the
                                        hit NORMAL (equirect, nearest);  albedo, p0=h_offset, texture=index into scene.textures.
                                        No loader path of the reference produces it (parser.rs:315-424 never yields Texture);
                                        a host that builds its Scene in code can. */
    MI355RT_MAT_KIND_COUNT      = 10
};

typedef struct mi355rt_material {      /* 64 bytes */
    uint32_t kind;
    float    albedo[3];
    float    aux[3];
    float    p0;
    float    p1;
    float    eta[3];                   /* MetalType::ior_k().0, tungsten/materials.rs:115-152      */
    float    k[3];                     /* MetalType::ior_k().1                                     */
    uint32_t texture;                  /* MI355RT_MAT_TEXTURE: index into mi355rt_scene.textures; 0 otherwise */
} mi355rt_material;

/* An 8-bit RGBA image as `image::RgbaImage` holds it (parser.rs:201): row-major, row 0 = top, 4 bytes per pixel. */
typedef struct mi355rt_texture {
    const uint8_t* rgba8;
    uint32_t width, height;
} mi355rt_texture;

/* ---- top-level primitives: the five `impl Hittable` types ------------------------------------ */
enum {
    MI355RT_PRIM_SPHERE = 0, /* src/objects/sphere.rs:9-13   data: center[3], radius                */
    MI355RT_PRIM_PLANE  = 1, /* src/objects/plane.rs:9-13    data: p1[3], normal[3] (unit)          */
    MI355RT_PRIM_QUAD   = 2, /* src/tungsten/objects/quad.rs:10-21  data: base[3], edge0[3], edge1[3],
                                normal[3], d, inv_edge0_len_sq, inv_edge1_len_sq                    */
    MI355RT_PRIM_CUBE   = 3, /* src/objects/cube.rs:11-17    data: object_to_world[16], world_to_object[16] */
    MI355RT_PRIM_MESH   = 4, /* src/mesh/mesh_object.rs:17-22 data: object_to_world[16], world_to_object[16];
                                `mesh` indexes mi355rt_scene.meshes                                 */
    MI355RT_PRIM_KIND_COUNT = 5
};

typedef struct mi355rt_primitive {     /* 144 bytes */
    uint32_t kind;
    uint32_t material;                 /* index into mi355rt_scene.materials                       */
    uint32_t mesh;                     /* MI355RT_PRIM_MESH only                                   */
    uint32_t _pad;
    float    data[32];
} mi355rt_primitive;

/* ---- mesh payload: src/mesh/triangle.rs:5-11 and src/acceleration/bvh.rs:7-12 ----------------- */
typedef struct mi355rt_triangle {      /* object space, 48 bytes; `material` lives on the primitive */
    float v0[3];
    float v1[3];
    float v2[3];
    float normal[3];                   /* Triangle::new, triangle.rs:14-25                          */
} mi355rt_triangle;

/* One BVHNode, flattened by any visitor.  Indices are relative to the owning mesh's
 * first_node / first_index.  Inner node: index_count == 0, left/right = child node indices.
 * Leaf: index_count > 0 and [first_index, first_index+index_count) is its `triangle_indices`
 * list (values index the mesh's triangles).  Node 0 of a mesh is its root.                       */
typedef struct mi355rt_bvh_node {      /* 40 bytes */
    float    bmin[3];
    float    bmax[3];
    uint32_t left;
    uint32_t right;
    uint32_t first_index;
    uint32_t index_count;
} mi355rt_bvh_node;

typedef struct mi355rt_mesh {
    uint32_t first_triangle, triangle_count;   /* range in mi355rt_scene.triangles               */
    uint32_t first_node, node_count;           /* range in mi355rt_scene.nodes                    */
    uint32_t first_index, index_count;         /* range in mi355rt_scene.tri_indices              */
    uint32_t max_depth;                        /* depth of the deepest node (root = 0); 0 = unknown */
    uint32_t _pad;
} mi355rt_mesh;

/* ---- the scene: src/scene.rs:6-10 flattened --------------------------------------------------- */
typedef struct mi355rt_scene {
    const mi355rt_primitive* primitives;  uint32_t n_primitives;
    const mi355rt_material*  materials;   uint32_t n_materials;
    const mi355rt_mesh*      meshes;      uint32_t n_meshes;
    const mi355rt_triangle*  triangles;   uint32_t n_triangles;
    const mi355rt_bvh_node*  nodes;       uint32_t n_nodes;
    const uint32_t*          tri_indices; uint32_t n_tri_indices;
    /* Colours -- miss_color, sky texels, albedos, emitted colours -- are not validated: non-finite and out-of-range values are accepted
     * and propagate as in the reference's f32 arithmetic (inf * 0 = NaN: a path that runs out of depth with an infinite throughput is NaN,
     * not black; sums overflow to +-inf; negative and denormal values stay what they are) through the path ends, the sample-order sum,
     * the progressive sums and the multi-device gathers into the linear output.  The packed pixel is sqrt, clamp(0, 1) where NaN stays,
     * * 255, saturating conversion: NaN and negative channels pack as 0, +inf as 255. */
    float        miss_color[3];           /* Color::GRAY at HEAD, src/renderer.rs:61             */
    uint32_t     sky_width, sky_height;   /* equirect HDR skybox, src/renderer.rs:40-54; 0 = none */
    const float* sky_rgb;                 /* sky_width*sky_height*3 f32, row 0 = top; NULL = constant miss_color */
    const mi355rt_texture* textures;      uint32_t n_textures;   /* images of the MI355RT_MAT_TEXTURE materials (ABI 2) */
} mi355rt_scene;

/* ---- options that have no counterpart in the reference ---------------------------------------- */
enum {
    MI355RT_RNG_CTR = 0, /* counter-based per-ray generator (pcg4d since round 5, Philox4x32-10 before) addressed by (row y; x, sample, ray, block).
                            GPU-native default; any tiling gives bit-identical images.           */
    MI355RT_RNG_REF = 1  /* replay of the reference stream: StdRng::seed_from_u64(y) shared by a
                            whole row (src/renderer.rs:91). One lane per row -- validation only.   */
};

/* options.flags */
/* Opt-in fix, never the default (it changes the image): the BVH slab test misses a box only when t_max < t_min.
 * The reference tests t_max <= t_min (src/acceleration/aabb.rs:41), so boxes of zero thickness -- every leaf of
 * axis-aligned flat geometry -- are never entered and their triangles are invisible.
 * Counter-mode RNG only. */
#define MI355RT_FLAG_FIXED_AABB 1u

typedef struct mi355rt_options {
    uint32_t abi_version;     /* MI355RT_ABI_VERSION                                               */
    uint32_t rng_mode;        /* MI355RT_RNG_*                                                     */
    uint64_t seed;            /* 0 reproduces the reference: row key = y + seed                    */
    /* Row selection. Rows are dealt in strips of `strip_rows` rows; this call renders the strips
     * with (strip_index % n_parts) == part, restricted to [row_begin, row_end).  The output
     * buffers then hold ONLY those rows, packed in ascending row order.
     * {0, height, 1, 1, 0} renders the whole image.  row_end == 0 means `height`.               */
    uint32_t row_begin, row_end;
    uint32_t strip_rows, n_parts, part;
    uint32_t flags;             /* MI355RT_FLAG_*; 0 reproduces the reference                      */
    uint64_t workspace_bytes; /* cap for the per-sample radiance workspace in HBM; 0 = default (32 GiB,
                                 of which only width*rows*spp*12 bytes are allocated)             */
} mi355rt_options;

typedef struct mi355rt_stats {
    double   render_kernel_ms;   /* sum over bands of the path-tracing kernel, HIP events          */
    double   resolve_kernel_ms;  /* sum over bands of the ordered sum + gamma + pack kernel        */
    double   total_ms;           /* first launch -> last kernel done (device timeline)             */
    uint64_t samples;            /* camera paths started                                           */
    uint64_t rays;               /* trace_ray invocations that intersected the scene               */
    uint32_t rows_rendered;
    uint32_t bands;
    uint32_t grid_blocks, block_threads;
    uint32_t kernel_vgprs, kernel_sgprs;   /* 0 if the runtime does not report them                */
} mi355rt_stats;

/* ---- one-shot call: host buffers in, host buffers out (what src/main.rs:57 would call) -------- */
int mi355rt_render(const mi355rt_scene* scene, const mi355rt_camera* camera,
                   const mi355rt_settings* settings, const mi355rt_options* options_or_null,
                   uint32_t* out_packed_rgb,       /* rows_rendered*width, 0x00RRGGBB              */
                   float*    out_linear_rgb_or_null,/* rows_rendered*width*3, pre-gamma mean       */
                   mi355rt_stats* stats_or_null);

/* ---- resident-scene API: upload once, render many times, device-side outputs ------------------ */
typedef struct mi355rt_context mi355rt_context;

int  mi355rt_context_create(int hip_device, mi355rt_context** out_ctx);
void mi355rt_context_destroy(mi355rt_context* ctx);
/* Uploads the scene (every array is copied: the caller's buffers may be freed afterwards) and picks the kernel for it.  BLOCKING, and it may
 * LAUNCH: for mesh-free scenes that mix a rough conductor with another scattering material a probe render of the same view (<= 64 pixels across,
 * <= 4 samples per pixel; deterministic, a fraction of a millisecond) runs on the NULL stream and is waited for -- its rays per path decide
 * between the lockstep and the wavefront kernel.  The probe stays out of the timing pool (mi355rt_context_set_timing).  Like every entry point
 * that looks at the context's error word, set_scene returns a pending watchdog failure of an EARLIER asynchronous render on this context
 * (MI355RT_ERR_HIP, once) instead of proceeding; call it again.                                                                          */
int  mi355rt_context_set_scene(mi355rt_context* ctx, const mi355rt_scene* scene,
                               const mi355rt_camera* camera, const mi355rt_settings* settings);
/* Number of rows the given options select (so callers can size their buffers).                  */
int  mi355rt_rows_selected(const mi355rt_settings* settings, const mi355rt_options* options_or_null,
                           uint32_t* out_rows);
/* Enqueue a render on `hip_stream` (a hipStream_t, or NULL for the default stream).  Outputs are
 * DEVICE pointers.  The call returns after the work is enqueued unless `stats_or_null` is given,
 * in which case it synchronises the stream to read the timers.                                   */
int  mi355rt_context_render(mi355rt_context* ctx, const mi355rt_options* options_or_null,
                            void* d_out_packed_rgb, void* d_out_linear_rgb_or_null,
                            void* hip_stream, mi355rt_stats* stats_or_null);

/* Frames in flight.  A render's path-tracing kernel is PERSISTENT: it launches as many workgroups as the device holds and each keeps claiming
 * samples until the frame is done -- so the end of every launch is a tail in which ever fewer paths keep the device busy, and a second frame
 * enqueued on another stream only trickles in as the first frame's workgroups retire.  For a large frame the tail is noise; for a small one -- the
 * eighth of an 800 x 600 image that one of 8 GPUs renders, src/renderer.rs:87-103 sharded by rows -- it is a third of the launch.  A caller that
 * renders a SEQUENCE of frames (an animation, progressive refinement, the bench) can hide it: keep F frames in flight, each on its own context
 * (own workspace) and its own stream, and tell every one of these contexts that it has 1 / share_of of the device: its kernels then launch that
 * fraction of the resident grid, F launches are co-resident, and a draining frame shares every SIMD with frames in their steady state.
 * share_of = 1 (the default) is the whole device; valid: 1 .. 16.  F > 4 streams buy nothing (HIP multiplexes streams onto 4 hardware queues by
 * default); F = 4 with share_of = 4 (mesh scenes with short walks: 2) measured best -- DESIGN.md section 7.  The image does not depend on it.
 * Takes effect with the next render on the context.                                                                                     */
int  mi355rt_context_set_share(mi355rt_context* ctx, uint32_t share_of);

/* Completion check of the asynchronous form.  render_scene is infallible (src/renderer.rs:67): it either returns the whole image or
 * panics.  mi355rt_context_render with stats == NULL only ENQUEUES work, so a failure inside a kernel -- a wave of the wavefront
 * kernel that gives up a bounded wait leaves paths unfinished -- cannot be returned by that call.  It is never lost: every render
 * leaves the context's error word behind in stream order, and the next of
 *   - mi355rt_context_check (waits for every render enqueued on this context so far),
 *   - mi355rt_context_read_timing,
 *   - the next mi355rt_context_render* on this context (without waiting: it sees the renders that have finished),
 *   - the same call, when it was given stats and therefore synchronises,
 * returns MI355RT_ERR_HIP once per failed render ("kernel watchdog ... that image is incomplete").  A caller that consumes images
 * from the asynchronous form calls mi355rt_context_check after synchronising its stream and before using them.                     */
int  mi355rt_context_check(mi355rt_context* ctx);

/* Progressive rendering (the sample loop of src/renderer.rs:93-101 cut into chunks): trace samples
 * [sample_begin, sample_end) of every selected pixel and add them, in sample order, to the running
 * sums in `d_accum` (DEVICE, 4 floats per selected pixel, row-major over the selected rows; read only
 * when sample_begin > 0, always written).  The outputs hold the image of the first `sample_end`
 * samples (sum * 1/sample_end, renderer.rs:103).  Because every draw is addressed by (row, x, sample,
 * ray) and the f32 additions happen in the same order, a sequence of calls covering 0..N is
 * bit-identical to one mi355rt_context_render with samples_per_pixel == N -- for any chunking.
 * settings.samples_per_pixel is not consulted.  MI355RT_RNG_CTR only.                              */
int  mi355rt_context_render_progressive(mi355rt_context* ctx, const mi355rt_options* options_or_null,
                                        uint32_t sample_begin, uint32_t sample_end, void* d_accum,
                                        void* d_out_packed_rgb, void* d_out_linear_rgb_or_null,
                                        void* hip_stream, mi355rt_stats* stats_or_null);

/* ---- ray queries: what does a ray hit in the resident scene? (added within ABI version 5: probe for the symbols) -------------------
 * The closest hit of HittableList::hit (src/hittable.rs:45-58) with t_min = EPSILON, t_max = INFINITY -- exactly what trace_ray asks
 * (src/renderer.rs:24) -- as the geometric HitRecord (hittable.rs:10-27) plus WHICH primitive won and its material INDEX: the caller owns
 * the material table and gets the hit position, so albedos and checker cells are looked up on its side.  For picking, visibility,
 * ambient-occlusion and lightmap baking, sensor simulation, and the normal / depth guides of a denoiser.  Bit for bit the reference's
 * arithmetic: the render kernels' own intersection code.
 *   - The calls only READ the resident scene: no workspace, no counters.  They may be enqueued on another stream while a render of the same
 *     context is in flight, do not consult mi355rt_context_set_share, and cannot fail inside a kernel (no bounded waits: the list is walked
 *     once, the stackless BVH walk follows child and escape links only, whatever the values are -- NaN and infinite rays included).
 *   - A pending watchdog failure of an EARLIER render on the context is returned the way mi355rt_context_render returns it.
 *   - Null context, no scene, a null or misaligned pointer (with n_rays > 0), a bad abi_version or row selection: MI355RT_ERR_INVALID, decided
 *     before any HIP call.  options.flags & MI355RT_FLAG_FIXED_AABB: MI355RT_ERR_UNSUPPORTED (the queries answer as the reference does).
 *     options.rng_mode, seed and workspace_bytes are ignored.
 *   - mi355rt_context_set_scene and mi355rt_context_destroy replace and free what a query reads: synchronise the streams that carry
 *     queries before calling them (a query leaves no event behind that they could wait on).
 *   - One device only: there is no mi355rt_multi_context_* form of the queries. */
typedef struct mi355rt_ray {       /* 32 bytes; arrays 16-byte aligned */
    float origin[3];    float _pad0;
    float direction[3]; float _pad1;   /* need not be unit: normalised ONCE, as Ray::new does (src/ray.rs:12-17, src/vec3.rs:37-44:
                                          a length below 1e-4 leaves it as it is).  Pads are ignored. */
} mi355rt_ray;

#define MI355RT_NO_HIT 0xFFFFFFFFu
typedef struct mi355rt_hit {       /* 48 bytes; HitRecord, src/hittable.rs:10-27 */
    float position[3];  float t;             /* t along the normalised direction */
    float normal[3];    uint32_t front_face; /* normal already flipped against the ray (set_face_normal); 0 / 1 */
    uint32_t primitive;                      /* index into mi355rt_scene.primitives; MI355RT_NO_HIT = miss */
    uint32_t material;                       /* that primitive's material index; MI355RT_NO_HIT on a miss */
    uint32_t _pad[2];                        /* written as 0 */
} mi355rt_hit;
/* A miss writes primitive = material = MI355RT_NO_HIT, t = +inf and every other word 0.  EVERY word of every record is written: the caller
 * never clears the buffer, and two results compare bytewise. */

/* n_rays arbitrary rays.  DEVICE pointers, 16-byte aligned; enqueues on hip_stream (NULL = default stream) and returns.
 * n_rays == 0 is a no-op that returns MI355RT_OK. */
int  mi355rt_context_trace_rays(mi355rt_context* ctx, const void* d_rays, uint32_t n_rays, void* d_hits, void* hip_stream);
/* (mi355rt_context_first_hits, below: the FIRST call with a row selection this context has not seen since set_scene allocates a small device
 * table for it -- hipMalloc, which may wait for the device -- and uploads it on hip_stream; later calls with that selection only enqueue.  A
 * context that has seen 16 different selections waits for the device once and starts over.) */
/* The same record for the ray through the CENTRE of every selected pixel: u = (x + 0.5) / width, v = (y + 0.5) / height, Camera::get_ray
 * (src/camera.rs:33-42) with the camera and settings of set_scene; rows selected by options exactly as mi355rt_context_render selects them
 * (mi355rt_rows_selected sizes the buffer); d_hits (DEVICE, 16-byte aligned) holds rows * width records, row-major over the selected rows. */
int  mi355rt_context_first_hits(mi355rt_context* ctx, const mi355rt_options* options_or_null, void* d_hits, void* hip_stream);
/* One-shot with HOST buffers (context on device 0, upload, query, copy back, destroy): what a host that owns no device memory calls.
 * It pays mi355rt_context_set_scene in full on every call -- the scene upload and, for the scenes named there, its probe render -- so a caller
 * with more than one batch of rays keeps a context and calls mi355rt_context_trace_rays. */
int  mi355rt_trace_rays(const mi355rt_scene* scene, const mi355rt_ray* rays, uint32_t n_rays, mi355rt_hit* out_hits);

/* ---- occlusion queries: does anything lie in front of t_max? (added within ABI version 5: probe for the symbols) --------------------------
 * For visibility and shadow tests and for ambient-occlusion and lightmap baking: one word out per ray instead of a 48-byte record, no record
 * is built, and the walk may stop early.
 *
 * DEFINITION.  Let h be the record mi355rt_context_trace_rays writes for the mi355rt_ray {origin, direction}.  Then
 *       out[i] = (h.primitive != MI355RT_NO_HIT && h.t < t_max) ? 1 : 0,
 * the comparison strict and in float32.  t_max is measured along the NORMALISED direction, the unit of mi355rt_hit.t.
 * CONSEQUENCES.  A NaN t_max gives 0.  A NaN h.t gives 0 (the reference's negated comparisons accept such "hits": a zero direction against
 * a sphere, an overflowing discriminant).  t_max = +inf asks for any hit with an ordered t.  t_max <= EPSILON (1e-4) gives 0: no hit is
 * accepted at or below t_min = EPSILON.  Every output word is written, nothing is written past word n - 1, n == 0 is a no-op.
 * THE WALK is the reference's (src/hittable.rs:45-58): closest_so_far starts at INFINITY and shrinks, whatever t_max is.  It does NOT start
 * at t_max: Mesh::hit hands closest_so_far to its BVH as an object-space bound (sic), so a smaller start would prune other triangles and
 * could change h.  Skipped is only this: once every ray of a wave holds an accepted candidate below its t_max, the rest of the LIST is not
 * walked -- exact, because a later candidate is only accepted at or below the current one, so the final t is below t_max as well.  That
 * argument needs every candidate's t to be ordered (after a NaN candidate the reference accepts anything).  The exit is therefore taken only
 * where no test can produce a NaN: every number the tests read from the scene and every component of the ray's origin within +-65536, the
 * normalised direction of a length in [1/2, 2] (any direction longer than 1e-4 that does not overflow).  Other rays, and every ray of other
 * scenes, walk the whole list.  Inside a mesh's tree nothing is skipped: Mesh::hit rejects the whole mesh when the FINAL triangle's
 * t_world lies below EPSILON, so a later, nearer triangle can turn a mesh that looked like a hit into a miss.
 * The calls follow the protocol of the ray queries above: they only read the resident scene, may run on another stream beside a render of the
 * same context, ignore mi355rt_context_set_share, cannot fail inside a kernel, and return a pending watchdog failure of an EARLIER render the
 * way mi355rt_context_render returns it.  Every refusal is decided before any HIP call and is MI355RT_ERR_INVALID with a text that names the
 * argument: a null context, no scene, a null or misaligned pointer (16 bytes for segments and hits, 4 for the outputs) when there is
 * something to do, a bad abi_version or row selection, params out of range.  options.flags & MI355RT_FLAG_FIXED_AABB: MI355RT_ERR_UNSUPPORTED.
 * One device only. */
typedef struct mi355rt_segment {   /* 32 bytes; arrays 16-byte aligned; the layout of mi355rt_ray with the last pad read */
    float origin[3];    float _pad0;     /* ignored */
    float direction[3]; float t_max;     /* direction as in mi355rt_ray; t_max along the NORMALISED direction */
} mi355rt_segment;
/* n segments, DEVICE pointers; enqueues on hip_stream (NULL = default stream) and returns. */
int  mi355rt_context_occluded(mi355rt_context* ctx, const void* d_segments, uint32_t n, void* d_out_u32, void* hip_stream);
/* One-shot with HOST buffers (context on device 0, upload, query, copy back, destroy); it pays mi355rt_context_set_scene on every call. */
int  mi355rt_occluded(const mi355rt_scene* scene, const mi355rt_segment* segments, uint32_t n, uint32_t* out);

/* Ambient occlusion at the first hits: `samples` occlusion queries per selected pixel, made and counted on the device.
 * d_hits is what mi355rt_context_first_hits wrote for the same row selection (rows selected, and their tables kept, exactly as that call does
 * it); d_out_f32 (DEVICE, 4-byte aligned) holds one float per selected pixel, row-major over the selected rows.
 *
 * DEFINITION.  All arithmetic is float32, one rounding per operation, in the order written (the library is built without contraction).
 * A pixel whose record is a miss (primitive == MI355RT_NO_HIT) gives 1.0f.  Otherwise, with P = hit.position, N = hit.normal, x the pixel's
 * column and y its ABSOLUTE image row, for sample s = 0 .. samples-1:
 *   Tries j = 0 .. 15:  w = pcg4d(x, y, s * 16 + j, seed)   (Jarzynski & Olano, JCGT 9(3) 2020: per word v = v * 1664525 + 1013904223; then
 *       x += y*w, y += z*x, z += x*y, w += y*z; every word ^= itself >> 16; the four multiply-adds again; all in uint32),
 *       c_k = (float)(w_k >> 8) * 2^-24 * 2 - 1 for k = 0, 1, 2 (every step exact: c_k = m * 2^-23 - 1 in [-1, 1)),
 *       l2 = (c0*c0 + c1*c1) + c2*c2.   The first try with l2 < 1.0f gives v = c; if none of the 16 qualifies, v = (0, 0, 0).
 *   Direction d = N + v, component by component.  The sample ray is the mi355rt_ray {P, d}: normalised once, as Ray::new does.
 *   The sample is OCCLUDED exactly when mi355rt_context_occluded answers 1 for the segment {P, d, radius}.  The origin sits on the surface;
 *   t_min = EPSILON is the only offset, as for the reference's bounce rays.
 *   out = 1.0f - (float)count / (float)samples, count the INTEGER number of occluded samples: however the lanes are dealt and the counts
 *   reduced, the result is the same bits. */
typedef struct mi355rt_ao_params {   /* 16 bytes */
    uint32_t samples;   /* 1, 2, 4, ... 256: a power of two */
    uint32_t seed;
    float    radius;    /* > 0 or +inf; NaN refused */
    uint32_t _pad;      /* must be 0 */
} mi355rt_ao_params;
/* params_or_null == NULL: {16, 0, +inf, 0} */
int  mi355rt_context_ambient_occlusion(mi355rt_context* ctx, const mi355rt_options* options_or_null, const mi355rt_ao_params* params_or_null,
                                       const void* d_hits, void* d_out_f32, void* hip_stream);

/* ---- radiance queries: whole paths along caller-supplied rays (added within ABI version 5: probe for the symbols) ----
 * The reference's trace_ray(ray, scene, depth, rng) (src/renderer.rs:19-65: hit, emit, scatter, recurse) for rays of the caller's own: a thin
 * lens, a fisheye, a panorama or an orthographic view, a light probe, a lightmap texel, a virtual sensor -- or the resident scene from a moved
 * camera without another mi355rt_context_set_scene.  The library has no camera model here: the caller makes the rays.
 *
 * DEFINITION.  Sample s of ray i is one path in MI355RT_RNG_CTR's addressing (mi355rt_options.rng_mode; the generator of ABI version 4):
 *   ykey = (uint64)row + params.seed;  k0 = low word, k1 = high word;  the path's draws are those of rng.start(k0, k1, x, s) -- what the render
 *   draws for sample s of the pixel in column x of image row `row`.  The path STANDS AT RAY 0.  The words of (ray 0, block 0) are NOT drawn by
 *   the query: they belong to whoever made the ray.  Words 0 / 1 are the render's pixel jitter; words 2 / 3 are free, for a lens sample for
 *   example.  The scatter event after ray r draws from ray r + 1, exactly as the render does.
 *   The direction is normalised once (Ray::new, src/ray.rs:12-17; a length below 1e-4 is left alone); scattered rays are used as the
 *   materials return them.  Every segment is HittableList::hit with t_min = EPSILON (the record of mi355rt_context_trace_rays).
 *   The radiance is folded front to back, as the GPU render folds it: throughput * terminal, where terminal is the emitted colour of a
 *   material that does not scatter, the miss colour of a ray that hits nothing (the sky texture's texel when the scene has one), or BLACK when
 *   max_depth segments were traced -- so inf * 0 is NaN, as documented at mi355rt_scene.  max_depth == 0: every sample is 1 * BLACK = +0.
 * CONSEQUENCE.  Given the render's own camera rays (camera.rs:33-42 with u = (x + word 0) / width, v = (row + word 1) / height, normalised
 *   once) and x = the pixel's column, row = its image row, the result is the render's linear image bit for bit.
 * SUMS.  d_accum holds n_rays float4 running sums (x, y, z; w is written 0).  It is READ only when sample_begin > 0 and is ALWAYS written.  The
 *   samples [sample_begin, sample_end) of a ray are added in sample order, in float32, continuing from the stored sum (renderer.rs:100).
 *   d_out_linear, if given, receives n_rays * 3 floats: sum * (1.0f / (float)sample_end) (renderer.rs:85,103).  Calls that cover 0 .. N in any
 *   chunking are bit-identical to one call [0, N).
 * SCRATCH is the caller's (the denoiser's pattern): mi355rt_radiance_scratch_bytes(n_rays, sample_end - sample_begin) bytes, 16-byte aligned --
 *   12 bytes per (ray, sample) pair, rounded up to a multiple of 16.  Its contents mean nothing between calls.
 * REFUSALS, all decided before any HIP call, MI355RT_ERR_INVALID with a text that names the argument: null params, flags != 0, reserved != 0,
 *   sample_begin >= sample_end; with n_rays > 0 a null or misaligned (16 bytes) d_rays / d_accum / d_scratch, a d_out_linear off 4 bytes, or
 *   n_rays * (sample_end - sample_begin) >= 2^32 (split the call); a null context, a context without a scene.  n_rays == 0 is MI355RT_OK and
 *   does nothing.  mi355rt_radiance_scratch_bytes refuses a null out_bytes and the same overflow.
 * PROTOCOL of the ray queries above: the call only reads the resident scene -- no workspace of the context, no counters, no error word --, may
 *   be enqueued beside a render of the same context on another stream, ignores mi355rt_context_set_share, and returns a pending watchdog failure
 *   of an EARLIER render the way mi355rt_context_render returns it.  Its work per sample is bounded by max_depth: it has no watchdog of its own.
 *   One device only.  MI355RT_FLAG_FIXED_AABB and the reference stream (MI355RT_RNG_REF) have no form here. */
typedef struct mi355rt_path_ray {     /* 32 bytes; arrays 16-byte aligned */
    float origin[3];    uint32_t x;   /* stream address word "x" (the render uses the pixel column) */
    float direction[3]; uint32_t row; /* stream key: row + params.seed, 64 bit (the render uses the image row y) */
} mi355rt_path_ray;
typedef struct mi355rt_radiance_params {  /* 32 bytes */
    uint32_t sample_begin, sample_end;    /* samples [begin, end) of EVERY ray; begin < end */
    uint32_t max_depth;                   /* renderer.rs:19-21; 0 = every sample is 1 * BLACK */
    uint32_t flags;                       /* must be 0 */
    uint64_t seed;                        /* as mi355rt_options.seed */
    uint64_t reserved;                    /* must be 0 */
} mi355rt_radiance_params;
int  mi355rt_radiance_scratch_bytes(uint32_t n_rays, uint32_t samples, uint64_t* out_bytes);
/* n_rays rays, DEVICE pointers; enqueues on hip_stream (NULL = default stream) and returns. */
int  mi355rt_context_trace_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params,
                                    const void* d_rays, uint32_t n_rays, void* d_accum, void* d_out_linear_or_null,
                                    void* d_scratch, void* hip_stream);
/* One-shot with HOST buffers (context on device 0, upload, query, copy back, destroy); it pays mi355rt_context_set_scene on every call.
 * accum_in_out (n_rays * 4 floats) must not be null: it is uploaded when sample_begin > 0 and always copied back.  Without a device:
 * MI355RT_ERR_NO_DEVICE (no CPU path), like mi355rt_trace_rays. */
int  mi355rt_trace_radiance(const mi355rt_scene* scene, const mi355rt_radiance_params* params,
                            const mi355rt_path_ray* rays, uint32_t n_rays, float* accum_in_out, float* out_linear_or_null);

/* ---- camera views: device-made rays for a pinhole and a thin lens (added within ABI version 5: probe for the symbols) ----
 * A VIEW is a camera the caller describes per call, for the resident scene: a moved camera or a depth-of-field lens without another
 * mi355rt_context_set_scene.  The rays are made on the device, in front of the path loop of the radiance queries above: no host-made rays, no
 * upload per sample, one call for any range of samples.  For every other camera model the caller still makes the rays (mi355rt_context_trace_radiance).
 *
 * DEFINITION.  The view has its own width x height image, independent of the scene's settings.  Pixel (x, y) is pixel y * width + x (row-major,
 *   row 0 = top) and carries the stream address x = x, row = y.  For sample s, w[0..3] are the words of (ray 0, block 0) of
 *   rng.start(ykey lo, ykey hi, x, s) with ykey = (uint64)y + seed -- MI355RT_RNG_CTR's addressing, as above --, and f(w) = (w >> 8) * 2^-24.
 *   All arithmetic is float32, one rounding per operation, in the order written, IEEE division and square root; normalized() is
 *   src/vec3.rs:37-44 (a length below 1e-4 is left alone); camera_raw(cam, u, v) = forward + (right * ((2u - 1) * half_width) +
 *   true_up * ((1 - 2v) * half_height)) (src/camera.rs:33-42).
 *   u, v:       u = ((float)x + f(w[0])) / (float)width,  v = ((float)y + f(w[1])) / (float)height   (src/renderer.rs:96-99).
 *               With MI355RT_VIEW_CENTRE both jitters are 0.5 and the lens point is (a, b) = (0, 0): the ray through the pixel centre, the ray of
 *               mi355rt_context_first_hits.  Fed to mi355rt_context_trace_rays it gives the first-hit records the denoiser needs for a view.
 *   PINHOLE:    origin = position;  direction = normalized(camera_raw(cam, u, v)).
 *   THIN LENS:  the lens point (a, b) comes from rejection in the unit disk: try j = 0, 1, ... takes a = 2 f(w2) - 1, b = 2 f(w3) - 1 from the words
 *               2 / 3 of (ray 0, block j) -- the render never draws the blocks >= 1 of ray 0 -- and is accepted on a*a + b*b < 1.  After 64 rejected
 *               tries (a, b) = (0, 0): the work per item is bounded.  off = right * (lens_radius * a) + true_up * (lens_radius * b);
 *               origin = position + off;  direction = normalized(camera_raw(cam, u, v) * focus_distance - off).
 *   mi355rt_context_view_rays writes these rays for one sample index: width * height mi355rt_path_ray records {origin, x, direction, row = y}.
 *   mi355rt_context_render_view IS, by definition, mi355rt_context_trace_radiance along the rays of view_rays(sample = s) for every s in
 *   [params.sample_begin, params.sample_end): the query normalises the direction once more (Ray::new -- the render's double normalisation), the
 *   same fold, the same sums in sample order continuing from d_accum (read only when sample_begin > 0, always written), the same
 *   d_out_linear = sum * (1.0f / (float)sample_end); calls that cover 0 .. N in any chunking give the words of one call.  d_out_packed, if given,
 *   receives width * height words 0x00RRGGBB of the mean, as the render packs a pixel (sqrt, clamp, * 255, truncate: src/color.rs:87-93).
 * CONSEQUENCE.  A pinhole view with the camera and the size of set_scene gives mi355rt_context_render's images (MI355RT_RNG_CTR, the same seed)
 *   bit for bit.
 * SCRATCH is the caller's: mi355rt_view_scratch_bytes(view, sample_end - sample_begin) bytes, 16-byte aligned -- 12 bytes per (pixel, sample),
 *   rounded up to a multiple of 16.
 * REFUSALS, all decided before any HIP call, MI355RT_ERR_INVALID with a text that names the argument: a null view, an unknown model, width or
 *   height 0, unknown flags, non-zero reserved words, a camera field that is not finite, a thin lens whose lens_radius is negative or not finite or
 *   whose focus_distance is not positive and finite, a non-zero lens field on a pinhole, width * height * samples >= 2^32 (split the
 *   call); a null or misaligned d_rays (16 bytes); everything mi355rt_context_trace_radiance refuses about its params and pointers (d_accum and
 *   d_scratch 16 bytes, d_out_linear and d_out_packed 4 bytes); a null context, a context without a scene.  There is no host-buffer form: a view
 *   is only worth having on a resident scene.
 * PROTOCOL of the ray queries: the calls read the resident scene only, touch no workspace of the context, only enqueue, and may run on another
 *   stream beside a render of the same context. */
#define MI355RT_VIEW_PINHOLE   0u
#define MI355RT_VIEW_THIN_LENS 1u
#define MI355RT_VIEW_CENTRE    1u     /* mi355rt_view.flags */
typedef struct mi355rt_view {          /* 96 bytes */
    mi355rt_camera camera;             /* exactly what mi355rt_context_set_scene takes */
    uint32_t model;                    /* MI355RT_VIEW_PINHOLE | _THIN_LENS */
    uint32_t width, height;            /* the view's own image size */
    uint32_t flags;                    /* MI355RT_VIEW_CENTRE or 0 */
    float    lens_radius;              /* thin lens: >= 0, finite; 0 otherwise */
    float    focus_distance;           /* thin lens: > 0, finite; 0 otherwise */
    uint32_t reserved[4];              /* must be 0 */
} mi355rt_view;
/* samples = sample_end - sample_begin of the render_view call */
int  mi355rt_view_scratch_bytes(const mi355rt_view* view, uint32_t samples, uint64_t* out_bytes);
/* DEVICE pointers; both enqueue on hip_stream (NULL = default stream) and return.  d_rays: width * height mi355rt_path_ray. */
int  mi355rt_context_view_rays(mi355rt_context* ctx, const mi355rt_view* view, uint32_t sample, uint64_t seed, void* d_rays, void* hip_stream);
/* d_accum: width * height float4; d_out_linear: width * height * 3 floats; d_out_packed: width * height uint32. */
int  mi355rt_context_render_view(mi355rt_context* ctx, const mi355rt_view* view, const mi355rt_radiance_params* params,
                                 void* d_accum, void* d_out_linear_or_null, void* d_out_packed_or_null, void* d_scratch, void* hip_stream);

/* ---- surface probes: device-made cosine-hemisphere rays for baking (added within ABI version 5: probe for the symbols) ----
 * A PROBE is a surface point and its normal: a lightmap texel, a diffuse light probe.  The call answers with the cosine-weighted mean of the
 * radiance arriving at each point -- the radiance form of mi355rt_context_ambient_occlusion.  The rays are made on the device, in front of the
 * path loop of the radiance queries above: no host-made rays, no upload per sample, one call for any range of samples -- baking takes hundreds
 * to thousands of samples per point.
 *
 * DEFINITION.  A probe record has the layout of mi355rt_path_ray; x and row are the stream address, as there.  The normal is USED AS GIVEN: a
 *   unit normal is the caller's business (mi355rt_hit.normal is one).  For sample s of probe i, with ykey = (uint64)row + seed and the generator
 *   of rng.start(ykey lo, ykey hi, x, s) standing at ray 0 -- MI355RT_RNG_CTR's addressing, as above.  All arithmetic is float32, one rounding
 *   per operation, in the order written, IEEE division and square root; normalized() is src/vec3.rs:37-44 (a length below 1e-4 is left alone).
 *   TRIES:      try j = 0, 1, ... takes p = (r(w1), r(w2), r(w3)) from the words 1 / 2 / 3 of (ray 0, block j), r(w) = (w >> 9) * 2^-22 - 1 (the
 *               bounce's mapping, random_range(-1.0..1.0); not the lens's f(w)).  The render draws words 0 / 1 of block 0 of ray 0 and never its
 *               blocks >= 1.  A try is accepted on (p.x*p.x + p.y*p.y) + p.z*p.z < 1.0f (src/vec3.rs:54-61).  After 64 rejected tries
 *               p = (0, 0, 0): the work per item is bounded.
 *   DIRECTION:  d = N + normalized(p); if every |component| of d is below 1e-8 (near_zero, src/vec3.rs:63-66) then d = N
 *               (src/material.rs:54-62).  direction = normalized(d): normalised once.
 *   ORIGIN:     P + N * EPSILON, EPSILON = 1e-4f (the reference's bounce origin).
 *   mi355rt_context_probe_rays writes these rays for one sample index: n mi355rt_path_ray records {origin, x, direction, row}.
 *   mi355rt_context_probe_radiance IS, by definition, mi355rt_context_trace_radiance along the rays of probe_rays(sample = s) for every s in
 *   [params.sample_begin, params.sample_end): the query normalises the direction once more (Ray::new), the same fold, the same sums in sample
 *   order continuing from d_accum (read only when sample_begin > 0, always written), the same d_out_linear = sum * (1.0f / (float)sample_end),
 *   the same mi355rt_radiance_params; calls that cover 0 .. N in any chunking give the words of one call.
 * CONSEQUENCE.  The probe ray is the bounce a white Lambert surface at (P, N) would make, if that event were addressed at ray 0.  With a unit
 *   normal the directions are cosine-weighted about N, so d_out_linear is the COSINE-WEIGHTED MEAN RADIANCE at the point: the irradiance is pi
 *   times it, and the radiosity of a diffuse texel its albedo times it.  The library does not multiply.
 * SCRATCH is the caller's: mi355rt_radiance_scratch_bytes(n, sample_end - sample_begin) bytes, 16-byte aligned.
 * REFUSALS, all decided before any HIP call, MI355RT_ERR_INVALID with a text that names the argument: everything
 *   mi355rt_context_trace_radiance refuses, under the call's own name, with d_probes in the place of d_rays; for probe_rays with n > 0 a null
 *   or misaligned (16 bytes) d_probes or d_rays, then a null context, a context without a scene.  n == 0 is MI355RT_OK and does nothing.  There
 *   is no host-buffer form: the probes come from first-hit records that are already on the device, and a one-shot would pay
 *   mi355rt_context_set_scene for every call -- a probe is only worth having on a resident scene.
 * PROTOCOL of the ray queries: the calls read the resident scene only, touch no workspace of the context, only enqueue, may run on another
 *   stream beside a render of the same context, and run on one device. */
typedef struct mi355rt_probe {        /* 32 bytes; arrays 16-byte aligned */
    float position[3]; uint32_t x;    /* stream address word "x", as mi355rt_path_ray.x */
    float normal[3];   uint32_t row;  /* stream key: row + seed, 64 bit, as mi355rt_path_ray.row */
} mi355rt_probe;
/* DEVICE pointers; both enqueue on hip_stream (NULL = default stream) and return.  d_probes: n mi355rt_probe; d_rays: n mi355rt_path_ray. */
int  mi355rt_context_probe_rays(mi355rt_context* ctx, const void* d_probes, uint32_t n, uint32_t sample, uint64_t seed, void* d_rays, void* hip_stream);
/* d_accum: n float4; d_out_linear: n * 3 floats; d_scratch: mi355rt_radiance_scratch_bytes(n, sample_end - sample_begin) bytes. */
int  mi355rt_context_probe_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params, const void* d_probes, uint32_t n,
                                    void* d_accum, void* d_out_linear_or_null, void* d_scratch, void* hip_stream);

/* ---- denoising a preview: an edge-avoiding a-trous filter guided by first-hit records (added within ABI version 5: probe for the symbols) ----
 * For the first chunks of a progressive render: the noisy linear image and the records of mi355rt_context_first_hits for the same rows go in,
 * a filtered linear and / or packed image comes out.  Not part of the reference; an independent restatement of the definition below in
 * float32 is bit-identical to the kernels (the library is built without FMA contraction).
 *
 * WINDOW.  `rows` is a CONTIGUOUS window of the image, `width` pixels wide: the filter has no meaning across the gaps of an interleaved strip
 * selection.  Pass what mi355rt_rows_selected reports for {row_begin, row_end} with n_parts <= 1, and the buffers of that selection.
 *
 * THE FILTER.  All arithmetic is float32, one rounding per operation, in the order written, IEEE division.  c is the colour image of the
 * previous level (level 0: the input), g the guide record of a pixel; a pixel is a MISS when g.primitive == MI355RT_NO_HIT.
 *   Per level k = 0 .. levels-1: step s = 1 << k, sigma_k = sigma_color * 2^-k, a_k = 1.0f / (sigma_k * sigma_k)   (computed on the host, f32).
 *   Taps of pixel p = (x, y), y local to the window: dy = -2 .. 2 (outer loop), dx = -2 .. 2 (inner loop); q = (x + dx*s, y + dy*s); a tap
 *   outside [0, width) x [0, rows) is skipped.  h = K[|dy|] * K[|dx|], K = {3/8, 1/4, 1/16}.
 *   Geometry weight G:  p a miss: G = 1 if q is a miss, else 0.   p a hit, q a miss: G = 0.   Otherwise
 *       nd = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;   wn = nd > 0 ? nd : 0, then wn = wn*wn repeated normal_squarings times;
 *       D = P_q - P_p;   d = |(n_p.x*D.x + n_p.y*D.y) + n_p.z*D.z|;   e = 1 - d / (sigma_plane * t_p);   wp = e > 0 ? e : 0;   G = wn * wp.
 *   Colour weight:  dc = c_q - c_p;   d2 = (dc.r*dc.r + dc.g*dc.g) + dc.b*dc.b;   wc = 1 / (1 + d2 * a_k).
 *   Accumulation:  w = (h * G) * wc.  A tap with !(w > 0) is SKIPPED, nothing is added.  Otherwise acc.ch += c_q.ch * w (r, g, b), ws += w.
 *   Result of the level:  ws > 0 ? acc.ch / ws : c_p.ch   (one division per channel).
 *   d_out_linear receives the last level's image, d_out_packed color_to_u32(sqrt(.)) of it -- the packing of every render call (NaN and negative
 *   channels pack as 0, +inf as 255).  levels == 0 copies the input to the output (and packs it).
 * CONSEQUENCES.  A NaN or infinite pixel passes through unchanged and contaminates no neighbour (its taps have a NaN or zero weight): as in
 * mi355rt_scene, non-finite values propagate and nothing is validated.  NaN guides (t = NaN "hits", NaN normals) drop their taps.  A firefly
 * keeps itself (its colour weight towards everything else is small): a luminance clamp is not part of this call.  sigma_color halves per level
 * (the published rule), so levels past the third or fourth change little.
 *
 * THE CALL.  The context supplies the device only -- no scene is needed, nothing is allocated, no state is kept in the context: the call
 * enqueues its kernels on hip_stream and returns.  It may run beside a render or a query of the same context on another stream, and cannot
 * fail inside a kernel (no waits, no atomics, bounded loops).  A pending watchdog failure of an EARLIER render on the context is returned the
 * way the ray queries return it.  Every argument check comes before any HIP call and returns MI355RT_ERR_INVALID with a text that names the
 * argument: a null context, input, hits or scratch; both outputs null; d_hits or d_scratch not 16-byte aligned, a float or packed buffer not
 * 4-byte aligned; width or rows 0, width * rows >= 2^31; params out of range or not finite.
 * d_out_linear MAY ALIAS d_linear_in: the first kernel copies the input into the scratch and nothing reads it afterwards.  Every word of every
 * output record is written; nothing is written past the end of an output or of the scratch.  What the scratch holds afterwards is unspecified.
 * One device only: the assembled image of a mi355rt_multi_context lives on hip_devices[0]; keep one mi355rt_context there for first_hits + denoise. */
typedef struct mi355rt_denoise_params {   /* 16 bytes */
    uint32_t levels;            /* a-trous passes, step 1, 2, 4, ...; 0 .. 8; 0 = copy (and pack) */
    uint32_t normal_squarings;  /* normal weight = max(0, n_p . n_q) squared this many times; 0 .. 8 */
    float    sigma_color;       /* > 0, finite; halved per level */
    float    sigma_plane;       /* > 0, finite; plane distance relative to the centre's t */
} mi355rt_denoise_params;
/* params_or_null == NULL: {5, 5, 2.0f, 0.05f} */

/* Bytes of d_scratch for a window of rows x width pixels (the layout is the library's own). */
int  mi355rt_denoise_scratch_bytes(uint32_t width, uint32_t rows, uint64_t* out_bytes);
/* DEVICE pointers: d_linear_in rows*width*3 floats in the layout of d_out_linear_rgb; d_hits rows*width mi355rt_hit, what
 * mi355rt_context_first_hits wrote for the same window; d_scratch mi355rt_denoise_scratch_bytes; at least one of the outputs. */
int  mi355rt_context_denoise(mi355rt_context* ctx, uint32_t width, uint32_t rows, const mi355rt_denoise_params* params_or_null,
                             const void* d_linear_in, const void* d_hits, void* d_scratch,
                             void* d_out_linear_or_null, void* d_out_packed_or_null, void* hip_stream);
/* One-shot with HOST buffers on device 0 (upload, filter, copy back): what a host that owns no device memory calls. */
int  mi355rt_denoise(uint32_t width, uint32_t rows, const mi355rt_denoise_params* params_or_null,
                     const float* linear_in, const mi355rt_hit* hits, float* out_linear_or_null, uint32_t* out_packed_or_null);

/* mi355rt_render over several GPUs from ONE host process (the reference's host is a single `main`):
 * row strips of options.strip_rows rows (0 -> 4) are dealt round-robin over `hip_devices`, each device
 * renders its strips with the full scene resident and copies them into the caller's image; no
 * collective is involved.  options.n_parts / part must be left 0 (row_begin / row_end still select a
 * window, and the outputs then hold only that window).  Bit-identical to the one-device image.  A
 * device may be listed more than once (testing on a one-GPU machine).                                */
int  mi355rt_render_multi(const mi355rt_scene* scene, const mi355rt_camera* camera,
                          const mi355rt_settings* settings, const mi355rt_options* options_or_null,
                          const int* hip_devices, uint32_t n_devices,
                          uint32_t* out_packed_rgb, float* out_linear_rgb_or_null, mi355rt_stats* stats_or_null);

/* ---- resident multi-device form: one process, several GPUs, scene and buffers kept across calls ----------------------------
 * What mi355rt_render_multi does in one call, split into a context that stays: every entry of `hip_devices` is one PART with its own
 * mi355rt_context, a non-blocking stream, a staging buffer for its rows and a done-event; hip_devices[0] is the DESTINATION device, on
 * which both outputs live.  A device may be listed more than once (each entry is still its own part: how a one-GPU machine tests this).
 * Strips of options.strip_rows rows (0 -> 4) are dealt round-robin over the parts; options.n_parts / part must be left 0 (or n_parts 1);
 * row_begin / row_end select a window (the outputs then hold only those rows); rng_mode, seed, flags and workspace_bytes pass through to
 * every part.  The image is bit-identical, packed and linear, to mi355rt_context_render of the same window on one device.
 * Every entry point leaves the calling thread's current HIP device as it found it.                                                  */
typedef struct mi355rt_multi_context mi355rt_multi_context;

int  mi355rt_multi_context_create(const int* hip_devices, uint32_t n_devices, mi355rt_multi_context** out);
/* Waits for every render enqueued on the context, then frees it.  Peer access enabled by create stays enabled (process-wide state). */
void mi355rt_multi_context_destroy(mi355rt_multi_context* m);
/* BLOCKING: uploads the scene to every part at once (one host thread per part; a part whose thread cannot be started is uploaded on the
 * calling thread).  May be called again to change scene, camera or settings.                                                         */
int  mi355rt_multi_context_set_scene(mi355rt_multi_context* m, const mi355rt_scene* scene,
                                     const mi355rt_camera* camera, const mi355rt_settings* settings);
/* Outputs are DEVICE pointers on hip_devices[0]; `hip_stream` is a hipStream_t of hip_devices[0] or NULL (its default stream).  Every part
 * renders its strips on its own stream after the work already enqueued on `hip_stream`; the strips come back with one peer copy per part and
 * output (copy engines, no CU slots) and one k_gather_strips launch puts every row in its place, all on `hip_stream`, which therefore orders
 * the result.  With stats == NULL the call only enqueues.  With stats it waits, and fills: render / resolve kernel ms = the largest over the
 * parts (HIP events of each part's own timeline), samples / rays / rows_rendered / bands = sums, total_ms = host wall time from entry to the
 * end of the assembly (devices share no event timeline); grid_blocks, block_threads, kernel_vgprs, kernel_sgprs are 0.               */
int  mi355rt_multi_context_render(mi355rt_multi_context* m, const mi355rt_options* options_or_null,
                                  void* d_out_packed_rgb, void* d_out_linear_rgb_or_null,
                                  void* hip_stream, mi355rt_stats* stats_or_null);
/* Waits for every render enqueued so far and returns the first pending watchdog failure of a part (mi355rt_context_check), once, with
 * the device named.  Every other multi-context call that finds such a failure pending returns it the same way.                      */
int  mi355rt_multi_context_check(mi355rt_multi_context* m);

/* Progressive rendering on the resident multi-device context (added within ABI version 5: probe for the symbol): what
 * mi355rt_context_render_progressive is on one device.  Samples [sample_begin, sample_end) of every selected pixel are traced and added,
 * in sample order, to running sums; the outputs (DEVICE pointers on hip_devices[0], the selected rows, as in mi355rt_multi_context_render)
 * hold the image of the first `sample_end` samples, packed, and linear when asked for.  Bit-identical to mi355rt_context_render_progressive
 * fed the same chunks on one device, and so to mi355rt_context_render at samples_per_pixel = the sum (settings.samples_per_pixel is not
 * consulted).
 *   - Where the sums live: every PART owns them -- a float4 per pixel of its own strips, on its own device, allocated on first use and only
 *     grown.  They never cross a device link between chunks, and they are separate from the workspaces: a plain
 *     mi355rt_multi_context_render between two chunks leaves the sequence intact.
 *   - A SEQUENCE starts with sample_begin == 0.  sample_begin > 0 continues it and must equal the sample_end of the last progressive call on
 *     this context, with the same row selection (row_begin, row_end, strip_rows), rng_mode, seed and flags; any other call returns
 *     MI355RT_ERR_INVALID saying why.  A call refused by these checks or by its argument checks changes nothing.
 *   - What ends a sequence (the only valid next call then starts at 0): mi355rt_multi_context_set_scene; a progressive call that fails after
 *     its checks, a pending part watchdog failure that it reports included; a mi355rt_multi_context_check that reports a failure; a
 *     mi355rt_multi_context_render that returns MI355RT_ERR_HIP (the failure it reports may be an earlier chunk's).
 *   - d_accum_or_null (on hip_devices[0]; WRITTEN, never read): when given, it receives the gathered sums of the selected rows in the layout
 *     of mi355rt_context_render_progressive's d_accum (4 floats per pixel, row-major), bit-identical to what that call leaves there after the
 *     same chunks -- to checkpoint them or to hand them to a single-device context.
 *   - Stream protocol: that of mi355rt_multi_context_render.  Every part runs mi355rt_context_render_progressive on its own stream into its
 *     own sums; the sums, when asked for, go peer-to-peer straight from every part's sums to a staging area on hip_devices[0] (one more peer
 *     copy per part) and one k_gather_accum launch puts their rows in place.  Without stats the call only enqueues; with stats it waits once
 *     and fills the fields of mi355rt_multi_context_render (samples = rows * width * (sample_end - sample_begin)).
 *   - MI355RT_RNG_CTR only (MI355RT_RNG_REF -> MI355RT_ERR_INVALID); options.n_parts / part must be left 0.  Every entry point leaves the
 *     calling thread's current HIP device as it found it.                                                                                */
int  mi355rt_multi_context_render_progressive(mi355rt_multi_context* m, const mi355rt_options* options_or_null,
                                              uint32_t sample_begin, uint32_t sample_end,
                                              void* d_accum_or_null,
                                              void* d_out_packed_rgb, void* d_out_linear_rgb_or_null,
                                              void* hip_stream, mi355rt_stats* stats_or_null);

/* One-shot progressive render with HOST buffers: mi355rt_render in chunks of `chunk_spp` samples.  After
 * every chunk `on_chunk_or_null(user, samples_done, samples_total, out_packed_rgb)` sees the image so far
 * (what the reference's preview window, src/main.rs:60-75, would show); a non-zero return stops early and
 * leaves the image of `samples_done` samples in the outputs.  The final image equals mi355rt_render's.   */
typedef int (*mi355rt_progress_fn)(void* user, uint32_t samples_done, uint32_t samples_total, const uint32_t* packed_rgb);
int  mi355rt_render_progressive(const mi355rt_scene* scene, const mi355rt_camera* camera,
                                const mi355rt_settings* settings, const mi355rt_options* options_or_null,
                                uint32_t chunk_spp, mi355rt_progress_fn on_chunk_or_null, void* user,
                                uint32_t* out_packed_rgb, float* out_linear_rgb_or_null, mi355rt_stats* stats_or_null);
/* Its multi-device twin (added within ABI version 5: probe for the symbol), built on mi355rt_multi_context_render_progressive: strips dealt
 * over `hip_devices` as in mi355rt_render_multi (options.n_parts / part left 0), chunks of `chunk_spp` samples, the last one possibly
 * shorter.  After every chunk the packed image comes back to out_packed_rgb and on_chunk_or_null sees it; a non-zero return stops early
 * and leaves the image of `samples_done` samples in the outputs.  The final image equals mi355rt_render's and mi355rt_render_multi's.
 * stats: kernel ms summed over the chunks, samples / rays summed, rows_rendered of one chunk.                                          */
int  mi355rt_render_progressive_multi(const mi355rt_scene* scene, const mi355rt_camera* camera,
                                      const mi355rt_settings* settings, const mi355rt_options* options_or_null,
                                      const int* hip_devices, uint32_t n_devices,
                                      uint32_t chunk_spp, mi355rt_progress_fn on_chunk_or_null, void* user,
                                      uint32_t* out_packed_rgb, float* out_linear_rgb_or_null, mi355rt_stats* stats_or_null);

/* Kernel timing without extra synchronisation: while enabled, every mi355rt_context_render call that
 * passes stats == NULL records HIP events around its kernels on the caller's stream.  After the
 * caller has synchronised that stream, read_timing returns the summed kernel durations and the
 * number of (path tracing + resolve) launch pairs since the last read, and resets the pool.        */
int  mi355rt_context_set_timing(mi355rt_context* ctx, int enable);
int  mi355rt_context_read_timing(mi355rt_context* ctx, double* render_kernel_ms, double* resolve_kernel_ms,
                                 uint32_t* launches);

const char* mi355rt_last_error(void);
uint32_t    mi355rt_abi_version(void);

/* =================================================================================================
 * Host-side helpers (libmi355rt_host.so, pure CPU).  They stand in for the parts of the Rust host
 * that cannot be built here: the producers of the arrays above.
 * ================================================================================================= */

/* BVHNode::new (src/acceleration/bvh.rs:15-76) over object-space triangles: median split on the
 * largest-extent axis, leaf when <= 4 triangles or depth >= 25.  The centroid sort restates Rust's
 * slice::sort_unstable_by (ipnsort, Rust 1.81+) including its order of equal keys, so the arrays are the tree
 * the reference's own BVHNode::new builds (csrc/host/rust_sort_unstable.hpp).
 * Two-call pattern: pass NULL arrays to get the counts.                                           */
int mi355rt_bvh_build(const mi355rt_triangle* triangles, uint32_t n_triangles,
                      mi355rt_bvh_node* out_nodes, uint32_t* inout_n_nodes,
                      uint32_t* out_indices, uint32_t* inout_n_indices,
                      uint32_t* out_max_depth);

/* load_scene_from_json (src/tungsten/parser.rs:245-815) + Camera::new (src/camera.rs:14-31) +
 * Mesh::from_obj / from_wo3 (src/mesh/mesh_object.rs:59-259).  Overrides replace the values parsed
 * at parser.rs:260-285 (0 = keep the file's value).                                               */
typedef struct mi355rt_loaded_scene mi355rt_loaded_scene;

typedef struct mi355rt_load_overrides {
    uint32_t width, height, samples_per_pixel, max_depth;
    uint32_t skip_unknown_primitives;  /* 0 = hard error like serde (parser.rs:135-165), 1 = skip   */
    uint32_t wo3_four_index_stride;    /* 0 = the reference's reader, which steps 3 u32 per triangle through a file that stores 4
                                        *     (mesh_object.rs:190-192: ~1/4 of the triangles survive);
                                        * 1 = opt-in fix: read (v0, v1, v2, material) per triangle.  Changes the image.               */
} mi355rt_load_overrides;

int  mi355rt_scene_load_json(const char* json_path, const mi355rt_load_overrides* overrides_or_null,
                             mi355rt_loaded_scene** out_scene);
void mi355rt_scene_free(mi355rt_loaded_scene* s);
const mi355rt_scene*    mi355rt_loaded_scene_get(const mi355rt_loaded_scene* s);
const mi355rt_camera*   mi355rt_loaded_scene_camera(const mi355rt_loaded_scene* s);
const mi355rt_settings* mi355rt_loaded_scene_settings(const mi355rt_loaded_scene* s);

/* save_image's pixel conversion (src/renderer.rs:125-143) into an 8-bit RGB PNG.                  */
int mi355rt_write_png(const char* path, const uint32_t* packed_rgb, uint32_t width, uint32_t height);

/* The pre-gamma f32 image (out_linear_rgb) as a little-endian Portable FloatMap, for parity tooling.  */
int mi355rt_write_pfm(const char* path, const float* linear_rgb, uint32_t width, uint32_t height);
/* The same image as an OpenEXR file: scan-line, three 32-bit FLOAT channels (B, G, R), uncompressed, rows top-down. */
int mi355rt_write_exr(const char* path, const float* linear_rgb, uint32_t width, uint32_t height);

/* ---- noise estimate of a progressive render: is this image good enough yet? (added within ABI version 5: probe for the symbols) ------------
 * For the caller of mi355rt_context_render_progressive that does not want to guess samples_per_pixel: after every chunk it hands a HOST copy
 * of the running sums (d_accum) to mi355rt_noise_update, and mi355rt_noise_evaluate answers with a per-pixel relative standard error of the
 * mean luminance and a verdict.  Pure CPU; not part of the reference (src/main.rs renders the file's spp and stops).
 *
 * DEFINITION.  All arithmetic is IEEE double, one rounding per operation, in the order written (the library is built without contraction).
 * State per pixel p: prev[3] (float, the last running sums, 0 at the start), T (the sum of Y) and Q (the sum of Y*Y/n), both 0 at the start.
 * Global state: K chunks and N samples, both 0 at the start.
 *   update(accum, samples_total), which needs samples_total > N:   n = samples_total - N;   for c = r, g, b:
 *       d_c = (double)accum[4p+c] - (double)prev[c];   Y = (0.2126*d_r + 0.7152*d_g) + 0.0722*d_b;
 *       T += Y;   Q += (Y*Y)/(double)n;   prev = accum;   then K += 1, N = samples_total.   Chunks may differ in size.  accum[4p+3] is not read.
 *   evaluate, which needs K >= 2:   m = T/N;   ss = Q - (T*T)/N;   var = (ss > 0 ? ss : 0)/(K-1);   se = sqrt(var/N);
 *       err = se/((m > 0 ? m : 0) + floor).
 *       A pixel whose T or Q is not finite has err = NaN; so has a pixel whose division is 0/0 (floor = 0 and neither signal nor variance).
 *       Such a pixel is counted in `nonfinite`, never in `above`, and is left out of max_error and mean_error.
 *       above = the number of pixels with err > threshold (an err of +inf counts).   max_error = the largest err, 0 when no pixel is counted.
 *       mean_error = (the sum of err in pixel order) / (pixels - nonfinite), 0 when no pixel is counted.   out_error[p] = (float)err, a NaN as 0x7FC00000.
 *       converged = (K >= min_chunks && above <= allowed_above).
 * WHY.  This is the weighted batch-means estimator: the samples of the counter-mode stream are independent, a chunk of n_k samples has the
 * mean m_k = Y_k/n_k, and the expectation of  sum over k of n_k*(m_k - m)^2  =  Q - T*T/N  is (K-1)*sigma^2, sigma^2 the variance of one
 * sample's luminance.  So se estimates the standard error of the pixel's mean luminance after N samples, err the same relative to that mean;
 * `floor` keeps dark pixels from asking for ever more samples.
 * WHAT IT DOES NOT DO.  A firefly that no chunk has seen yet is not estimated: a pixel can look converged until its first rare bright path
 * arrives.  A small K gives a noisy estimate (the relative deviation of se is about 1/sqrt(2(K-1))): min_chunks guards the verdict, not the map.
 * Non-finite pixels (an infinite emitter, a NaN path: mi355rt_scene) are reported in `nonfinite` and do NOT block convergence -- more samples
 * never make them finite.  It estimates luminance only, over the image before gamma and packing; it knows nothing of a denoiser applied later.
 * REFUSALS are MI355RT_ERR_INVALID with a text (mi355rt_host_last_error) that names the argument: a null state, out, accum or out_summary;
 * width or rows 0, width * rows >= 2^31; samples_total not above the samples already seen; evaluate before the second update; threshold not
 * > 0 or not finite, floor negative or not finite, min_chunks < 2, _pad not 0.  A failed allocation is MI355RT_ERR_OOM.  A refused call
 * changes nothing.  A state is not thread-safe; different states are independent. */
typedef struct mi355rt_noise_state mi355rt_noise_state;
typedef struct mi355rt_noise_params {   /* 32 bytes */
    double   threshold;      /* > 0, finite: a pixel is `above` when err > threshold */
    double   floor;          /* >= 0, finite: added to the mean luminance in the denominator */
    uint32_t min_chunks;     /* >= 2: no verdict of `converged` before this many chunks */
    uint32_t _pad;           /* must be 0 */
    uint64_t allowed_above;  /* converged while at most this many pixels are above */
} mi355rt_noise_params;
/* params_or_null == NULL: {0.02, 0.01, 4, 0, 0} */

typedef struct mi355rt_noise_summary {  /* 56 bytes */
    uint32_t chunks, samples;           /* K, N */
    uint64_t pixels, above, nonfinite;
    double   max_error, mean_error;
    uint32_t converged, _pad;           /* 0 / 1; _pad written as 0 */
} mi355rt_noise_summary;

int  mi355rt_noise_create(uint32_t width, uint32_t rows, mi355rt_noise_state** out);
void mi355rt_noise_free(mi355rt_noise_state* state);
/* Back to K = N = 0 and zero sums: the next update starts a new sequence (after a camera or scene change). */
int  mi355rt_noise_reset(mi355rt_noise_state* state);
/* accum: rows*width*4 floats, a host copy of d_accum after the chunk that ended at sample_end = samples_total. */
int  mi355rt_noise_update(mi355rt_noise_state* state, const float* accum, uint32_t samples_total);
/* out_error_or_null: rows*width floats.  Reads the state only: it may be called after any update, with any params. */
int  mi355rt_noise_evaluate(const mi355rt_noise_state* state, const mi355rt_noise_params* params_or_null,
                            float* out_error_or_null, mi355rt_noise_summary* out_summary);

const char* mi355rt_host_last_error(void);

/* ---- the same estimate on the device, beside the running sums (libmi355rt.so; added within ABI version 5: probe for the symbols) -------------
 * mi355rt_noise_update / mi355rt_noise_evaluate above want a HOST copy of d_accum after every chunk; these read d_accum where it is -- the buffer of
 * mi355rt_context_render_progressive, or what mi355rt_multi_context_render_progressive leaves in d_accum_or_null -- and leave the verdict as the
 * 56 bytes of a mi355rt_noise_summary in stream order.  The object stands alone: a device number and its buffers (48 bytes per pixel and 32 per
 * tile), no mi355rt_context.  reset, update and evaluate only ENQUEUE on hip_stream and return; K and N are kept on the host side of the object
 * at enqueue time, so every refusal is decided before any HIP call.  The calls make the object's device current, as mi355rt_context_* do.  One
 * object's calls belong on one stream at a time (evaluate's per-tile records are the object's); the caller synchronises the streams that carry
 * its work before destroy.  An object is not thread-safe; different objects are independent.
 *
 * DEFINITION.  update and evaluate are the DEFINITION above, operation for operation in IEEE double with one rounding each (divisions and the
 * square root correctly rounded), with the same NaN rules: the error map, chunks, samples, pixels, above, nonfinite, max_error, converged and
 * _pad are bit for bit what mi355rt_noise_evaluate gives for the same sums.  accum[4p+3] is not read.  mean_error alone is summed in another
 * ORDER -- a fixed tree instead of the host's sum in pixel order -- so it differs from the host's by rounding only: all terms are >= 0, so both
 * sums are within (pixels + 64) * 2^-53, relative, of each other.  The order depends on the pixel count alone: not on a grid size, not on the
 * device, not on timing (no floating-point atomics).
 *   e[p] = err of pixel p, and +0.0 where the pixel is not counted (nonfinite) and for p >= pixels; pixels = width * rows.
 *   TILES.   The list is cut into tiles of 256 consecutive pixels: tile j holds the pixels 256 j .. 256 j + 255, n_tiles = ceil(pixels / 256).
 *   TREE(v), v[0 .. 255]:   each run of 64 (a wave: v[64 w .. 64 w + 63], w = 0 .. 3) is halved six times -- x[i] = x[i] + x[i + h] for
 *       i < h, with h = 32, 16, 8, 4, 2, 1 -- which leaves the wave's sum s_w in x[0];   TREE = (s_0 + s_1) + (s_2 + s_3).
 *   S_j = TREE(e[256 j .. 256 j + 255]) for every tile j.
 *   ACROSS TILES.   a[t] = ((S_t + S_(t + 256)) + S_(t + 512)) + ... for t = 0 .. 255: tile sums 256 apart, added in ascending order,
 *       0.0 where there is no tile t.   sum = TREE(a).
 *   mean_error = sum / (double)(pixels - nonfinite), 0 when no pixel is counted.
 *   max_error and the counts go the same way; a maximum and an integer sum do not depend on the order.
 * evaluate writes every one of the 56 bytes of *d_out_summary, _pad as 0, and rows * width floats to d_out_error when that is given: nothing else.
 * d_accum: rows * width * 4 floats, 16-byte aligned.  d_out_summary: any 8-byte aligned memory the device can write -- hipMalloc'ed, or
 * pinned host memory (then the caller reads it after an event recorded behind evaluate).  d_out_error_or_null: rows * width floats, 4-byte aligned.
 * REFUSALS are MI355RT_ERR_INVALID with a text (mi355rt_last_error) that names the argument, the host's texts with the prefix noise_device_:
 * a null state, out, d_accum or d_out_summary; a d_accum that is not 16-byte aligned, a d_out_summary not 8-byte, a d_out_error not 4-byte
 * aligned; width or rows 0, width * rows >= 2^31; samples_total not above the samples already seen; evaluate before the second update;
 * threshold not > 0 or not finite, floor negative or not finite, min_chunks < 2, _pad not 0.  No device is MI355RT_ERR_NO_DEVICE, a failed
 * allocation MI355RT_ERR_OOM.  A refused call changes nothing; a call that returns an error has not advanced K or N.  After MI355RT_ERR_HIP the
 * contents are unspecified until reset. */
typedef struct mi355rt_noise_device mi355rt_noise_device;
int  mi355rt_noise_device_create(int hip_device, uint32_t width, uint32_t rows, mi355rt_noise_device** out);
void mi355rt_noise_device_destroy(mi355rt_noise_device* s);
/* Back to K = N = 0 and zero sums, in stream order. */
int  mi355rt_noise_device_reset(mi355rt_noise_device* s, void* hip_stream);
/* d_accum after the chunk that ended at sample_end = samples_total; it is read in stream order, so enqueue it behind the render on the same stream. */
int  mi355rt_noise_device_update(mi355rt_noise_device* s, const void* d_accum, uint32_t samples_total, void* hip_stream);
int  mi355rt_noise_device_evaluate(mi355rt_noise_device* s, const mi355rt_noise_params* params_or_null,
                                   void* d_out_error_or_null, void* d_out_summary, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355RT_H */
