/*
 * mi355rt.h — C ABI of libmi355rt.so, the MI355X (gfx950) render path behind
 * raytracer-rs's `raytracer_lib` API.
 *
 * Every entry point names the reference interface it replaces (paths relative to
 * /root/reference/raytracer_lib/src).  Conventions:
 *   - plain pointers and sizes only; the caller owns every input pointer, the library copies
 *     during `create`; output buffers are caller-allocated;
 *   - functions return 0 on success or a negative MI355RT_E_* code, and
 *     mi355rt_last_error() then returns the message the reference would carry in its
 *     `Result<_, String>` (lib.rs:15-27);
 *   - a handle may be created on one thread and used on another (main.rs:183,194-196): every
 *     entry binds the handle's HIP device; calls on ONE handle must not overlap;
 *   - there is NO CPU fallback: without a usable HIP device `create` fails with
 *     MI355RT_E_NO_DEVICE.
 */
#ifndef MI355RT_H
#define MI355RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355RT_OK            0
#define MI355RT_E_INVALID    -1   /* bad argument */
#define MI355RT_E_NO_DEVICE  -2   /* no HIP device / HIP runtime error */
#define MI355RT_E_LOAD       -3   /* scene load error (SceneLoadError, loaders/mod.rs:20-25); film file error (mi355rt_film_load / _save / _file_info) */
#define MI355RT_E_HIP        -4   /* HIP runtime error after creation */

/* DEFAULT_TRIANGLES_PER_LEAF, oct_tree_intersector.rs:12 / lib.rs:7 */
#define MI355RT_DEFAULT_TRIANGLES_PER_LEAF 70u
/* rows per stripe of the deal over ranks / devices / frame slices when config.stripe_rows is 0 (and what mi355rt_default_config sets) */
#define MI355RT_DEFAULT_STRIPE_ROWS 4u

/* Config.flags */
#define MI355RT_FLAG_FIX_ROW_INDEX  1u  /* v = idx / width instead of the reference's idx / height (mod.rs:93-96) */
#define MI355RT_FLAG_COUNT_STEPS    2u  /* instrumented traversal: count BVH nodes visited / triangles tested */
#define MI355RT_FLAG_TIME_KERNELS   4u  /* bracket every trace-kernel launch with HIP events */
/* Intersector semantics — CREATE-time flags.
 *   default (neither flag): the reference's DEFAULT intersector, OctTreeIntersector (lib.rs:29-44 wires it): sorted
 *     front-to-back children, first leaf whose closest triangle's hit point lies inside the leaf cube wins
 *     (oct_tree_intersector.rs:148-206).  Served by the BVH (true closest hit) plus the octree CONFIRM step, which derives
 *     the octree's answer from the true closest hit exactly (csrc/traverse.hpp, confirm_walk); the octree is built with
 *     config.triangles_per_leaf.
 *   MI355RT_FLAG_OCTREE_SEMANTICS: the same semantics by walking the reference's octree directly, bug for bug — slow;
 *     kept as the independent cross-check of the confirm step.
 *   MI355RT_FLAG_TRUE_CLOSEST_HIT: the true closest hit, i.e. the reference's NoAccelerationIntersector
 *     (no_acceleration_intersector.rs:13-41); no octree is built, triangles_per_leaf is ignored. */
#define MI355RT_FLAG_OCTREE_SEMANTICS 8u
#define MI355RT_FLAG_TRUE_CLOSEST_HIT 32u
/* CREATE-time flag, testing only: the members of a device group (config.device_count > 1) all use config.device
 * instead of consecutive devices, so that the group's decomposition and gather run on a single-GPU machine. */
#define MI355RT_FLAG_GROUP_SHARES_DEVICE 16u
/* Create-time: build the BVH on the device (Morton order, Karras' parallel hierarchy, bottom-up refit: csrc/lbvh.hip) instead
 * of the host's binned-SAH build — the replacement north_star names for oct_tree_intersector.rs:66-146.  Results are identical
 * (any conservative tree gives the same hits); a frame is slower (Morton-order trees cost more node visits per ray) and create
 * is faster on large scenes.  Falls back to the host build when the device tree would be deeper than the traversal stack or the
 * scene fits one leaf; mi355rt_accel_stats out[6] then reports the host build's time and mi355rt_last_error says why. */
#define MI355RT_FLAG_DEVICE_LBVH 64u
/* Create-time: the handle keeps a DIRECT FILM next to the film (the sum of every sample's root light term), read with
 * mi355rt_film_get_direct and used by mi355rt_get_denoised_pixels_split (see there).  12 bytes per pixel more device
 * memory; without the flag every kernel, buffer and result of the handle is what it is without this feature. */
#define MI355RT_FLAG_DIRECT_FILM 128u
/* Create-time: the handle keeps one LIGHT FILM per light of the scene next to the film (see LIGHT FILMS below), read with
 * mi355rt_light_films_get and mixed without tracing by mi355rt_get_relit_pixels.  12 bytes per pixel and light more device memory; at most
 * MI355RT_LIGHT_FILMS_MAX_LIGHTS lights, one device; without the flag every kernel, buffer and result of the handle is what it is without this feature. */
#define MI355RT_FLAG_LIGHT_FILMS 256u
#define MI355RT_LIGHT_FILMS_MAX_LIGHTS 8u

typedef struct mi355rt_handle mi355rt_handle;

/* Material.diffuse, scene/mod.rs:63-69 + color.rs:98-108.  kind 0 = Diffuse::Color(rgb),
 * kind 1 = Diffuse::TextureId(tex_id).  emissive/specular/ior are never read by shading. */
typedef struct mi355rt_material {
    uint32_t kind;
    float rgb[3];
    uint32_t tex_id;
} mi355rt_material;

/* Light, scene/mod.rs:12-16 */
typedef struct mi355rt_light {
    float pos[3];
    float color[3];
} mi355rt_light;

/* Texture, scene/texture.rs:6-10: width*height RGB f32 texels (byte/256.0), row-major */
typedef struct mi355rt_texture {
    uint32_t width, height;
    const float* rgb;
} mi355rt_texture;

/* Scene, scene/mod.rs:18-23, flattened: one triangle soup in geometry order (= visual-scene
 * node order), tri_geom[i] = index of the geometry (and of its material) triangle i belongs to;
 * camera = the arguments of Camera::from_orientation_matrix for scene.cameras[0]
 * (camera.rs:22-27, lib.rs:39). */
typedef struct mi355rt_scene_desc {
    const float* tri_verts;          /* ntri * 9 floats, world space */
    const uint32_t* tri_geom;        /* ntri */
    uint32_t ntri;
    const mi355rt_material* materials;
    uint32_t nmaterials;
    const mi355rt_light* lights;
    uint32_t nlights;
    const mi355rt_texture* textures;
    uint32_t ntextures;
    float camera_orientation[16];    /* vecmath Matrix (row-vector convention) */
    float camera_fov_deg;
} mi355rt_scene_desc;

typedef struct mi355rt_config {
    uint32_t width, height;          /* create_raytracer(.., width, height), lib.rs:15 */
    uint32_t triangles_per_leaf;     /* leaf size of the reference's octree (the BVH underneath has its own) */
    uint32_t recursions;             /* RECURSIONS = 2, mod.rs:81 (0 selects the default) */
    uint32_t spread;                 /* SUB_SPREAD = 1, mod.rs:82 (0 selects the default) */
    uint32_t flags;                  /* MI355RT_FLAG_* */
    uint64_t seed;                   /* counter-RNG seed (the reference draws OS entropy); low 32 bits used */
    int32_t device;                  /* HIP device ordinal */
    /* Row-stripe ownership for multi-GPU rendering: this handle renders the stripes of
     * `stripe_rows` rows whose index is congruent to stripe_rank modulo stripe_world.
     * stripe_world <= 1 renders every row.  mi355rt_default_config sets stripe_rows = 4: thin stripes balance the ranks (the
     * slowest rank sets the frame), and the pixel tiles of a pass are cut to the stripe height, so they cost nothing per ray. */
    uint32_t stripe_rows, stripe_rank, stripe_world;
    uint32_t samples_per_pass;       /* samples per pixel traced per wavefront pass (0 = auto) */
    /* Device group: the handle drives `device_count` HIP devices of THIS process (device, device + 1, ...).  Rows
     * are dealt to them in stripes of stripe_rows; every entry point works on the group as on one device (the
     * reference's callers see one RayTracer, main.rs:183-216); mi355rt_get_tonemapped_pixels gathers the packed
     * stripes on the first device with hipMemcpyPeerAsync over xGMI.  0 or 1: one device.  Not combinable with
     * stripe_world > 1 (that is the one-process-per-GPU decomposition, gathered with mi355rt_comm_*). */
    uint32_t device_count;
} mi355rt_config;

/* Ray counters of one mi355rt_render / mi355rt_trace_frame_additive call. */
typedef struct mi355rt_ray_counts {
    uint64_t primary;        /* primary samples (the reference's own rays/s metric, stats.rs:27) */
    uint64_t bounce;         /* reflection rays, mod.rs:156-158 */
    uint64_t shadow;         /* shadow rays, mod.rs:226 */
    uint64_t primary_hits;
    uint64_t primary_culled; /* primary samples never traced: their 256-sample chunk lies outside the screen bounds of the
                              * top BVH boxes (all of them miss, mod.rs:99-100); traced primary rays = primary - primary_culled */
    uint64_t nodes_visited;  /* only with MI355RT_FLAG_COUNT_STEPS */
    uint64_t tris_tested;    /* only with MI355RT_FLAG_COUNT_STEPS */
    uint64_t trace_launches; /* trace-kernel launches (a 50-row frame: fused launches) */
    uint64_t inner_execs;    /* only with MI355RT_FLAG_COUNT_STEPS: wave-level executions of the inner-node section */
    uint64_t leaf_execs;     /* only with MI355RT_FLAG_COUNT_STEPS: wave-level executions of the triangle section */
    double trace_ms;         /* summed HIP-event time of the trace kernels (MI355RT_FLAG_TIME_KERNELS) */
    double total_ms;         /* HIP-event time of the whole call on the handle's stream */
    double trace_secondary_ms;        /* the part of trace_ms spent in launches of rounds >= 1 (reflection + shadow rays) */
    uint64_t trace_secondary_launches;
    double shader_clock_mhz; /* only with MI355RT_FLAG_COUNT_STEPS: the clock the trace waves actually ran at, sum of delta s_memtime over
                              * sum of delta s_memrealtime (100 MHz) of all waves of the call's trace launches; 0 when not measured */
    uint64_t shadow_skipped; /* shadow rays (counted in `shadow`) never traced: the depth cube map around their light proves that nothing lies
                              * between the shaded point and the light, so no intersector could block them; traced shadow rays = shadow - shadow_skipped */
    uint64_t bounce_skipped; /* reflection rays (counted in `bounce`) never traced: the direction mask of the triangle they start on proves that they
                              * hit nothing (they contribute black, mod.rs:160-171); traced reflection rays = bounce - bounce_skipped */
} mi355rt_ray_counts;

void mi355rt_default_config(mi355rt_config* cfg);

/* build_raytracer, lib.rs:29-44 (octree build replaced by a BVH build + upload).
 * Refused with MI355RT_E_INVALID, the cause in mi355rt_last_error(NULL), *out left NULL: a textured material whose tex_id is not below ntextures
 * ("material texture id out of range"), a texture with width 0, height 0 or a NULL rgb ("empty texture").  A texture's rgb must hold width * height * 3
 * floats: the struct carries no length, so that is the caller's word.
 * The four create entries never let a C++ exception out: a failed allocation and the like return an error code with the exception's text, and a file
 * whose header declares more than its data can hold (a PNG, a scene container) is refused with MI355RT_E_LOAD before anything of that size is allocated. */
int mi355rt_create(const mi355rt_scene_desc* scene, const mi355rt_config* cfg, mi355rt_handle** out);
/* create_raytracer(collada_doc, triangles_per_leaf, width, height), lib.rs:15-20.
 * data_dir (may be NULL) is where texture files are looked up (colladaloader.rs:146-150). */
int mi355rt_create_from_collada_str(const char* doc, size_t len, const char* data_dir,
                                    const mi355rt_config* cfg, mi355rt_handle** out);
/* create_raytracer_from_file(collada_filename, ...), lib.rs:22-27 */
int mi355rt_create_from_collada_file(const char* path, const mi355rt_config* cfg, mi355rt_handle** out);
/* flat scene container written by tools/dae2scene (no reference counterpart) */
int mi355rt_create_from_scene_file(const char* path, const mi355rt_config* cfg, mi355rt_handle** out);
void mi355rt_destroy(mi355rt_handle* h);

/* Error text of the last failed call; h == NULL returns the last creation error of this thread. */
const char* mi355rt_last_error(const mi355rt_handle* h);

/* RayTracer::trace_frame_additive, mod.rs:80-117: 50 rows x width pixels x 1 sample, row cursor
 * wraps modulo height; returns 50*width (0 on error).  With stripes, only owned rows are traced. */
uint32_t mi355rt_trace_frame_additive(mi355rt_handle* h);
/* Whole frame (owned stripes) x spp samples per pixel — the benchmark entry; no reference
 * counterpart (the reference has no spp concept).  counts may be NULL. */
int mi355rt_render(mi355rt_handle* h, uint32_t spp, mi355rt_ray_counts* counts);
/* The same frame, QUEUED only: returns as soon as the launches are on the handle's stream(s), like mi355rt_trace_frame_additive does;
 * mi355rt_last_counts / mi355rt_synchronize / any read-out waits for it.  Consecutive frames then run back to back on the device
 * (every later call on the handle is ordered behind it).  A device group of several devices still waits. */
int mi355rt_render_async(mi355rt_handle* h, uint32_t spp);
/* counters of the last trace_frame_additive / render call (waits for an asynchronous call to finish) */
int mi355rt_last_counts(mi355rt_handle* h, mi355rt_ray_counts* counts);

/* ---- adaptive sampling: render until every tile's noise meets a target (no reference counterpart).
 * The image is cut into image-aligned tiles of MI355RT_ADAPTIVE_TILE x MI355RT_ADAPTIVE_TILE pixels (clipped at the right and
 * bottom edges).  A tile's owned pixels are those of the handle's owned rows ((row / stripe_rows) % stripe_world == stripe_rank).
 * With n = film_n, s = film_sum[c], q = film_sumsq[c] a pixel is SETTLED when n >= 2, n >= min_spp and, for each of the three
 * channels c, the test below holds, evaluated in f32, unfused, in exactly this order (a NaN does not pass):
 *     fn  = (float)n
 *     lhs = fn*q - s*s
 *     m   = max(s, abs_floor*fn)
 *     rhs = (rel_error*rel_error) * ((fn - 1.0f) * (m*m))
 *     pass iff lhs <= rhs
 * i.e. "standard error of the mean <= rel_error * max(mean, abs_floor)" with the divisions multiplied out.
 * A tile is ACTIVE when some owned pixel of it is not settled AND (max n over its owned pixels) + batch_spp <= max_spp.
 * One round: compute the active tiles from the current film; stop if none is active or max_rounds rounds were rendered; otherwise
 * add exactly batch_spp samples (sample numbers film_n + s, as mi355rt_render numbers them) to every owned pixel of every active
 * tile and to no other pixel — no ray of any kind is traced for a pixel outside the active tiles.  The call's counters
 * (mi355rt_last_counts) are summed over the rounds and count the added samples only (primary == samples_added).
 * The call is synchronous; a queued mi355rt_render_async or drop-in speculation is settled first.  Device groups
 * (config.device_count > 1) are not supported: MI355RT_E_INVALID. */
#define MI355RT_ADAPTIVE_TILE 8u
typedef struct mi355rt_adaptive_config {
    uint32_t min_spp;     /* >= 2: a pixel with fewer samples is never settled */
    uint32_t max_spp;     /* >= min_spp: no round pushes a pixel beyond this */
    uint32_t batch_spp;   /* >= 1: samples added per round to each owned pixel of an active tile */
    uint32_t max_rounds;  /* 0: until no tile is active */
    float rel_error;      /* >= 0, finite */
    float abs_floor;      /* >= 0, finite: means below this are judged against it (dark pixels) */
} mi355rt_adaptive_config;

typedef struct mi355rt_adaptive_stats {
    uint32_t rounds;               /* passes rendered */
    uint32_t tiles;                /* tiles with >= 1 owned pixel */
    uint32_t tiles_active_first;   /* active at the first verdict of the call */
    uint32_t tiles_active_last;    /* active at the last verdict (0: everything settled or capped) */
    uint64_t samples_added;        /* increase of the sum of film_n over the call */
} mi355rt_adaptive_stats;

/* min 16, max 64, batch 16, max_rounds 0, rel_error 0.05, abs_floor 0.02 (measured choice: DESIGN.md §3c) */
void mi355rt_adaptive_default_config(mi355rt_adaptive_config* cfg);
/* Rounds as above until no tile is active (or max_rounds).  An invalid config returns MI355RT_E_INVALID, names the field in
 * mi355rt_last_error and leaves the film untouched.  stats may be NULL.  Under a lens other than MI355RT_LENS_PINHOLE this entry is refused; the same loop
 * built from mi355rt_adaptive_tile_mask and mi355rt_render_tiles (`refine`, see RENDER TILES below) runs under any lens. */
int mi355rt_render_adaptive(mi355rt_handle* h, const mi355rt_adaptive_config* cfg, mi355rt_adaptive_stats* stats);
/* The verdict the next round would use, without rendering: out[ty * tiles_x + tx] = 1 if the tile is active, else 0
 * (tiles_x = ceil(width / MI355RT_ADAPTIVE_TILE), ntiles >= tiles_x * ceil(height / MI355RT_ADAPTIVE_TILE)).
 * Returns the number of active tiles, or a negative error code. */
int mi355rt_adaptive_tile_mask(mi355rt_handle* h, const mi355rt_adaptive_config* cfg, uint8_t* out, size_t ntiles);

/* ---- denoised read-out: an edge-stopping a-trous wavelet filter over the film means, guided by the variance of each mean and by the
 * primary hit of each pixel (no reference counterpart).  It only reads: the film, the counters and every other output stay
 * as they are (a speculative 50-row frame is settled first).  Device groups (config.device_count > 1) and striped handles
 * (stripe_world > 1) are not supported: MI355RT_E_INVALID.
 *
 * GUIDES.  Pixel p of the width x height image has u = p % width and v = p / height (v = p / width with MI355RT_FLAG_FIX_ROW_INDEX: the
 * pixel -> ray mapping of the film itself), and its guide ray is mi355rt_camera_get_ray(u, v, 0.5, 0.5), intersected as
 * mi355rt_intersect_rays would.  A hit stores prim (global triangle index), depth = t, normal = the triangle normal shading uses
 * (mod.rs:198-205) and albedo = shade()'s diffuse colour (mod.rs:242-248: the material colour, or its texture at the hit's (u, v)).  A miss
 * stores prim 0xFFFFFFFF, depth 0 and a zero normal and albedo.  The guides are kept on the device and rebuilt only when the camera or the
 * FIX_ROW_INDEX flag changes.
 *
 * FILTER.  Everything is f32, unfused, in the order written; pos(x) = x > 0 ? x : 0 (NaN -> 0).  From the film (n, s[3], q[3]), fn = (float)n:
 *     n == 0 : the pixel is EMPTY: never a tap, and its output is the film mean as it stands (NaN: white once packed)
 *     c      = s * (1.0f / fn)                                                  per channel (mi355rt_film_get_pixels)
 *     n >= 2 : v_ch = pos(fn*q - s*s) / ((fn*fn) * (fn - 1.0f)) per channel, var = (v_r + v_g) + v_b  (the variance of the mean)
 *     n == 1 : the variance is UNKNOWN, var = 0
 * Iteration i = 0 .. iterations-1, step h = 1 << i, reads the previous iteration's (c, var); for every non-empty pixel p at (x, y):
 *     W = 0, S = (0, 0, 0), V = 0
 *     for dy = -2..2, for dx = -2..2: tap q at (x + dx*h, y + dy*h); skip it when outside the image or empty
 *         k = K1[dx+2] * K1[dy+2], K1 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
 *         q == p: w = k
 *         else: skip the tap when exactly one of p, q is a miss;  both miss: g = 1;  both hit:
 *             d  = (Np.x*Nq.x + Np.y*Nq.y) + Np.z*Nq.z;  wn = pos(d), squared normal_power_log2 times
 *             rz = |tp - tq| / (sigma_depth * tp);   wz = 1.0f / (1.0f + rz*rz)
 *             ra = ((|Ap.r-Aq.r| + |Ap.g-Aq.g|) + |Ap.b-Aq.b|) / sigma_albedo;  wa = 1.0f / (1.0f + ra*ra)
 *             g  = (wn * wz) * wa
 *           wl = 1 when p or q has unknown variance, else, with L(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b, dl = L(cp) - L(cq):
 *             wl = 1.0f / (1.0f + (dl*dl) / ((sigma_luminance*sigma_luminance) * (varp + varq) + 1e-12f))
 *           w = pos((k * g) * wl)
 *         S += w * cq (per channel);  W += w;  V += (w*w) * varq
 *     c' = S / W (per channel), var' = V / (W*W)
 * rgb = c after the last iteration; packed = that c mapped as mi355rt_get_tonemapped_pixels maps a film mean (c/(1+c), to u8, 0xAARRGGBB).
 * iterations = 0 returns exactly mi355rt_film_get_pixels and mi355rt_get_tonemapped_pixels.
 * Device memory, allocated on the first call that needs it and counted in mi355rt_hbm_allocated_bytes: 32 bytes per pixel for the guides,
 * 52 more per pixel on the first denoised read-out. */
typedef struct mi355rt_denoise_config {
    uint32_t iterations;          /* 0..10; 0 = the film means unchanged */
    uint32_t normal_power_log2;   /* 0..10 */
    float sigma_luminance;        /* > 0, finite */
    float sigma_depth;            /* > 0, finite */
    float sigma_albedo;           /* > 0, finite */
} mi355rt_denoise_config;
/* iterations 5, normal_power_log2 7, sigma_luminance 1, sigma_depth 0.1, sigma_albedo 0.1 (measured choice: DESIGN.md §3d) */
void mi355rt_denoise_default_config(mi355rt_denoise_config* cfg);
/* rgb: npix*3 floats, packed: npix u32 (either may be NULL, not both); npix >= width*height.  An invalid config returns MI355RT_E_INVALID,
 * names the field in mi355rt_last_error and writes nothing. */
int mi355rt_get_denoised_pixels(mi355rt_handle* h, const mi355rt_denoise_config* cfg, float* rgb, uint32_t* packed, size_t npix);
/* ---- direct film and split read-out (MI355RT_FLAG_DIRECT_FILM; no reference counterpart).  Almost all of a film's noise is in
 * the bounce tree; the light arriving at the primary hit straight from the lights has none beyond pixel jitter, yet it carries the shadow
 * edges, the highlights and the texture detail that the filter above blurs.  A handle created with the flag therefore keeps that part of
 * the film apart, and a second denoised read-out filters only what is left.
 *
 * DIRECT FILM.  direct[width*height*3], f32, zero at creation.  Whenever a sample is added to a pixel's film (PixelData::add_sample,
 * film.rs:20-24) the pixel gets direct = direct + L0, in the same place and in the same sample order.  L0 is the root node's light sum of
 * the sample, the first term of its colour L0 + (...) * 0.5 (mod.rs:146-175 with mod.rs:211-254: the node_L[0] of mi355rt_debug_sample); it
 * is (0, 0, 0) for a primary miss, for a hit the octree semantics drop and for every sample that writes no light term.  So direct[p] is the
 * sequential f32 sum over the pixel's samples of node_L[0], bit for bit.  It is cleared wherever the film is cleared (mi355rt_film_clear,
 * which the reference's loop calls after every camera move); a pixel whose film is not written (an inactive tile of mi355rt_render_adaptive,
 * a row the handle does not own) keeps its direct sum.
 *
 * mi355rt_film_get_direct returns the sums, width*height*3 floats.  It follows mi355rt_film_get: queued work and a speculative 50-row frame
 * are settled first, a striped handle returns zero for the rows it does not own, a device group gathers its members' rows.  A handle
 * without the flag: MI355RT_E_INVALID, mi355rt_last_error names MI355RT_FLAG_DIRECT_FILM, nothing is written.
 *
 * SPLIT READ-OUT.  mi355rt_get_denoised_pixels_split takes the arguments, the validation and the side-effect rules of
 * mi355rt_get_denoised_pixels (device groups and striped handles: MI355RT_E_INVALID) and also refuses a handle without the flag.  From the
 * film (n, s[3], q[3]) and the direct sums d[3], fn = (float)n, everything f32, unfused, in this order:
 *     n == 0 : the pixel is EMPTY: never a tap, and its output is the film mean as it stands
 *     inv = 1.0f / fn;  c = s * inv;  cd = d * inv;  ci = c - cd                 per channel
 *     var exactly as FILTER defines it from s and q: the variance of the TOTAL.  (Evaluated on the CPU, a second variance of the indirect
 *     samples alone bought nothing — tone-mapped RMSE 0.01197 against 0.01193 at 8 spp, 0.00690 against 0.00692 at 32 — so the film keeps one
 *     more sum per pixel, not two.)
 *     the `iterations` a-trous iterations of FILTER on (ci, var), unchanged: the luminance term is now on ci, var' = V / (W*W) as there
 *     rgb = cd + ci' per channel; packed = that value mapped as mi355rt_get_tonemapped_pixels maps a film mean
 * iterations = 0 returns exactly mi355rt_film_get_pixels and mi355rt_get_tonemapped_pixels (not cd + (c - cd)).
 * Device memory: the guides and the filter's buffers of mi355rt_get_denoised_pixels, shared with it; nothing more. */
int mi355rt_film_get_direct(mi355rt_handle* h, float* sum_rgb);
int mi355rt_get_denoised_pixels_split(mi355rt_handle* h, const mi355rt_denoise_config* cfg, float* rgb, uint32_t* packed, size_t npix);
/* the guide buffers above, width*height entries each (normal3, albedo3: 3 floats per pixel); any pointer may be NULL */
int mi355rt_get_guides(mi355rt_handle* h, float* depth, float* normal3, float* albedo3, uint32_t* prim, size_t npix);

/* ---- display read-out: exposure, tone curves, sRGB, auto-exposure (no reference counterpart).  mi355rt_get_tonemapped_pixels is the
 * reference's c / (1 + c) truncated to 8 bits: linear values that every viewer reads as sRGB, no exposure.  This read-out maps any of the three images
 * the handle can produce through an exposure, one of four tone curves and one of two transfers.  It only reads, under the denoiser's rules: a queued
 * mi355rt_render_async and a speculative 50-row frame are settled first; the film, the counters, mi355rt_current_row and the changed-row tracking of
 * mi355rt_get_tonemapped_pixels stay as they are.  Device groups (config.device_count > 1) and striped handles (stripe_world > 1) are not supported, for
 * every source: MI355RT_E_INVALID (add the stripes into one handle first: RECIPES below).
 *
 * SOURCE IMAGE.  c[p] is, per pixel, exactly the three floats the named read-out returns as `rgb`; an empty pixel therefore carries its film mean as it
 * stands.  n[p] is the film count.  `dn` is ignored for SOURCE_FILM; for the other two NULL means mi355rt_denoise_default_config.  One call runs the
 * denoiser at most once, also with auto_exposure.
 *
 * HISTOGRAM (mi355rt_display_histogram).  Per pixel: n == 0 counts in `empty`, whatever its sums.  Otherwise L = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b,
 * f32, unfused (the L of FILTER above); L NaN counts in `nan`; L <= 0 counts in `nonpositive`; otherwise, with bits(L) the float's bit pattern,
 *     b = clamp((int)(bits(L) >> 20) - 856, 0, 255);  bins[b] += 1;  max_bits = max(max_bits, bits(L))   (unsigned)
 * i.e. eight bins per octave, cut on the float's own exponent and top three mantissa bits, from 2^-20 to 2^12; everything below (denormals included) lands
 * in bin 0, everything above (+inf included) in bin 255.  Every output is an integer that does not depend on the order of accumulation.
 *
 * AUTO-EXPOSURE (mi355rt_display_auto_exposure; HOST code, IEEE double).  N = sum of bins; lo = floor((double)low * N), hi = ceil((double)high * N).  Bin b
 * holds the ranks [C_b, C_b + bins[b]) with C_b the running sum; kept_b = max(0, min(C_b + bins[b], hi) - max(C_b, lo)); K = sum of kept_b;
 *     mean = (sum over b ascending of kept_b * centre_b) / K,   centre_b = (b + 856.5) / 8.0 - 127.0
 *     *exposure = (float)((double)key * exp2(-mean));   K == 0: *exposure = 1.0f (and the call returns 0)
 * key must be finite and > 0, and 0 <= low < high <= 1: otherwise MI355RT_E_INVALID, mi355rt_last_error(NULL) names the field and nothing is written.
 *
 * sRGB TABLE (mi355rt_display_srgb_thresholds; HOST code).  out[k - 1] = T[k] for k = 1..255: e = (k - 0.5) / 255, T[k] = (float)EOTF(e) in double,
 * EOTF(e) = e / 12.92 for e <= 0.04045, else ((e + 0.055) / 1.055)^2.4.  Strictly increasing in f32 (smallest gap 3.0e-4).  The device reads this
 * table; no powf runs there.
 *
 * DISPLAY MAPPING (mi355rt_get_display_pixels).  With the effective exposure E, per channel, f32, unfused, in this order:
 *     x = c * E
 *     CURVE_REINHARD        y = x / (1.0f + x)
 *     CURVE_REINHARD_WHITE  y = (x * (1.0f + x / (white*white))) / (1.0f + x)
 *     CURVE_ACES            y = (x * (2.51f*x + 0.03f)) / (x * (2.43f*x + 0.59f) + 0.14f)
 *     CURVE_CLAMP           y = x
 *     z = fmaxf(fminf(y, 1.0f), 0.0f)                      (a NaN becomes 1: white, as the reference has it)
 *     TRANSFER_REFERENCE    u = (uint32_t)(z * 255.0f) & 0xFF
 *     TRANSFER_SRGB         u = number of k in 1..255 with T[k] <= z
 *     packed = B | G << 8 | R << 16 | 255 << 24
 * E is config.exposure when auto_exposure == 0; otherwise the auto-exposure of the source's histogram with config.key / low / high.  *exposure_used
 * (may be NULL) receives E either way.  With mi355rt_display_default_config the call returns exactly mi355rt_get_tonemapped_pixels; sources 1 and 2 with
 * the other fields at their defaults return the `packed` of mi355rt_get_denoised_pixels / _split.
 *
 * ERRORS.  npix != width * height, an unknown source, curve or transfer, auto_exposure > 1, a bad float field (exposure is checked only when it is used,
 * white, key, low and high always), a bad `dn`, a NULL output, SOURCE_DENOISED_SPLIT on a handle without MI355RT_FLAG_DIRECT_FILM (the message names the
 * flag): MI355RT_E_INVALID, mi355rt_last_error names the field and nothing is written.
 * Device memory, allocated on first use and counted in mi355rt_hbm_allocated_bytes: the histogram's 1040 bytes; with the first mi355rt_get_display_pixels
 * also the table (1 KiB) and 4 bytes per pixel; for sources 1 and 2 the denoiser's buffers, shared with it. */
#define MI355RT_DISPLAY_SOURCE_FILM            0u  /* the film means, mi355rt_film_get_pixels */
#define MI355RT_DISPLAY_SOURCE_DENOISED        1u  /* rgb of mi355rt_get_denoised_pixels */
#define MI355RT_DISPLAY_SOURCE_DENOISED_SPLIT  2u  /* rgb of mi355rt_get_denoised_pixels_split (needs MI355RT_FLAG_DIRECT_FILM) */
#define MI355RT_CURVE_REINHARD        0u
#define MI355RT_CURVE_REINHARD_WHITE  1u
#define MI355RT_CURVE_ACES            2u
#define MI355RT_CURVE_CLAMP           3u
#define MI355RT_TRANSFER_REFERENCE    0u  /* (u8)(z * 255), truncating: what mi355rt_get_tonemapped_pixels does */
#define MI355RT_TRANSFER_SRGB         1u
#define MI355RT_HIST_BINS 256u

typedef struct mi355rt_luminance_histogram {
    uint32_t bins[MI355RT_HIST_BINS];
    uint32_t empty;        /* pixels with film n == 0 */
    uint32_t nan;          /* non-empty pixels whose L is NaN */
    uint32_t nonpositive;  /* non-empty pixels with L <= 0 (includes -0.0 and -inf) */
    uint32_t max_bits;     /* bit pattern of the largest L counted in bins[] (0 when none; +inf is 0x7F800000) */
} mi355rt_luminance_histogram;

typedef struct mi355rt_display_config {
    uint32_t source, curve, transfer;
    uint32_t auto_exposure;   /* 0: use `exposure`; 1: derive it from the source's histogram (key, low, high); `exposure` is ignored */
    float exposure;           /* > 0, finite */
    float white;              /* > 0, finite; read by CURVE_REINHARD_WHITE only, validated always */
    float key, low, high;     /* key > 0 finite; 0 <= low < high <= 1 */
} mi355rt_display_config;

/* source FILM, CURVE_REINHARD, TRANSFER_REFERENCE, auto_exposure 0, exposure 1, white 4, key 0.18 (the usual middle grey), low 0, high 1 */
void mi355rt_display_default_config(mi355rt_display_config* cfg);
/* DISPLAY MAPPING of an image that is no film (a baked atlas): npix x 3 floats of host memory -> packed 0xAARRGGBB, by the kernel and with the rules of
 * mi355rt_get_display_pixels at the fixed exposure cfg->exposure; cfg->source is not read; cfg == NULL: exposure 1, the Reinhard curve and the reference's
 * transfer, i.e. mi355rt_get_tonemapped_pixels' map.  Every buffer is a temporary of the call; nothing of the handle changes.  MI355RT_E_INVALID for a device
 * group, an invalid config, auto_exposure (it reads a film source's histogram), NULL pointers with npix > 0, npix > 2^28. */
int mi355rt_display_image(mi355rt_handle* h, const float* rgb3, size_t npix, const mi355rt_display_config* cfg /* may be NULL */, uint32_t* packed);
int mi355rt_display_histogram(mi355rt_handle* h, uint32_t source, const mi355rt_denoise_config* dn, mi355rt_luminance_histogram* out);
int mi355rt_display_auto_exposure(const mi355rt_luminance_histogram* hist, float key, float low, float high, float* exposure);   /* HOST only */
int mi355rt_display_srgb_thresholds(float out[255]);                                                                             /* HOST only */
int mi355rt_get_display_pixels(mi355rt_handle* h, const mi355rt_display_config* cfg, const mi355rt_denoise_config* dn,
                               uint32_t* packed, size_t npix, float* exposure_used /* may be NULL */);

/* RayTracer::get_tonemapped_pixels, mod.rs:120-128: width*height u32 0xAARRGGBB (A = 255). */
int mi355rt_get_tonemapped_pixels(mi355rt_handle* h, uint32_t* out, size_t n);
/* Same, written to DEVICE memory on the handle's device (e.g. a buffer owned by the caller's
 * collective library).  Rows owned by this handle only, packed in ascending row order:
 * mi355rt_owned_rows(h) * width values.  Synchronous with respect to the host. */
int mi355rt_tonemap_owned_rows_device(mi355rt_handle* h, uint32_t* device_out, size_t n);
/* Same, ASYNCHRONOUS: the kernel is launched on the caller's HIP stream (`hip_stream` is a hipStream_t),
 * after everything this handle has queued; the call returns at once and the write is ordered with the
 * caller's other work on that stream (buffer initialisation before, the collective after).  Later calls on
 * this handle wait for it. */
int mi355rt_tonemap_owned_rows_device_on_stream(mi355rt_handle* h, uint32_t* device_out, size_t n, void* hip_stream);
uint32_t mi355rt_owned_rows(const mi355rt_handle* h);
/* ascending list of the rows this handle owns */
int mi355rt_owned_row_list(const mi355rt_handle* h, uint32_t* rows, size_t n);

/* Film, film.rs:27-68.  pixel_datas: sum_rgb / sumsq_rgb hold width*height*3 floats, n holds
 * width*height counts; any pointer may be NULL. */
int mi355rt_film_get(mi355rt_handle* h, float* sum_rgb, float* sumsq_rgb, uint32_t* n);
int mi355rt_film_clear(mi355rt_handle* h);                                   /* Film::clear, film.rs:37-41 */
int mi355rt_film_get_pixels(mi355rt_handle* h, float* rgb);                  /* Film::get_pixels, film.rs:43-47 */
int mi355rt_film_get_estimated_variances(mi355rt_handle* h, float* rgb);     /* film.rs:51-67 */

/* ---- film set, add, save and load: resume and combine renders (no reference counterpart).  The film (n, sum, sumsq, and direct
 * with MI355RT_FLAG_DIRECT_FILM) is all a progressive render accumulates, and sample s of a call is numbered film_n + s (see mi355rt_render_adaptive
 * above), so a film that is put back is a complete checkpoint: a render continued from it equals, bit for bit, one that was never interrupted.
 *
 * SET AND ADD.  The planes are whole images in the layout of mi355rt_film_get / mi355rt_film_get_direct: sum_rgb, sumsq_rgb and direct_rgb hold
 * width*height*3 floats, n holds width*height counts.  npix must equal width*height; sum_rgb, sumsq_rgb and n are required; direct_rgb must be
 * non-NULL exactly when the handle has MI355RT_FLAG_DIRECT_FILM.  A violation returns MI355RT_E_INVALID, names the argument in mi355rt_last_error
 * and leaves the film untouched.  The values are data: they are not validated.
 *     set : the film's entries become the input's, bits unchanged (a NaN keeps its payload, -0.0 its sign)
 *     add : per pixel and channel s' = s + a, q' = q + b, d' = d + e, each ONE f32 addition with the handle's value on the left, and n' = n + m in
 *           u32 (an overflow of n is the caller's business: not checked)
 * Only the rows the handle owns (mi355rt_owned_row_list: (row / stripe_rows) % stripe_world == stripe_rank) are written; the input's other rows are
 * ignored, so on a striped handle every other row stays zero, as mi355rt_film_clear, mi355rt_film_get and the tone-mapper expect.  A device group
 * (config.device_count > 1) hands the planes to each member, which takes its own rows: mi355rt_film_get afterwards returns what one handle would.
 * A queued mi355rt_render_async and a speculative 50-row frame are settled first (the frame's rows are given back BEFORE the film is written; the
 * other order would overwrite the new film), every row is marked changed for mi355rt_get_tonemapped_pixels, and nothing else of the handle changes:
 * camera, seed, flags, mi355rt_current_row, the last counters, the denoiser's guides and the culling caches stay.  The call returns once the
 * caller's arrays may be reused; later calls on the handle are ordered behind it.  The device staging (28 bytes per pixel, 40 with a direct plane)
 * is temporary: mi355rt_hbm_allocated_bytes is the same before and after.
 *
 * FILM FILE, version 1, little-endian: a 64-byte header, then the planes, nothing else.
 *     header: magic "MI355FLM" (8 bytes) | u32 version = 1 | u32 width | u32 height | u32 planes (bit 0: a direct plane is present; other bits 0)
 *             | u64 seed (low 32 bits used) | u32 flags (the handle's config.flags at save) | zeros up to byte 64
 *     planes: n (u32 x npix) | sum (f32 x 3 npix) | sumsq (f32 x 3 npix) | direct (f32 x 3 npix, only with bit 0 of `planes`);  npix = width*height
 * The file's length must be exactly 64 + npix * 28 (40 with a direct plane) bytes.
 * mi355rt_film_save writes what mi355rt_film_get and mi355rt_film_get_direct return (a striped handle: zeros in the rows it does not own; a device
 * group: its gathered film).  A file that cannot be written: MI355RT_E_LOAD.
 * mi355rt_film_load reads and checks the WHOLE file before it touches the device, then sets (add == 0) or adds (add != 0) its planes as above.
 * It returns MI355RT_E_LOAD, names the reason in mi355rt_last_error and leaves the film untouched for: a file that cannot be read, bad magic or
 * version, unknown `planes` bits, a width or height that differs from the handle's, a wrong file length, a MI355RT_FLAG_FIX_ROW_INDEX bit in the
 * header's flags that differs from the handle's current flag (the pixel -> ray mapping differs), and a file without a direct plane for a handle with
 * MI355RT_FLAG_DIRECT_FILM.  A file WITH a direct plane loads into a handle without the flag: the plane is skipped (the header said it was there).
 * Neither the camera nor the scene is checked: that the film belongs to this view is the caller's word.
 * mi355rt_film_file_info is HOST code (no device, no handle): out = version, width, height, planes, seed low, seed high, flags, 0.  It makes the
 * file's own checks (magic, version, planes bits, non-zero size, length), returns MI355RT_E_LOAD for them and leaves the reason in
 * mi355rt_last_error(NULL).
 *
 * RECIPES.  Resume: save; later create a handle with the same scene, camera, seed and flags, load, render on.  Stripes to the denoiser: add every
 * rank's mi355rt_film_get (zero outside its rows, so 0 + x is exact) into one unstriped handle, which then serves mi355rt_get_denoised_pixels.
 * Disjoint sample ranges of one seed: a worker sets zero sums with n = offset and renders k samples, its film then holds samples offset ..
 * offset + k - 1; the caller subtracts offset from its n before merging. */
int mi355rt_film_set(mi355rt_handle* h, const float* sum_rgb, const float* sumsq_rgb, const uint32_t* n, const float* direct_rgb, size_t npix);
int mi355rt_film_add(mi355rt_handle* h, const float* sum_rgb, const float* sumsq_rgb, const uint32_t* n, const float* direct_rgb, size_t npix);
int mi355rt_film_save(mi355rt_handle* h, const char* path);
int mi355rt_film_load(mi355rt_handle* h, const char* path, int add);
int mi355rt_film_file_info(const char* path, uint32_t out[8]);

/* Camera, camera.rs:63-78 (the `pub camera` field of RayTracer, mod.rs:38). */
int mi355rt_camera_move_rel(mi355rt_handle* h, float x, float y, float z);
int mi355rt_camera_add_x_angle(mi355rt_handle* h, float radians);
int mi355rt_camera_add_y_angle(mi355rt_handle* h, float radians);
/* rotation_matrix / orientation_matrix after update_matrices (camera.rs:92-98), max_x, max_y */
int mi355rt_camera_get(const mi355rt_handle* h, float rot16[16], float orient16[16], float max_xy[2]);
/* Camera::get_ray, camera.rs:80-90, with explicit jitter (xi1, xi2 in [0,1)): out = pos3, dir3 */
int mi355rt_camera_get_ray(const mi355rt_handle* h, uint32_t u, uint32_t v, float xi1, float xi2, float ray6[6]);

/* Re-seed: afterwards the handle renders what a handle created with this seed renders (the per-sample hash key AND
 * the 65 536-entry direction table are functions of the seed; only its low 32 bits are used).  The film is kept. */
int mi355rt_set_seed(mi355rt_handle* h, uint64_t seed);
/* Run-time flags (FIX_ROW_INDEX, COUNT_STEPS, TIME_KERNELS).  The create-time flags (OCTREE_SEMANTICS, TRUE_CLOSEST_HIT, GROUP_SHARES_DEVICE,
 * DEVICE_LBVH, DIRECT_FILM) are fixed at creation: pass the bits as they were created, a call that would change one fails with
 * MI355RT_E_INVALID and changes nothing. */
int mi355rt_set_flags(mi355rt_handle* h, uint32_t flags);
/* Number of concurrent frame slices mi355rt_render splits its rows into (1..8, default 3, or the
 * environment variable MI355RT_SLICES).  Each slice runs its wavefront passes on its own HIP stream, so the
 * drain window of one slice's trace launch is filled by another slice's kernels; results do not depend on
 * it.  With MI355RT_FLAG_TIME_KERNELS the per-kernel times only mean something with 1 slice. */
int mi355rt_set_slices(mi355rt_handle* h, uint32_t slices);
uint32_t mi355rt_get_slices(const mi355rt_handle* h);

/* Intersector::intersect_ray, accel_intersect.rs:10-13, batched on the device: rays6 = n x
 * (pos3, dir3); out tuv = n x 3 (untouched on a miss), prim = n global triangle indices
 * (0xFFFFFFFF on a miss; geometry_index = tri_geom[prim], vertex_index = 3 * index within
 * the geometry, mod.rs:17-21).  Semantics of the handle's intersector (see the flags above): by default the
 * reference's OctTreeIntersector, with MI355RT_FLAG_TRUE_CLOSEST_HIT the true closest hit (lowest t, ties to
 * the lowest triangle index). */
int mi355rt_intersect_rays(mi355rt_handle* h, const float* rays6, size_t n, float* tuv, uint32_t* prim);
/* shadow-ray predicate of shade(), mod.rs:222-230: blocked[i] = 1 iff the closest hit of ray i
 * has 0.01 < t < 1.0 */
int mi355rt_occluded_rays(mi355rt_handle* h, const float* rays6, size_t n, uint8_t* blocked);

/* ---- caller-supplied rays: radiance along any ray, and custom cameras (no reference counterpart).  Everything above renders through one
 * ray generator, the reference's pinhole camera (camera.rs:80-90).  These two entries open the seam one step below it: the caller brings the primary rays
 * and the library does everything after ray generation exactly as it does for its own — the same kernels, the same bounce tree, the same arithmetic.  A
 * sample's colour depends only on its ray, its hits and its key (pixel, sampleno): shade() reads ray.dir, never the camera.  So an orthographic, panoramic
 * or fisheye view, depth of field, a lens-distortion model, a stereo pair or an irradiance probe is a ray generator on the caller's side
 * (raytracer_rs_amd.cameras has four).
 *
 * RAYS.  rays6 = n x (pos3, dir3) f32, 4-byte aligned, used AS GIVEN: dir is not normalised (the camera's own rays have |dir| ~ 1.11), t and the
 * specular term follow dir as they do in mi355rt_intersect_rays.  Non-finite rays are data and are handled as mi355rt_intersect_rays handles them.
 * WHERE.  MI355RT_RAYS_HOST: every pointer of the call is host memory; the library stages it through temporary device buffers (24 bytes per ray, 8 per
 * key, 12 / 12 / 12 / 4 per ray of the outputs asked for, 16 per ray of a pass for tuv or prim), so mi355rt_hbm_allocated_bytes is the same before and
 * after, apart from pass buffers that grew.  MI355RT_RAYS_DEVICE: every pointer is device memory on the handle's device (a torch tensor's data_ptr), read
 * and written in place by kernels on the handle's stream; the call is synchronous with respect to the host, like mi355rt_tonemap_owned_rows_device, and work
 * the caller queued on other streams that produces the rays must have finished.
 *
 * mi355rt_trace_rays: the radiance of n arbitrary rays.  It touches no film.  keys2 = n x (pixel, sampleno), or NULL for (i, 0): the key replaces
 * (pixel, sampleno) in every hash of the sample's bounce tree ({key0, key1, 1 + child_node, seed}, mod.rs:187 as this library seeds it) and need not be a
 * pixel of the image; two rays with the same key draw the same random numbers.  Outputs (any pointer of `out` may be NULL, not all of them):
 *     rgb    n x 3: the sample's radiance, compute_radiance's value (mod.rs:146-175; the color3 of mi355rt_debug_sample); (0, 0, 0) for a miss
 *     direct n x 3: node_L[0], the root light sum (the DIRECT FILM's L0 above); (0, 0, 0) for a miss
 *     tuv    n x 3 and prim n: exactly what mi355rt_intersect_rays returns for the same rays (tuv untouched on a miss)
 * The call follows the read-out rules of mi355rt_debug_sample: a queued mi355rt_render_async and a speculative 50-row frame are settled first; the film, the
 * direct film, the camera, mi355rt_current_row, the changed-row tracking of mi355rt_get_tonemapped_pixels and the denoiser's guides stay as they are.
 * mi355rt_last_counts afterwards reports primary == n, primary_hits == the number of hits and primary_culled == 0 (no camera made the rays: nothing is
 * culled, and the primary round walks the tree).  n == 0 succeeds and writes nothing.  Any n < 2^32 is served, in as many passes as the pass buffers need
 * (config.samples_per_pass, when set, bounds a pass at that many images' worth of rays).  Striped handles serve it: rays belong to no row.
 *
 * mi355rt_render_rays: mi355rt_render with the caller's rays.  rays6[(s * npix + p) * 6] is the ray of the CALL's sample s of film pixel p (npix = width *
 * height, p the index the film planes use); nrays must equal npix * spp.  Sample s of pixel p has the key (p, film_n[p] + s), as mi355rt_render numbers it;
 * the samples are added to the film (and to the direct film with MI355RT_FLAG_DIRECT_FILM) in sample order.  Rows the handle does not own are neither read
 * nor written.  Counters and `counts` are as for mi355rt_render, with primary_culled == 0.  With the camera's own rays (cameras.pinhole) the film equals
 * mi355rt_render(spp) bit for bit; with any other rays MI355RT_FLAG_FIX_ROW_INDEX has nothing to act on.
 * THE GUARD.  The denoiser's guides and the adaptive sampler's view of the image are built from the handle's camera, so they would be wrong for a film of
 * other rays.  mi355rt_render_rays marks the film as holding caller-ray samples; mi355rt_film_clear and mi355rt_film_set lift the mark (mi355rt_film_add and
 * mi355rt_film_load with add != 0 keep it).  While it is set mi355rt_get_denoised_pixels, mi355rt_get_denoised_pixels_split, the display entries with
 * sources 1 and 2 and mi355rt_render_adaptive return MI355RT_E_INVALID with a message that names mi355rt_render_rays.  The film, variance, tone-mapped and
 * SOURCE_FILM display read-outs and film add / save / load work as always.  mi355rt_trace_rays never sets the mark.
 *
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error, nothing written: a NULL rays6 with n > 0; `out` NULL or all of its pointers NULL;
 * an unknown `where`; nrays != width * height * spp; spp == 0; a device group (config.device_count > 1). */
#define MI355RT_RAYS_HOST   0u   /* every pointer of the call is host memory */
#define MI355RT_RAYS_DEVICE 1u   /* every pointer is device memory on the handle's device (a torch tensor's data_ptr);
                                    synchronous with respect to the host, like mi355rt_tonemap_owned_rows_device */
typedef struct mi355rt_ray_outputs {   /* any pointer may be NULL, not all of them */
    float*    rgb;     /* n x 3: the sample's radiance, compute_radiance's value; (0,0,0) for a miss */
    float*    direct;  /* n x 3: node_L[0], the root light sum (the DIRECT FILM's L0) */
    float*    tuv;     /* n x 3 and */
    uint32_t* prim;    /* n: exactly what mi355rt_intersect_rays returns for the same rays */
} mi355rt_ray_outputs;
int mi355rt_trace_rays(mi355rt_handle* h, const float* rays6, const uint32_t* keys2 /* n x (pixel, sampleno); NULL: (i, 0) */,
                       size_t n, uint32_t where, const mi355rt_ray_outputs* out);
int mi355rt_render_rays(mi355rt_handle* h, const float* rays6, size_t nrays, uint32_t spp, uint32_t where, mi355rt_ray_counts* counts);

/* ---- lens models: depth of field and orthographic views made on the device (no reference counterpart).  A handle has a LENS: the ray
 * generator of mi355rt_render.  PINHOLE is the reference's camera and the state of every handle at creation; with it every entry launches the kernels and
 * returns the bits it always did.  THIN and ORTHO are raytracer_rs_amd.cameras.thin_lens and .orthographic made by the kernels themselves, in registers,
 * bit for bit: no 24-byte-per-ray buffer, and — because the library knows each pixel's centre ray — guides, so the denoised, split and display read-outs
 * work on such a film.
 *
 * THE RAY OF A SAMPLE.  Sample `sampleno` of pixel p: (w0, w1, w2, w3) = pcg4d(p, sampleno, 0, seed); xi1 = u01(w0), xi2 = u01(w1) (the jitter, as always),
 * l1 = u01(w2), l2 = u01(w3) (the lens sample; nothing else uses these words).  rot, orient, max_xy: what mi355rt_camera_get returns; origin[k] =
 * 0 * orient[k] + 0 * orient[4 + k] + 0 * orient[8 + k] + 1 * orient[12 + k].  Every expression is f32, unfused, evaluated as written (raytracer_rs_amd/cameras.py
 * is the statement; k = 0, 1, 2):
 *   PINHOLE  x = p % width, y = p / width with MI355RT_FLAG_FIX_ROW_INDEX, else p / height (the reference's row)
 *            dir_x = -max_x + (2 * max_x) * ((x + xi1) / width), dir_y = -max_y + (2 * max_y) * ((y + xi2) / height)
 *            d[k] = dir_x * rot[k] + (-dir_y) * rot[4 + k] + 1 * rot[8 + k] + 1 * rot[12 + k],  o[k] = origin[k]
 *   THIN     (o, d) as PINHOLE; lx = 2 * l1 - 1, ly = 2 * l2 - 1; off[k] = radius * (lx * rot[k] + ly * rot[4 + k]);
 *            o'[k] = o[k] + off[k], d'[k] = focus * d[k] - off[k]: a point of a square lens of half-width radius, through o + focus * d, which stays sharp
 *   ORTHO    hw = width_world * 0.5, hh = hw * (height / width); x = p % width, y = p / width (always the true row)
 *            sx = -hw + (2 * hw) * ((x + xi1) / width), sy = -hh + (2 * hh) * ((y + xi2) / height)
 *            o[k] = (origin[k] + sx * rot[k]) + (-sy) * rot[4 + k],  d[k] = rot[8 + k] + rot[12 + k]
 * A THIN lens with radius 0 and focus 1 makes the pinhole's rays but is NOT folded into the pinhole path: it runs the lens kernels.
 *
 * mi355rt_set_lens.  Only the fields the model reads are checked: THIN needs radius finite and >= 0 and focus finite and > 0, ORTHO needs width_world finite
 * and > 0; an unknown model is an error.  A failure returns MI355RT_E_INVALID, names the field in mi355rt_last_error and changes nothing.  Setting a lens
 * keeps the film, as a camera move does (that the film belongs to the view stays the caller's word), and does not touch the caller-ray mark, the counters or
 * mi355rt_current_row.  The guides' cache is keyed by (camera, FIX_ROW_INDEX bit, lens).  On a device group (config.device_count > 1) a model other than
 * PINHOLE is refused with MI355RT_E_INVALID.
 *
 * WITH A LENS OTHER THAN PINHOLE
 *   mi355rt_render, mi355rt_render_async   render through it; film and direct film accumulate as always, sample s of pixel p has key (p, film_n[p] + s); striped
 *                                          handles render their rows.  primary_culled == 0 and the primary round walks the tree: the culling rectangles, the
 *                                          coverage mask and the tile bins describe pinhole rays and are not used.  The ordering contract of render_async holds.
 *   mi355rt_get_guides, mi355rt_get_denoised_pixels[_split], display sources 1 and 2
 *                                          use the lens's guide ray: the lens ray with xi1 = xi2 = l1 = l2 = 0.5, intersected as mi355rt_intersect_rays would.
 *                                          Everything else of GUIDES and FILTER is as written above.
 *   mi355rt_trace_frame_additive           returns 0, and
 *   mi355rt_render_adaptive                returns MI355RT_E_INVALID; both messages name mi355rt_set_lens (their fused launch and tile masks rest on the pinhole path).
 *   mi355rt_adaptive_tile_mask, mi355rt_render_tiles
 *                                          work under every lens (RENDER TILES below): the verdict only reads the film, and masked lens passes honour the tile mask.
 *   mi355rt_camera_get_ray, mi355rt_trace_rays, mi355rt_render_rays are unaffected.
 *
 * mi355rt_lens_ray: HOST code — no device, no handle — the lens ray from the outputs of mi355rt_camera_get; flags: bit 0 = MI355RT_FLAG_FIX_ROW_INDEX.  The lens
 * is validated as by mi355rt_set_lens; NULL pointers, width or height 0 or pixel >= width * height give MI355RT_E_INVALID, the argument named in
 * mi355rt_last_error(NULL), ray6 untouched.
 * mi355rt_lens_rays: the rays the next mi355rt_render(spp) would take under the handle's lens (PINHOLE included), in mi355rt_render_rays layout: ray
 * (s * npix + p) has key (p, film_n[p] + s); every pixel is written, owned or not.  `where` as for mi355rt_trace_rays (HOST: staged through a temporary
 * device buffer of 24 bytes per ray).  nrays must equal width * height * spp, spp >= 1; else MI355RT_E_INVALID and nothing is written.  A read-out by the
 * rules of mi355rt_trace_rays: queued work is settled first, nothing of the handle changes.  Not available on a device group. */
#define MI355RT_LENS_PINHOLE 0u   /* the reference's camera: everything as it is without a lens */
#define MI355RT_LENS_THIN    1u   /* cameras.thin_lens(radius, focus) */
#define MI355RT_LENS_ORTHO   2u   /* cameras.orthographic(width_world) */
typedef struct mi355rt_lens { uint32_t model; float radius, focus, width_world; } mi355rt_lens;
void mi355rt_lens_default(mi355rt_lens* lens);            /* PINHOLE, radius 0, focus 1, width_world 0 */
int  mi355rt_set_lens(mi355rt_handle* h, const mi355rt_lens* lens);
int  mi355rt_get_lens(const mi355rt_handle* h, mi355rt_lens* lens);
int  mi355rt_lens_ray(const float rot16[16], const float orient16[16], const float max_xy[2], uint32_t width, uint32_t height, uint32_t flags,
                      const mi355rt_lens* lens, uint32_t pixel, float xi1, float xi2, float l1, float l2, float ray6[6]);
int  mi355rt_lens_rays(mi355rt_handle* h, uint32_t spp, uint32_t where, float* rays6, size_t nrays);

/* ---- RENDER TILES: samples into the tiles of a caller's mask, under any lens (no reference counterpart).
 * One round of the adaptive sampler with the verdict supplied by the caller: a crop, a region of interest, tiles farmed out to several handles and merged
 * with mi355rt_film_add — or, from mi355rt_adaptive_tile_mask (which only reads the film and works under any lens) and this call, the adaptive loop run on the
 * caller's side, which under a lens is adaptive depth of field (raytracer_rs_amd/adaptive.py: refine; csrc/raytracer_lib.hpp: RayTracer::refine).
 *
 * TILES AND MASK.  The tiles are the image-aligned MI355RT_ADAPTIVE_TILE x MI355RT_ADAPTIVE_TILE tiles of the adaptive section; tile_mask[ty * tiles_x + tx] != 0
 * selects tile (tx, ty); ntiles must equal tiles_x * tiles_y exactly (tiles_x = ceil(width / MI355RT_ADAPTIVE_TILE), tiles_y likewise from the height).
 *
 * THE CALL adds exactly spp samples to every owned pixel of every selected tile.  Sample s of pixel p has the key (p, film_n[p] + s), as mi355rt_render numbers
 * it; the samples go into the film — and into the direct film with MI355RT_FLAG_DIRECT_FILM — in sample order.  No bit of any other pixel's film or direct
 * film changes, and no ray of any kind is traced for a pixel outside the selected tiles.  Every pixel therefore ends with the bits of a uniform render of its
 * own sample count.
 *
 * LENS.  Works under MI355RT_LENS_PINHOLE, THIN and ORTHO.  Under the pinhole it uses the tile bins, the culling and the cached verdicts exactly as a round of
 * mi355rt_render_adaptive does; under a lens it runs lens passes as mi355rt_render does (the primary round walks the tree, nothing is culled).
 *
 * COUNTERS (counts may be NULL; mi355rt_last_counts gives the same).  primary == spp * (owned pixels in selected tiles); every other counter counts the added
 * samples only.  primary_culled follows the adaptive round's rule under the pinhole (culled samples of selected tiles) and is 0 under a lens.
 *
 * AROUND THE CALL.  Synchronous like mi355rt_render; a queued mi355rt_render_async and a speculative 50-row frame are settled first.  The touched rows are
 * marked changed for mi355rt_get_tonemapped_pixels.  Camera, lens, seed, mi355rt_current_row, the guides and the caller-ray mark are untouched; an existing
 * caller-ray mark is ignored, as mi355rt_render ignores it.  Striped handles render their owned pixels of the selected tiles.  An all-zero mask succeeds,
 * renders nothing and reports zero counters.
 *
 * WHERE.  MI355RT_RAYS_HOST: the mask is host memory and is copied into a handle-owned device buffer of ntiles bytes (allocated on first use, shared with the
 * adaptive sampler's verdict, counted in mi355rt_hbm_allocated_bytes).  MI355RT_RAYS_DEVICE: the mask is device memory on the handle's device (a torch uint8
 * tensor's data_ptr); it is read in place — and copied back once, ntiles bytes, for the sample count — and must not change during the call.
 *
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing changed, for: tile_mask NULL; ntiles != tiles_x * tiles_y; spp == 0; an
 * unknown `where`; a device group (config.device_count > 1). */
int  mi355rt_render_tiles(mi355rt_handle* h, const uint8_t* tile_mask, size_t ntiles, uint32_t spp, uint32_t where, mi355rt_ray_counts* counts);

/* ---- FEATURE FILM: per-sample guides, coverage (alpha), denoising under any rays (no reference counterpart).
 * The GUIDES of the denoised read-out rest on one centre ray per pixel: pinhole-sharp under a thin lens, absent for a film of mi355rt_render_rays, aliased
 * at every edge, and silent about which share of a pixel's samples hit the scene.  The feature film accumulates the PRIMARY HIT's attributes over jittered
 * samples, under the handle's lens or along the caller's rays, beside the film.  It is a read-side pass of its own: no trace, shade, resolve or fused
 * launch changes, and a handle that never calls these entries allocates nothing and launches nothing new.
 *
 * PLANES.  Five planes over width * height pixels: n (u32), hits (u32), depth (f32), normal (3 x f32), albedo (3 x f32): 36 bytes per pixel, allocated (zeroed)
 * on the first call that needs them and counted in mi355rt_hbm_allocated_bytes.  There is no create-time flag.
 *
 * mi355rt_features_render(h, spp).  For every owned pixel p and s = 0 .. spp-1, in this order: the sample's key is (p, feat_n[p] + s); its ray is the ray
 * mi355rt_lens_rays would make for that key under the handle's current lens (PINHOLE included, and the MI355RT_FLAG_FIX_ROW_INDEX mapping): lens_ray with the
 * four pcg4d(p, sampleno, 0, seed) words; its hit (t, u, v, prim) is what mi355rt_intersect_rays returns for that ray in the handle's intersector semantics.
 * Then n += 1 and, ON A HIT ONLY (a miss adds nothing, not even +0.0):
 *     hits += 1;  depth = depth + t;  normal[c] = normal[c] + N[prim][c];  albedo[c] = albedo[c] + A[c]
 * with N and A exactly the normal and albedo GUIDES defines above; each is one f32 addition with the handle's value on the left, in sample order.  Because the
 * keys are the film's own, a feature film and a film that both start cleared and take the same spp see the SAME RAYS: hits[p] is then the number of the
 * film's samples that hit.
 *
 * mi355rt_features_render_rays(h, rays6, nrays, spp, where).  The same accumulation along caller rays; layout and `where` as in mi355rt_render_rays: ray
 * (s * npix + p), nrays == npix * spp, HOST is staged through a temporary device buffer, DEVICE is read in place.  Keys play no part: nothing is random after
 * the ray.  Rows the handle does not own are neither read nor written.
 *
 * mi355rt_features_get(h, n, hits, depth, normal3, albedo3, npix).  Any pointer may be NULL, not all of them; npix must equal width * height.  A striped
 * handle returns zeros in the rows it does not own.  A feature film that was never allocated reads as zeros (and stays unallocated).
 * mi355rt_features_clear(h).  Zeroes the planes (owned rows) and the view stamp below.
 * mi355rt_features_alpha(h, alpha, npix).  alpha[p] = n == 0 ? 0.0f : (float)hits / (float)n: one IEEE division.
 *
 * VIEW STAMP.  The first accumulation into a cleared feature film records what made its rays: the camera (rotation, orientation, max_xy, the FIX_ROW_INDEX bit
 * and the lens: the key of the guides cache), or "caller rays".  A later mi355rt_features_render under a different camera stamp, or a mix of camera and caller
 * rays, returns MI355RT_E_INVALID, names mi355rt_features_clear in mi355rt_last_error and writes nothing.  mi355rt_film_clear, mi355rt_film_set, camera moves
 * and mi355rt_set_lens do NOT touch the feature film.
 *
 * AROUND THE CALLS.  Synchronous like mi355rt_get_guides; a queued mi355rt_render_async and a speculative 50-row frame are settled first.  The film, the
 * direct film, the counters of mi355rt_last_counts, mi355rt_current_row, the changed-row tracking and the caller-ray mark stay as they are.  Striped handles
 * work on their rows.
 *
 * GUIDE SOURCE.  mi355rt_set_guide_source(h, MI355RT_GUIDES_CENTRE | MI355RT_GUIDES_FEATURES); CENTRE is the state at creation, and with it every entry
 * returns the bits it returns without this section.  With FEATURES, mi355rt_get_guides, mi355rt_get_denoised_pixels, ..._split, and
 * mi355rt_display_histogram / mi355rt_get_display_pixels with sources 1 and 2 take their guides from the feature film; per pixel, f32, unfused, in this order:
 *     h = hits[p];  h == 0 (which includes n == 0): a miss guide (prim 0xFFFFFFFF, zeros)
 *     fh = (float)h;  inv = 1.0f / fh
 *     depth = dsum * inv;   m[c] = nsum[c] * inv;   albedo[c] = asum[c] * inv
 *     len = sqrtf((m.x*m.x + m.y*m.y) + m.z*m.z)
 *     normal[c] = len > 0 ? m[c] / len : 0.0f          (three divisions)
 *     prim = 0                                          (the filter only asks "miss or not")
 * The converted guides are cached in guide buffers of their own (32 bytes per pixel, allocated on first use) and rebuilt when the feature film changes.
 * Under FEATURES: an empty feature film (never accumulated since its last clear) returns MI355RT_E_INVALID; a camera-stamped feature film whose stamp
 * differs from the handle's current view returns MI355RT_E_INVALID and names mi355rt_features_clear; the caller-ray guard on the film is LIFTED for the
 * denoised and display read-outs when the feature film is caller-stamped — if it is not, the read-out is refused with a message naming
 * mi355rt_features_render_rays.  mi355rt_render_adaptive stays refused for a caller-ray film.
 *
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: a device group (config.device_count > 1); spp == 0; nrays !=
 * width * height * spp; npix != width * height; rays6 NULL; an unknown `where` or guide source; every output pointer NULL.
 * Film files, mi355rt_film_set / _add do not carry the feature film. */
#define MI355RT_GUIDES_CENTRE   0u   /* one centre ray per pixel: GUIDES of the denoised read-out */
#define MI355RT_GUIDES_FEATURES 1u   /* the feature film's means */
int  mi355rt_features_render(mi355rt_handle* h, uint32_t spp);
int  mi355rt_features_render_rays(mi355rt_handle* h, const float* rays6, size_t nrays, uint32_t spp, uint32_t where);
int  mi355rt_features_get(mi355rt_handle* h, uint32_t* n, uint32_t* hits, float* depth, float* normal3, float* albedo3, size_t npix);
int  mi355rt_features_clear(mi355rt_handle* h);
int  mi355rt_features_alpha(mi355rt_handle* h, float* alpha, size_t npix);
int  mi355rt_set_guide_source(mi355rt_handle* h, uint32_t source);
uint32_t mi355rt_get_guide_source(const mi355rt_handle* h);

/* ---- LIGHT FILMS: a film per light, and relighting without tracing (no reference counterpart).
 * A sample's colour is a sum over the scene's lights: every term of its bounce tree is (diffuse * ndl + spec) * light.color of one light (mod.rs:214-257).
 * A handle created with MI355RT_FLAG_LIGHT_FILMS keeps, beside the film, nlights planes light[li][width * height * 3] of f32, zero at creation, owned by the
 * handle and counted in mi355rt_hbm_allocated_bytes (12 bytes per pixel and light).  nlights == 0 is allowed (no planes).  mi355rt_create* refuses the flag
 * with MI355RT_E_INVALID, the cause in mi355rt_last_error(NULL), for a scene of more than MI355RT_LIGHT_FILMS_MAX_LIGHTS lights and for a device group
 * (config.device_count > 1).  mi355rt_set_flags passes the bit unchanged and cannot toggle it.
 *
 * STATEMENT.  The light radiance R_li of a sample is compute_radiance's value (mod.rs:146-175) with the same fold, the same order and the same 1 / k factors,
 * where each node's light sum is (+0.0f) + term[node][li] instead of the sum over all lights: the sample's colour in a scene in which every other light's
 * colour is (0, 0, 0).  It is (0, 0, 0) for a sample without a slot (a primary miss, or a hit the octree semantics drop).  Whenever a sample is added to a
 * pixel's film (PixelData::add_sample), light[li] = light[li] + R_li for every li: one f32 addition with the handle's value on the left, in sample order,
 * as the direct film takes L0.  So every entry that adds samples through the resolve (mi355rt_render, _render_async, _render_adaptive, _render_tiles,
 * _render_rays, under any lens) adds to the light films for the same pixels and no others; an inactive tile, an unowned row or an unselected tile keeps its
 * bits; a pixel of a culled block takes +0.0 once, as the film does.  The film itself (sum, sumsq, n, direct) is, bit for bit, the film of the same handle
 * without the flag.  With one light, light[0] equals the film's sum.  The planes add up to the film's sum only to rounding: the film adds the lights per
 * node before the fold, the planes after it.
 *   mi355rt_film_clear clears the light films (owned rows).  mi355rt_film_set / _add / _load / _save and film files do NOT carry them: after a film_set
 *   the caller restores them with the entries below, and that they match the film is the caller's word.
 *   mi355rt_trace_frame_additive on a handle with the flag returns 0 and mi355rt_last_error names MI355RT_FLAG_LIGHT_FILMS (the fused 50-row kernel keeps
 *   no light films).  mi355rt_debug_sample and mi355rt_trace_rays touch no light film.
 *
 * mi355rt_light_films_get / _set / _add: layout light_rgb[(li * npix + p) * 3 + c].  Queued work is settled first; only owned rows are written, a striped
 * handle reads zeros elsewhere; set keeps bit patterns (a NaN's payload, -0.0); add is one f32 addition with the handle's value on the left; nothing else of
 * the handle changes.  The staging buffer of set / add is temporary: mi355rt_hbm_allocated_bytes is the same before and after.
 *
 * mi355rt_get_relit_pixels: the frame under other light colours, without tracing.  weights3: nweights == nlights * 3 floats, an RGB factor per light (data,
 * not validated).  Per pixel p and channel ch, f32 and unfused, with n the film's count:
 *     fn = (float)n;  inv = 1.0f / fn
 *     c[ch] = +0.0f;  for li ascending:  m = light[li][p][ch] * inv;  c[ch] = c[ch] + weights3[li * 3 + ch] * m
 * Nothing special is done for n == 0 (NaN, white once packed, like the film's read-out).  rgb (npix * 3 floats) receives c.  packed: with display == NULL
 * c is mapped as mi355rt_get_tonemapped_pixels maps a film mean; otherwise DISPLAY MAPPING of the display section is applied to c, display->source must be
 * MI355RT_DISPLAY_SOURCE_FILM, and auto_exposure == 1 derives E from the HISTOGRAM of c with the film's n deciding `empty`; *exposure_used (may be NULL)
 * receives E (1 with display == NULL).  Either of rgb and packed may be NULL, not both.  The call only reads.  A striped handle serves its rows; elsewhere
 * its planes and n are zero.  Device memory allocated on the first call and counted in mi355rt_hbm_allocated_bytes: 16 bytes per pixel (c and packed) and 96 bytes (the weights), and
 * with the first non-NULL display the display section's histogram and sRGB table (1040 + 1024 bytes) where that section has not allocated them yet.
 *
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: a handle without the flag (the message names
 * MI355RT_FLAG_LIGHT_FILMS); nlights != the scene's; nweights != nlights * 3; npix != width * height; a NULL light_rgb with nlights > 0; a NULL weights3
 * with nweights > 0; rgb and packed both NULL; a display config that mi355rt_get_display_pixels refuses, or whose source is not the film. */
int  mi355rt_light_films_get(mi355rt_handle* h, float* light_rgb, size_t nlights, size_t npix);
int  mi355rt_light_films_set(mi355rt_handle* h, const float* light_rgb, size_t nlights, size_t npix);
int  mi355rt_light_films_add(mi355rt_handle* h, const float* light_rgb, size_t nlights, size_t npix);
int  mi355rt_get_relit_pixels(mi355rt_handle* h, const float* weights3, size_t nweights, const mi355rt_display_config* display /* may be NULL */,
                              float* rgb, uint32_t* packed, size_t npix, float* exposure_used /* may be NULL */);

/* ---- GATHER: light arriving at caller-given points, sampled on the device (no reference counterpart).
 * The points are a film of their own: per point n, sum, sumsq (and hits, near), accumulated in sample order.  The rays are made on the device from the
 * renderer's own hemisphere sampler; everything about a ray after it is made is mi355rt_trace_rays.
 *
 * THE SAMPLE.  Sample s of point i has the key (id_i, first_sample + s); id_i = ids[i], or i with ids == NULL.
 *     start = (uint32_t)(((uint64_t)h0 * 65535) >> 32),  h0 = word 0 of pcg4d(id_i, first_sample + s, 0xFFFFFFFE, seed)       (a hash stream of its own)
 *     d = table[start];  while dot(d, normal) <= 0:  start = (start + 1) % 65535, d = table[start]          (reflection_ray's walk, mod.rs:187-189)
 *     ray = (point + 0.00001f * d, d)                                                                         (mod.rs:192-193)
 * dot(d, n) = d.x * n.x + d.y * n.y + d.z * n.z, f32, unfused, left to right.  The normal is used as given (not normalised; pass unit normals).  The walk stops
 * after one full turn of the table: a normal no entry satisfies (zero, or so small that every product underflows) makes the sample VOID: n does not count
 * it and nothing is added for it.  A NaN normal accepts the start entry (NaN <= 0 is false).  normals3 == NULL is SPHERE MODE: no walk, d = table[start].
 * The ray is traced under its key as mi355rt_trace_rays traces it.
 *
 * PER POINT, in sample order, for every sample that is not void, with w = 1 (MI355RT_GATHER_MEAN) or w = 2.0f * dot(d, normal) (MI355RT_GATHER_COSINE) and
 * v = w * rgb per channel (one f32 multiply, unfused):
 *     sum += v;  sumsq += v * v;  n += 1;  hits += hit;  near += hit && t < near_distance          (t as mi355rt_intersect_rays reports it)
 * accumulate != 0: the outputs are read, added to and written back, so gather(3) followed by gather(5, first_sample 3, accumulate) is gather(8) bit for bit;
 * otherwise they start from 0.  mean = sum / n is the reference's bounce estimator at the point (MEAN), or irradiance / pi (COSINE: the table is uniform
 * on the sphere, the accepted half has density 1 / (2 pi)).
 *
 * DIRECT (needs normals; always overwritten, never accumulated): the point-light term of shade() (mod.rs:207-261) without material and specular.  Over the
 * lights in scene order: l = light - p, ndl = dot(normal, normalized(l)); a light with ndl < 0 is skipped; the shadow ray (p + l * 0.01f, l) is blocked by
 * the rule of mi355rt_occluded_rays; otherwise direct += color * ndl (from +0.0f).
 *
 * AROUND THE CALL.  The read-out rules of mi355rt_trace_rays: a queued or speculative frame is settled first; film, direct film, light films, camera, lens,
 * current row, caller-ray mark and guides are untouched; mi355rt_last_counts reports the rays traced (npoints * spp primary); striped handles serve it.
 * `where` as for mi355rt_trace_rays: every pointer (points3, normals3, ids and the outputs) is host memory, staged, or device memory, used in place on the
 * handle's stream.  Every temporary is freed by the end of the call (pass buffers that grew excepted, as for mi355rt_trace_rays).
 *
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: NULL points3 with npoints > 0; out NULL or all outputs NULL;
 * cfg NULL; spp == 0 while n, hits, near, sum or sumsq is asked for; COSINE or direct without normals; an unknown weight or where; a NaN near_distance;
 * npoints * spp >= 2^32; first_sample + spp overflowing 32 bits; a device group.  npoints == 0 succeeds and writes nothing.
 *
 * mi355rt_gather_ray: THE SAMPLE on the host, no handle: the same header the kernel compiles (csrc/gather_walk.hpp).  table3: 65536 x 3 floats
 * (mi355rt_get_sample_table).  ray6 receives the ray; a void sample gets the harmless ray of the start entry and *valid = 0 (valid may be NULL). */
#define MI355RT_GATHER_MEAN   0u   /* w = 1: the reference's bounce estimator (mod.rs:146-175) */
#define MI355RT_GATHER_COSINE 1u   /* w = 2 * dot(d, normal): mean = irradiance / pi under the table's uniform hemisphere */
typedef struct mi355rt_gather_config  { uint32_t spp, first_sample, weight, accumulate; float near_distance; } mi355rt_gather_config;
typedef struct mi355rt_gather_outputs { uint32_t *n, *hits, *near; float *sum, *sumsq, *direct; } mi355rt_gather_outputs;  /* any may be NULL, not all */
void mi355rt_gather_default_config(mi355rt_gather_config* cfg);   /* spp 16, first_sample 0, MEAN, accumulate 0, near_distance +inf */
int  mi355rt_gather(mi355rt_handle* h, const float* points3, const float* normals3 /* NULL: whole sphere */, const uint32_t* ids /* NULL: i */,
                    size_t npoints, const mi355rt_gather_config* cfg, uint32_t where, const mi355rt_gather_outputs* out);
int  mi355rt_gather_ray(const float* table3 /* 65536 x 3 */, uint32_t seed, const float point[3], const float* normal3 /* may be NULL */,
                        uint32_t id, uint32_t sampleno, float ray6[6], uint32_t* valid);

/* ---- BAKE: UV charts to surface points, and per-point values back into an atlas with filled borders (no reference counterpart).
 * A lightmap bake is mi355rt_bake_texels, then mi355rt_gather at the points it lists, then mi355rt_bake_atlas.  raytracer-rs_amd/bake.py states all of it.
 *
 * TEXELS.  uv: ntri x 3 x 2 floats, one UV triangle (a, b, c) per scene triangle in scene order; u runs to the right and v downwards; texel (x, y) has
 * index y * width + x and its centre at (x + 0.5, y + 0.5).  f32, unfused, in the order written:
 *     px_k = u_k * (float)width,  py_k = v_k * (float)height;   cx = (float)x + 0.5f,  cy = (float)y + 0.5f
 *     edge(p, q) = (px_p - cx) * (py_q - cy) - (py_p - cy) * (px_q - cx);   e0 = edge(b, c), e1 = edge(c, a), e2 = edge(a, b), s = (e0 + e1) + e2
 *     covered <=> ((e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0)) && s != 0
 *                 && floor(min px) - 1 <= x <= floor(max px) + 1 && floor(min py) - 1 <= y <= floor(max py) + 1           (THE BOX)
 *     owner(x, y) = the LOWEST triangle index that covers the texel, 0xFFFFFFFF if none;   u = e1 / s,  v = e2 / s  (the hit record's u, v)
 *     P = (A + u * (B - A)) + v * (C - A) per component, A B C the triangle's vertices as given at create
 * The edge functions are relative to the centre, so edge(p, q) == -edge(q, p) exactly: two triangles that share an edge with the same UV bits never both
 * reject a centre because of it.  Both windings count (mirrored charts).  A triangle with a NaN or infinite px or py covers nothing; triangles off the atlas are cut by it, nothing
 * is clamped.  THE BOX holds every exactly covered centre with a texel to spare; it keeps a sliver from claiming a far centre that only the rounding of
 * its edge functions gives it, and it is what lets the device bin the triangles.
 * Outputs (any may be NULL, not all of them and ncovered): owner u32 [w * h]; bary f32 [w * h * 2], untouched where uncovered; and the compact lists of
 * the covered texels in ascending texel index, which the caller sizes for w * h entries: ids (the texel index: the gather's key, so a bake does not depend on
 * chart order or chunking), points3, normals3 (the triangle's normal as shading uses it, calc_normal mod.rs:198-205; flip != 0: negated), albedo3 (the
 * material's diffuse colour, or its texture's texel at (u, v) as texture.rs:21-27 fetches it).  *ncovered: their length.
 * `where` as for mi355rt_gather: every pointer but ncovered is host memory, staged, or device memory used in place on the handle's stream.
 *
 * ATLAS.  ids[n] (texel indices), values3[n x 3] -> atlas f32 [w * h * 3] and valid u8 [w * h] (either may be NULL, not both): the values scattered, 0
 * elsewhere, valid 1 where scattered.  Then `dilate` times, from the PREVIOUS iteration's image: an empty texel with a non-empty 8-neighbour becomes
 * (((v0 + v1) + v2) + ...) / (float)count over the neighbours that exist and are not empty, in the order N, W, E, S, NW, NE, SW, SE (N is y - 1), f32 with one
 * division; its valid becomes 1 + k in iteration k = 1, 2, ..., saturating at 255.  The atlas borders do not wrap.  An empty texel that can be filled
 * at all is filled by iteration max(w, h) - 1, so min(dilate, max(w, h) - 1) iterations are run: the result is that of `dilate` iterations.
 *
 * AROUND THE CALLS.  A speculative frame is settled first and a queued one runs ahead; film, direct film, light films, feature film, camera, lens, current
 * row, caller-ray mark, guides and mi355rt_last_counts are untouched.  Every temporary is freed by the end of the call; the first mi355rt_bake_texels that
 * asks for points3 keeps 36 bytes per triangle (A, B - A, C - A in scene order) on the device for the handle's life, counted in mi355rt_hbm_allocated_bytes.
 * Striped handles serve both calls (a bake is no part of the image).
 *
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: a device group; an unknown `where`; width or height 0 or
 * above 16384; uv NULL on a scene with triangles; every output NULL; ids or values3 NULL with n > 0; n > width * height; an id >= width * height; an id
 * named twice (the order of the two would decide the texel).
 *
 * mi355rt_bake_texel: TEXELS for one triangle and one texel on the host, no handle: the same header the kernels compile (csrc/bake_raster.hpp).
 * *covered: 0 or 1; bary2 = (u, v) when covered, else untouched.  mi355rt_bake_point: P of one component, (a + u * e1) + v * e2.
 * mi355rt_bake_dilate_texel: one dilation step for the empty texel (x, y) of an image on the host; returns the count, rgb3 written when it is not 0.
 *
 * mi355rt_bake_auto_atlas: a chart for a mesh that has none, host only.  Two triangles per square cell of *cell texels, cells row by row from the top
 * left, cell the largest that fits ceil(ntri / 2) cells into the atlas.  With g = gutter, L = cell - 2 g, d = max(g - 0.5, 0.5), leg = L - d, (ox, oy) the
 * cell's corner, in texels:  even i: (ox + g, oy + g), (ox + g + leg, oy + g), (ox + g, oy + g + leg);  odd i: (ox + cell - g, oy + cell - g),
 * (ox + cell - g - leg, oy + cell - g), (ox + cell - g, oy + cell - g - leg);  uv = texels / (float)size.  No texel is claimed twice, texels of different
 * triangles are at least max(gutter, 1) apart (Chebyshev), of different cells 2 gutter + 1.  Refused (MI355RT_E_INVALID, mi355rt_last_error(NULL)) when
 * L < 1 + d: a half would own no texel. */
typedef struct mi355rt_bake_texel_outputs { uint32_t *owner; float *bary; uint32_t *ids; float *points, *normals, *albedo; } mi355rt_bake_texel_outputs;
int  mi355rt_bake_texels(mi355rt_handle* h, const float* uv, uint32_t width, uint32_t height, uint32_t flip, uint32_t where,
                         const mi355rt_bake_texel_outputs* out, uint32_t* ncovered /* host memory; may be NULL */);
int  mi355rt_bake_atlas(mi355rt_handle* h, const uint32_t* ids, const float* values3, size_t n, uint32_t width, uint32_t height, uint32_t dilate, uint32_t where,
                        float* atlas /* may be NULL */, uint8_t* valid /* may be NULL */);
int  mi355rt_bake_texel(const float uv6[6], uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t* covered, float bary2[2]);
float mi355rt_bake_point(float a, float e1, float e2, float u, float v);
uint32_t mi355rt_bake_dilate_texel(const float* atlas3, const uint8_t* valid, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float rgb3[3]);
int  mi355rt_bake_auto_atlas(uint32_t ntri, uint32_t width, uint32_t height, uint32_t gutter, float* uv /* ntri x 6 */, uint32_t* cell /* may be NULL */);

/* ---- PROBES: gathered light as spherical-harmonic coefficients, and a grid lookup (no reference counterpart).
 * A probe is a film of its own: per point n and 9 x 3 sums (and hits, near), accumulated in sample order over mi355rt_gather's SPHERE-MODE samples.  The
 * lookup is a read-out of such a film laid out as a grid.  raytracer-rs_amd/probes.py states all of it.  Everything is f32, unfused, in the order written.
 *
 * THE BASIS.  Real spherical harmonics up to band 2, polynomial in the direction d = (x, y, z), which is used as given:
 *     b_0 = c0          b_1 = c1 * y        b_2 = c1 * z                          b_3 = c1 * x        b_4 = c2 * (x * y)
 *     b_5 = c2 * (y * z)                    b_6 = c3 * (3.0f * (z * z) - 1.0f)    b_7 = c2 * (x * z)  b_8 = c4 * (x * x - y * y)
 *     c0 = 0.282094792f, c1 = 0.488602512f, c2 = 1.092548431f, c3 = 0.315391565f, c4 = 0.546274215f
 *
 * GATHER.  Sample s of point i is exactly mi355rt_gather's sphere-mode sample: key (id_i, first_sample + s), hash stream 0xFFFFFFFE, d = table[start], ray
 * (point + 0.00001f * d, d), traced under its key as mi355rt_trace_rays traces it.  Per point, in sample order:
 *     sh[k][c] += b_k(d) * rgb_c   (one multiply, one add);   n += 1;   hits += hit;   near += hit && t < near_distance
 * sh is npoints x 9 x 3 floats.  accumulate != 0: the outputs are read, added to and written back, so probes_gather(3) followed by probes_gather(5,
 * first_sample 3, accumulate) is probes_gather(8) bit for bit; otherwise they start from 0.  The radiance arriving from direction w is estimated by
 * sum_k (4 pi / n) * sh[k] * b_k(w): the table is uniform on the sphere.
 * Around the call mi355rt_gather's rules hold: a speculative frame is settled and a queued one runs ahead; every film, camera, lens, current row, caller-ray
 * mark and guide is untouched; mi355rt_last_counts reports the rays (npoints * spp primary); striped handles serve it; every temporary is freed by the end of
 * the call (pass buffers that grew excepted).  `where` as for mi355rt_gather.
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: NULL points3 with npoints > 0; out NULL or all of its
 * pointers NULL; cfg NULL; spp == 0; an unknown where; a NaN near_distance; npoints * spp >= 2^32; first_sample + spp overflowing 32 bits; a device group.
 * npoints == 0 succeeds and writes nothing.
 *
 * LOOKUP of one query (p, dir) in a grid.  Probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix and sits at origin_a + (float)i_a * spacing_a; n is u32 per
 * probe, sh f32 [probe][9][3] (the sums above), usable u8 per probe (optional).  In this order:
 *     per axis a:  g = (p_a - origin_a) / spacing_a;  g = g >= 0.0f ? g : 0.0f  (a NaN becomes 0: no index is ever made from a NaN);
 *                  top = (float)(count_a - 1);  g = g <= top ? g : top;  i = (uint32_t)g;  if (count_a >= 2 && i > count_a - 2) i = count_a - 2;
 *                  f = g - (float)i;  with count_a == 1: i = 0, f = 0
 *     corner j = 0 .. 7: bit 0 is x + 1, bit 1 is y + 1, bit 2 is z + 1, the index clamped to count_a - 1;  t_j = (wx * wy) * wz with w_a = f_a for a set
 *                  bit and 1.0f - f_a otherwise.  A corner is SKIPPED if t_j == 0, if n_j == 0, or if usable is given and usable[j] == 0; a skipped corner
 *                  is never read into a sum, so an infinity in it cannot make a NaN out of a zero weight
 *     over the corners used, in j order, from +0.0f:  wsum += t_j;  s_j = t_j * (12.566370614f / (float)n_j);  C[k][c] += s_j * sh_j[k][c]
 *     MI355RT_SH_RADIANCE (from dir):         r_c = sum_k C[k][c] * b_k(dir), in k order from +0.0f
 *     MI355RT_SH_IRRADIANCE (at normal dir):  r_c = sum_k (A_k * C[k][c]) * b_k(dir);  A_0 = 3.14159265f, A_1..A_3 = 2.09439510f, A_4..A_8 = 0.785398163f
 *     rgb_c = r_c / wsum, ok = 1;  no corner used: rgb = 0, ok = 0
 * Nothing is clamped: a band-2 irradiance can ring below zero, and that is data.
 * mi355rt_probes_lookup traces nothing.  Around the call mi355rt_bake_texels' rules hold: films, camera, lens and mi355rt_last_counts are untouched, a striped
 * handle serves it.  `where` as for mi355rt_gather: every pointer is host memory, staged, or device memory used in place on the handle's stream.
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: grid NULL; a zero count; a count product of 2^31 or more; a
 * spacing that is not finite and positive; a non-finite origin; n, sh or rgb3 NULL; points3 or dirs3 NULL with npoints > 0; an unknown mode; an unknown
 * where; a device group.  npoints == 0 succeeds and writes nothing.
 *
 * Host only, no handle, the same header the kernels compile (csrc/sh9.hpp): mi355rt_sh9_basis (THE BASIS), mi355rt_probes_lookup_one (LOOKUP of one query,
 * *ok may be NULL; the grid is checked as above, the message in mi355rt_last_error(NULL)), mi355rt_probe_grid_points (the probes' positions in index order,
 * counts product x 3 floats). */
#define MI355RT_SH_RADIANCE   0u
#define MI355RT_SH_IRRADIANCE 1u
typedef struct mi355rt_probe_config  { uint32_t spp, first_sample, accumulate; float near_distance; } mi355rt_probe_config;   /* 16 bytes */
typedef struct mi355rt_probe_outputs { uint32_t *n, *hits, *near; float *sh; } mi355rt_probe_outputs;   /* sh: npoints x 9 x 3; any may be NULL, not all */
typedef struct mi355rt_probe_grid    { float origin[3], spacing[3]; uint32_t counts[3]; } mi355rt_probe_grid;   /* 36 bytes */
void mi355rt_probes_default_config(mi355rt_probe_config* cfg);   /* spp 64, first_sample 0, accumulate 0, near_distance +inf */
int  mi355rt_probes_gather(mi355rt_handle* h, const float* points3, const uint32_t* ids /* NULL: i */, size_t npoints, const mi355rt_probe_config* cfg, uint32_t where,
                           const mi355rt_probe_outputs* out);
int  mi355rt_probes_lookup(mi355rt_handle* h, const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable /* may be NULL */,
                           const float* points3, const float* dirs3, size_t npoints, uint32_t mode, uint32_t where, float* rgb3, uint8_t* ok /* may be NULL */);
int  mi355rt_sh9_basis(const float dir[3], float b[9]);
int  mi355rt_probes_lookup_one(const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable /* may be NULL */, const float point[3],
                               const float dir[3], uint32_t mode, float rgb[3], uint32_t* ok /* may be NULL */);
int  mi355rt_probe_grid_points(const mi355rt_probe_grid* grid, float* points3);

/* ---- PROBE VISIBILITY: depth moments per probe, and a lookup that trusts a probe less where it does not see (no reference counterpart).
 * Each probe also records how far it sees in each direction: a DEPTH FILM of res x res texels over an octahedral map of the sphere, per texel count (u32) and
 * the sums of dist and dist * dist (f32), accumulated in sample order over the SAME samples as PROBES' gather.  The weighted lookup multiplies each corner's
 * trilinear weight by a Chebyshev bound on the chance that the probe sees as far as the query.  raytracer-rs_amd/probes.py states all of it.  Everything is
 * f32, unfused, in the order written, with + - * / sqrt, comparisons and integer conversions only.
 *
 * THE MAP of a direction v = (x, y, z), used as given (not normalised), to the unit square:
 *     s = (|x| + |y|) + |z|;  px = x / s;  py = y / s;
 *     z < 0:  (px, py) = ((1 - |py|) * sx, (1 - |px|) * sy), both right sides from the old values, sx = x >= 0 ? 1 : -1, sy likewise
 *     u = px * 0.5f + 0.5f;  w = py * 0.5f + 0.5f
 * THE TEXEL of a sample: per axis g = u * (float)res, made 0 where !(g >= 0), i = min((uint32_t)g, res - 1); the texel's index is iy * res + ix.
 *
 * GATHER_DEPTH.  The samples, keys and rays are mi355rt_probes_gather's, traced once.  Per point, in sample order, with D = depth->max_distance:
 *     dist = hit ? (t < D ? t : D) : D   (a NaN t becomes D);   k = texel(d);   count[k] += 1;   moments[k][0] += dist;   moments[k][1] += dist * dist
 * Every sample goes into exactly one texel.  count is npoints x res * res u32, moments npoints x res * res x 2 f32.  `out` may be NULL (the depth film alone);
 * where it is given its sums are those of mi355rt_probes_gather on every bit.  cfg->accumulate covers the depth film as it covers `out`.  Around the call
 * mi355rt_probes_gather's rules hold; mi355rt_last_counts reports npoints * spp primary rays.
 * ERRORS.  Those of mi355rt_probes_gather (an `out` that is NULL is fine, one whose pointers are all NULL is not), and: depth NULL; res outside 2 .. 16;
 * max_distance not finite, not > 0 or > 1e12; count or moments NULL.  Nothing is written.
 *
 * VISIBILITY of one probe for v = p_b - probe position.  In this order:
 *     r = sqrt((x * x + y * y) + z * z);  r not a positive finite number (0, a NaN, an overflow to infinity): 1
 *     bilinear fetch of the texel means at (u, w) = map(v), per axis without a floor:  g = u * (float)res + 0.5f;  i1 = (uint32_t)g;  f = g - (float)i1;
 *         the two texels are i1 - 1 and i1 (signed) with weights 1 - f and f
 *     an index pair (i, j) outside [0, res - 1]^2 wraps by the octahedral rule, the x rule first and the y rule on its result:
 *         i < 0 -> (0, res-1-j);  i >= res -> (res-1, res-1-j);   then  j < 0 -> (res-1-i, 0);  j >= res -> (res-1-i, res-1)
 *     the four texels in the order (dj, di) = (0,0), (0,1), (1,0), (1,1), wt = wx * wy;  a texel with wt == 0 or count == 0 is skipped and never read into a sum;
 *         else  ws += wt;  a += wt * (m0 / (float)count);  b += wt * (m1 / (float)count)
 *     ws == 0 (no information): 1.   mean = a / ws;  mean2 = b / ws;   r <= mean: 1
 *     var = |mean2 - mean * mean|;  dd = r - mean;  c = var / (var + dd * dd);   the weight is (c * c) * c
 *
 * LOOKUP_VIS is LOOKUP of PROBES with the weight of corner j  wj = (t_j * vis) * face  in the place of t_j: in wsum += wj and in s_j = wj * (4 pi / n_j).
 *     p_b = p + normal_bias * normal (one multiply, one add per axis); without normals p_b = p.  v = p_b - probe position.
 *     vis = VISIBILITY(v) with MI355RT_VIS_CHEBYSHEV, else 1
 *     face = q * q + 0.2f with MI355RT_VIS_FACING where r is a positive finite number, else 1;  q = (dot / r + 1) * 0.5f, made 0.0001f where !(q >= 0.0001f),
 *         dot = ((-x) * nx + (-y) * ny) + (-z) * nz
 *     The cell and the trilinear fractions come from p, not p_b.  A corner with t_j == 0, n_j == 0 or usable == 0 is skipped before anything else of it is
 *     read, as in LOOKUP; a corner whose wj is 0 is skipped like them.  No corner used: rgb = 0, ok = 0.  Nothing is clamped.
 * With flags 0 and normal_bias 0 the call is mi355rt_probes_lookup on every bit: (t * 1) * 1 is t.  Around the call mi355rt_probes_lookup's rules hold.
 * ERRORS.  Those of mi355rt_probes_lookup, and: depth NULL, its res or max_distance out of range, its count or moments NULL; vc NULL; unknown flag bits; a
 * normal_bias that is not finite; MI355RT_VIS_FACING or a non-zero normal_bias with normals3 NULL.  Nothing is written.
 *
 * Host only, no handle, the same header the kernels compile (csrc/oct_vis.hpp): mi355rt_oct_encode (THE MAP), mi355rt_oct_texel (THE TEXEL: ixy = (ix, iy)),
 * mi355rt_probe_visibility_one (VISIBILITY; count and moments are the film of that one probe), mi355rt_probes_lookup_vis_one (LOOKUP_VIS of one query, *ok may
 * be NULL); the message of a refusal is in mi355rt_last_error(NULL). */
#define MI355RT_VIS_CHEBYSHEV 1u
#define MI355RT_VIS_FACING    2u
typedef struct mi355rt_probe_depth { uint32_t res; float max_distance; uint32_t* count; float* moments; } mi355rt_probe_depth;   /* 24 bytes */
typedef struct mi355rt_probe_vis_config { uint32_t flags; float normal_bias; } mi355rt_probe_vis_config;   /* 8 bytes */
void mi355rt_probes_vis_default_config(mi355rt_probe_vis_config* vc);   /* flags MI355RT_VIS_CHEBYSHEV | MI355RT_VIS_FACING, normal_bias 0 */
int  mi355rt_probes_gather_depth(mi355rt_handle* h, const float* points3, const uint32_t* ids /* NULL: i */, size_t npoints, const mi355rt_probe_config* cfg, uint32_t where,
                                 const mi355rt_probe_outputs* out /* may be NULL */, const mi355rt_probe_depth* depth);
int  mi355rt_probes_lookup_vis(mi355rt_handle* h, const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable /* may be NULL */,
                               const mi355rt_probe_depth* depth, const mi355rt_probe_vis_config* vc, const float* points3, const float* dirs3,
                               const float* normals3 /* may be NULL */, size_t npoints, uint32_t mode, uint32_t where, float* rgb3, uint8_t* ok /* may be NULL */);
int  mi355rt_oct_encode(const float dir[3], float uv[2]);
int  mi355rt_oct_texel(const float dir[3], uint32_t res, uint32_t ixy[2]);
int  mi355rt_probe_visibility_one(const mi355rt_probe_depth* depth_of_one_probe, const float v[3], float* weight);
int  mi355rt_probes_lookup_vis_one(const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable /* may be NULL */,
                                   const mi355rt_probe_depth* depth, const mi355rt_probe_vis_config* vc, const float point[3], const float dir[3],
                                   const float normal[3] /* may be NULL */, uint32_t mode, float rgb[3], uint32_t* ok /* may be NULL */);

/* SampleGenerator table, sample_generator.rs:15-24: 65 536 x 3 floats */
int mi355rt_get_sample_table(const mi355rt_handle* h, float* out);
/* Per-node direct-light terms of one primary sample, computed on the device by the same
 * kernels as a frame (stage-level parity): node_L = nodes x 3 floats (breadth-first radiance
 * tree, black where not reached), color3 = the sample's radiance.  Does not touch the film. */
int mi355rt_debug_sample(mi355rt_handle* h, uint32_t pixel, uint32_t sampleno, float color3[3], float* node_L, size_t nodes);
/* Device arithmetic self-check: quot = a/b, root = sqrt(a), pow32 = a^32 computed exactly as the
 * kernels compute them (IEEE division and square root; powf(x, 32.0) of mod.rs:255). */
int mi355rt_debug_numerics(mi355rt_handle* h, const float* a, const float* b, size_t n, float* quot, float* root, float* pow32);
/* intersect_cube_inverse_ray, oct_tree_intersector.rs:348-372, exactly as the reference-exact intersector runs it
 * on the device: inv_rays6 = n x (origin3, 1/dir3), cubes6 = n x (min3, max3); hit[i] = 1 iff the slab test
 * passes, tmin[i] = the entry distance it returns (negative when the origin is inside).  Exists so that the
 * reference's own known-answer vectors (oct_tree_intersector.rs:475-512) run through the HIP path. */
int mi355rt_debug_slab(mi355rt_handle* h, const float* inv_rays6, const float* cubes6, size_t n, uint8_t* hit, float* tmin);
uint32_t mi355rt_tree_nodes(const mi355rt_handle* h);
/* Speculation of the drop-in loop: out[0] = 50-row frames launched ahead of the call that asks for them, out[1] = how many of those the next
 * mi355rt_trace_frame_additive call took over (the others were given back: the caller did something else first).  Test hook; device 0 of a group. */
int mi355rt_debug_speculation(const mi355rt_handle* h, uint64_t out[2]);
/* The depth cube map the library builds around a point light (csrc/lightmap.hpp; what lets the shade kernels leave out the shadow rays of
 * mod.rs:224-232 whose way to the light is provably free).  HOST code, no device needed: out_dist2[6 * res * res] receives, per direction texel
 * (face = 2 * major axis + (component negative), then i over the lower and j over the higher of the two other axes), a lower bound of the squared
 * distance from `light` to any of the ntri triangles (tri_verts: ntri x 9 floats) padded by `pad`, +inf where no triangle is seen; *nearest the
 * distance to the nearest triangle.  Exists so that the bound can be checked against brute force without a GPU. */
int mi355rt_debug_light_map(const float* tri_verts, uint32_t ntri, const float light[3], double pad, uint32_t res, float* out_dist2, double* nearest);
/* The reflection masks the library builds per triangle (host code, no device needed): out_words receives ntri records of info[0] 32-bit words — 6 * bins^2
 * direction bits (face-major cube map, a SET bit means "trace"), then v0.xyz and the guard's height margin as f32 bits; NULL: only info is filled.
 * info: [0] words per triangle, [1] build ms, [2] work units, [3] clear bits, [4] minimum cosine, [5] angular pad, [6] barycentric guard margin,
 * [7] 1 when a mask was built (0: over work_budget, or no triangles).  work_budget 0: unlimited.  On ENTRY info[4] and info[5] choose the minimum cosine and
 * the angular pad to build with (0: the library's own; other values serve the census of the margins only — the kernels know the shipped ones). */
int mi355rt_debug_reflect_mask(const float* tri_verts, uint32_t ntri, double pad, uint32_t bins, uint64_t work_budget, uint32_t* out_words, double info[8]);

/* Test hook (host only, no device): the 4-wide tree of 48-byte nodes that experiment builds of the kernels walk (-DMI355RT_WIDE=1; bvh.hpp,
 * BvhNode4: 8-bit child boxes in a per-node frame), built from the ntri triangles like mi355rt_create builds the binary tree, then checked by a
 * walk that decodes the node words the way the kernels do.  out[0] wide nodes (0: the format does not serve this scene), [1] binary nodes,
 * [2] most deferred children of any walk (stack rows), [3] binary depth, [4] child slots in use, [5] triangles the walk of the wide tree reaches
 * exactly once, [6] child boxes that fail to contain a vertex of a triangle below them (must be 0), [7] triangles the re-pointed binary tree
 * reaches exactly once. */
int mi355rt_debug_wide_bvh(const float* tri_verts, uint32_t ntri, uint32_t out[8]);
/* Test hook (host only, no device, no handle): the reference's octree exactly as mi355rt_create builds it for the default intersector
 * (csrc/octree.hpp; the same build_octree call on the ntri triangles with tris_per_leaf), in its flat form by node index.  counts[8] receives what
 * mi355rt_octree_stats reports for that tree ([0] nodes .. [5] triangle references).  SIZE QUERY: all six arrays NULL; only counts is written.
 * Otherwise all six are required: cubes6 holds node_cap x (min3, max3); first_child, tri_first, tri_count and parent node_cap entries (first_child
 * >= 0: inner node with the children first_child .. first_child + 7, -1: leaf with the range tri_first, tri_count of leaf_tris; parent of the root: 0);
 * leaf_tris leaf_cap global triangle indices, the leaves' lists in list order.  node_cap < counts[0] or leaf_cap < counts[5]: MI355RT_E_INVALID and
 * nothing is written, not counts either.  Exists so that the build can be held to an independent statement without a GPU. */
int mi355rt_debug_octree(const float* tri_verts, uint32_t ntri, uint32_t tris_per_leaf, uint32_t counts[8], float* cubes6, int32_t* first_child,
                         uint32_t* tri_first, uint32_t* tri_count, uint32_t* parent, size_t node_cap, uint32_t* leaf_tris, size_t leaf_cap);
/* Test hook: the binary BVH itself, word for word (csrc/bvh.hpp: BvhNode is 8 words { h0[3], child0, h1[3], child1 }, BvhTri 12 words
 * { v0[3], prim, e1[3], geom, e2[3], pad }).  TWO SOURCES.  With a handle: the handle's host copy of the tree its kernels were given, whichever builder
 * made it (the device build of MI355RT_FLAG_DEVICE_LBVH, or the host build); tri_verts, tri_geom and ntri are ignored.  In a library whose kernels walk
 * the 4-wide tree the triangles are in that tree's order.  With h == NULL: host code, no device needed — the host build (build_bvh) of the ntri triangles
 * in tri_verts (ntri x 9 floats) with tri_geom (ntri indices; NULL: all 0), exactly as mi355rt_create runs it, MI355RT_BVH_OPT included.
 * info receives [0] nodes, [1] triangle slots, [2] root (an int32: a node index, or a leaf code when the scene is one leaf), [3] leaves, [4] max_depth,
 * [5] max_leaf, [6] [7] 0; bounds6 (may be NULL) scene_min then scene_max.  SIZE QUERY: nodes8 and tris12 both NULL; only info and bounds6 are written.
 * Otherwise both are required: nodes8 holds node_cap x 8 words, tris12 tri_cap x 12.  node_cap < info[0] or tri_cap < info[1]: MI355RT_E_INVALID and
 * nothing is written, not info either.  Exists so that the tree a kernel built can be held to an independent statement, node for node. */
int mi355rt_debug_bvh_read(const mi355rt_handle* h, const float* tri_verts, const uint32_t* tri_geom, uint32_t ntri, uint32_t info[8], float* bounds6,
                           uint32_t* nodes8, size_t node_cap, uint32_t* tris12, size_t tri_cap);

/* acceleration-structure facts: out[0] nodes, [1] leaves, [2] max depth, [3] max leaf size,
 * [4] node bytes, [5] triangle bytes, [6] BVH build time inside create (wall, microseconds; host SAH build, or the device
 * build with its uploads and read-back), [7] host octree build time inside create (microseconds; 0 with
 * MI355RT_FLAG_TRUE_CLOSEST_HIT) */
int mi355rt_accel_stats(const mi355rt_handle* h, uint32_t out[8]);
/* The direction masks that prove reflection rays free (one per triangle, built inside create): out[0] bins per cube-face edge (0: no mask — switched off
 * with MI355RT_NO_REFLECT_MASK, over the work budget MI355RT_REFLECT_MASK_WORK, or recursions == 0), [1] build time in ms, [2] share of clear bits, [3] bytes. */
int mi355rt_reflect_mask_info(const mi355rt_handle* h, double out[4]);
/* MI355RT_FLAG_COUNT_STEPS: the rays the trace launches of the last call took from their queues — primary rays that walk the tree, reflection rays and
 * shadow rays that were actually made (bounce - bounce_skipped, shadow - shadow_skipped), counted by the trace kernels themselves. */
int mi355rt_debug_rays_read(const mi355rt_handle* h, uint64_t* out);
/* which builder made the BVH: out[0] 1 = the device (MI355RT_FLAG_DEVICE_LBVH served the scene), 0 = the host;
 * out[1] device time of the build kernels + sort (HIP events, microseconds; 0 for a host build) */
int mi355rt_bvh_build_info(const mi355rt_handle* h, uint32_t out[2]);
/* the reference's octree (absent with MI355RT_FLAG_TRUE_CLOSEST_HIT): out[0] octree nodes, [1] inner, [2] leaves, [3] empty leaves, [4] depth,
 * [5] triangle references (the quantities of SURVEY.md 6.2) */
int mi355rt_octree_stats(const mi355rt_handle* h, uint32_t out[8]);
/* devices of the handle's group (1 for an ordinary handle) */
uint32_t mi355rt_device_count(const mi355rt_handle* h);
/* measurement hook behind bench.py's roofline (no reference counterpart): the rate at which the device's vector memory pipe serves
 * the trace kernels' kind of fetch and nothing else — every lane of 8 waves per SIMD walks `steps` random 32-byte nodes of an
 * L2-resident table of table_nodes nodes with two 16-byte loads per node (profiles/r03_notes.md).  out[0] cache-line accesses per
 * second (one per lane and load), out[1] kernel time in ms, out[2] node fetches per second. */
int mi355rt_debug_gather_rate(mi355rt_handle* h, uint32_t table_nodes, uint32_t steps, double out[3]);
/* test hook: with MI355RT_DEBUG_GUARD set in the environment every pass buffer is allocated with a 256-byte tail of 0xA5;
 * this returns how many of those bytes a launch has overwritten (0 = nothing wrote past a buffer; -1: error) */
int64_t mi355rt_debug_check_guards(mi355rt_handle* h);
/* device memory (HBM) the handle holds right now, summed over its devices: scene + acceleration structures + film + the
 * pass buffers of the largest pass rendered so far + gather slots */
uint64_t mi355rt_hbm_allocated_bytes(const mi355rt_handle* h);
/* wait until everything queued on the handle (50-row frames, gathers) has finished on its device(s) */
int mi355rt_synchronize(mi355rt_handle* h);

/* ---- one process per GPU: the framebuffer gather over RCCL / xGMI (no reference counterpart: the reference is
 * one process on one CPU).  Every process creates its handle with stripe_rank / stripe_world = its rank / the
 * number of processes.  Rank 0 obtains a 128-byte id (ncclUniqueId) with mi355rt_comm_unique_id and hands it to the
 * others by whatever means the host application has; then ALL ranks call mi355rt_comm_init (collective).
 * mi355rt_comm_gather_frame (collective) maps every rank's rows to packed u32 and moves them to `root` with grouped
 * ncclSend / ncclRecv on the handle's stream; the root places them into its frame.  host_out (root only, may be
 * NULL): width*height u32 copied out after a synchronisation; with NULL the call only queues the work
 * (mi355rt_synchronize waits for it).  librccl.so is loaded on first use. */
#define MI355RT_COMM_ID_BYTES 128
int mi355rt_comm_unique_id(uint8_t* id128);
/* local, communication-free pre-check of mi355rt_comm_init (librccl.so loadable with every symbol, device bindable, no live
 * communicator): the ranks should agree on this BEFORE any of them enters the collective mi355rt_comm_init, so that nobody
 * blocks inside RCCL's bootstrap waiting for a rank that cannot join */
int mi355rt_comm_available(mi355rt_handle* h);
int mi355rt_comm_init(mi355rt_handle* h, const uint8_t* id128);
int mi355rt_comm_gather_frame(mi355rt_handle* h, uint32_t root, uint32_t* host_out, size_t n);
int mi355rt_comm_destroy(mi355rt_handle* h);
/* ranks of the handle's live communicator as RCCL counts them (ncclCommCount; 0: no communicator, or it is not the one
 * this handle's stripe_rank was dealt into) */
uint32_t mi355rt_comm_ranks(mi355rt_handle* h);

uint32_t mi355rt_width(const mi355rt_handle* h);
uint32_t mi355rt_light_count(const mi355rt_handle* h);     /* lights of the handle's scene: nlights of the LIGHT FILMS entries */
uint32_t mi355rt_height(const mi355rt_handle* h);
uint32_t mi355rt_triangle_count(const mi355rt_handle* h);
uint32_t mi355rt_current_row(const mi355rt_handle* h);

/* ---- PROBE PLACEMENT: what a probe sees around itself, where it moves, the state it gets, and a lookup that knows the moves (no reference counterpart;
 * DESIGN.md §3q).  A probe that stands inside or against geometry is moved a fraction of a cell into free space, and what cannot be saved is marked.  A moved
 * probe is gathered with the existing entries at grid point + offset (one f32 addition per component).  raytracer-rs_amd/probes.py states all of it.
 * Everything is f32, unfused, in the order written, with + - * / sqrt, comparisons and integer conversions only.
 *
 * SURVEY.  The samples, keys and rays are mi355rt_probes_gather's (sphere mode), but only their CLOSEST HITS are taken: the rays of a chunk are traced with the
 * launch of mi355rt_intersect_rays, no bounce and no shadow ray is made, and mi355rt_last_counts reports npoints * spp primary rays and nothing else.
 * A sample is a HIT when its prim is not MISS and its t is a positive finite number, otherwise a miss.  A hit is a BACK hit when
 * (d.x * N.x + d.y * N.y) + d.z * N.z > 0, d the ray's direction as given and N the normal of the hit triangle (normalised cross(v1 - v0, v2 - v0), as the
 * feature film has it), negated with MI355RT_SURVEY_FLIP; otherwise, and with a NaN dot, a FRONT hit.  Per point, in sample order, with D = max_distance:
 *     n += 1
 *     back hit:   back += 1;   t < near_back.dist:  near_back = (t, d)
 *     front hit:  front += 1;  t < near_front.dist: near_front = (t, d);   dist = t < D ? t : D;   dist > far.dist: far = (dist, d)
 *     miss:       dist = D;    dist > far.dist: far = (D, d)
 * A record is four floats (dist, d.x, d.y, d.z) and is replaced on a strict comparison only: of samples at the same distance the first keeps it.  An empty
 * near record is (+inf, 0, 0, 0), an empty far (-inf, 0, 0, 0).  n, back, front are npoints u32, near_back, near_front, far npoints x 4 f32.  accumulate != 0:
 * the six arrays are read, continued and written back, so survey(3) followed by survey(5, first_sample 3, accumulate) is survey(8) bit for bit; otherwise they
 * start empty.  Around the call mi355rt_probes_gather's rules hold.  Device arrays of records must be 16-byte aligned.
 * ERRORS.  Those of mi355rt_probes_gather, and: out NULL or any of its six pointers NULL; unknown flag bits; max_distance not finite, not > 0 or > 1e12; with
 * MI355RT_RAYS_DEVICE a record array that is not 16-byte aligned.  Nothing is written.
 *
 * PLACE.  Per probe, from its survey, its offset (relative to its grid point; offsets NULL: zero) and the config; share = (float)back / (float)n.
 *     n == 0:                                                    no candidate                                                  MI355RT_PLACE_UNSAMPLED
 *     share > back_share and near_back.dist < +inf:              len = near_back.dist + 0.5f * min_front;  c_a = o_a + nb.d_a * len      MI355RT_PLACE_THROUGH
 *     else near_front.dist < +inf and near_front.dist < min_front:
 *         dot = (nf.x * far.x + nf.y * far.y) + nf.z * far.z;  ln = sqrt((nf.x * nf.x + nf.y * nf.y) + nf.z * nf.z);  lf likewise of far's direction
 *         dot <= (0.5f * ln) * lf:   m = far.dist < min_front ? far.dist : min_front;  c_a = o_a + (far.d_a * m) / lf                    MI355RT_PLACE_AWAY
 *         otherwise:                 no candidate                                                                                      MI355RT_PLACE_STAY
 *     else an offset component != 0:  lo = sqrt((o.x * o.x + o.y * o.y) + o.z * o.z);  room = near_front.dist - min_front
 *         near_front.dist < +inf and room < lo:  c_a = o_a + ((-o_a) * room) / lo;   otherwise c = (0, 0, 0), the whole way                MI355RT_PLACE_BACK
 *     else:                                                      no candidate                                                  MI355RT_PLACE_REST
 * The candidate is accepted, and becomes the new offset, only if every component satisfies |c_a| < max_offset * spacing_a or c_a == 0, where an axis with one
 * probe has spacing 0.  A component that is not finite fails both, so an overflow or a NaN on the way refuses the candidate.  A refused candidate leaves the
 * offset as it was and sets MI355RT_PLACE_REFUSED in the verdict, which otherwise is the branch above.
 * STATE of a probe: n == 0: MI355RT_PROBE_UNKNOWN; share > back_share: BURIED; !(near_front.dist < max_distance) (no front hit within reach, nothing there to
 * light): IDLE; else ACTIVE.  max_distance is the survey's.  ACTIVE and IDLE probes are usable in a lookup.
 * mi355rt_probes_place computes new_offsets (nprobes x 3 f32; may be `offsets` itself), verdict and state (nprobes u8 each) for the nprobes = counts product
 * probes of the grid; any of the three may be NULL, not all.  It traces nothing; mi355rt_probes_lookup's rules hold around it.  back_share 0.25 and max_offset
 * 0.45 are the published DDGI values; min_front has no default (a fifth of the smallest spacing is the usual choice).
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: a device group; an unknown where; the grid errors of
 * mi355rt_probes_lookup; survey NULL or any of its pointers NULL; cfg NULL; back_share not in [0, 1]; max_offset not finite or < 0; min_front not finite and
 * > 0 (when new_offsets or verdict is asked for); max_distance out of SURVEY's range (when state is asked for); all three outputs NULL; a host `offsets` that
 * holds a non-finite value; with MI355RT_RAYS_DEVICE a record array that is not 16-byte aligned (device offsets are not inspected: they are data).
 *
 * LOOKUP_PLACED is LOOKUP_VIS of PROBE VISIBILITY with offsets (nprobes x 3 f32): the probe position that enters v = p_b - position is
 * (origin_a + (float)i_a * spacing_a) + offset_a.  The cell, the fractions and the trilinear factor still come from the grid.  offsets NULL is
 * mi355rt_probes_lookup_vis on every bit; with flags 0 no position is made, the offsets are not read, and the call is mi355rt_probes_lookup on every bit.
 * ERRORS.  Those of mi355rt_probes_lookup_vis, and a host `offsets` that holds a non-finite value.  Offsets in device memory are not inspected: they are used
 * as data, and a non-finite one makes the weights of its probe what the arithmetic above makes of it.
 *
 * Host only, no handle, the same header the kernels compile (csrc/probe_place.hpp): mi355rt_probe_place_one (PLACE and STATE of one probe: counts3 = (n, back,
 * front), records12 = near_back, near_front, far; new_offset, verdict and state may each be NULL), mi355rt_probes_lookup_placed_one (LOOKUP_PLACED of one
 * query); the message of a refusal is in mi355rt_last_error(NULL). */
#define MI355RT_SURVEY_FLIP     1u
#define MI355RT_PROBE_UNKNOWN   0u
#define MI355RT_PROBE_BURIED    1u
#define MI355RT_PROBE_IDLE      2u
#define MI355RT_PROBE_ACTIVE    3u
#define MI355RT_PLACE_UNSAMPLED 0u
#define MI355RT_PLACE_THROUGH   1u
#define MI355RT_PLACE_AWAY      2u
#define MI355RT_PLACE_STAY      3u
#define MI355RT_PLACE_BACK      4u
#define MI355RT_PLACE_REST      5u
#define MI355RT_PLACE_REFUSED   8u
typedef struct mi355rt_probe_survey_config { uint32_t spp, first_sample, accumulate, flags; float max_distance; } mi355rt_probe_survey_config;   /* 20 bytes */
typedef struct mi355rt_probe_survey { uint32_t *n, *back, *front; float *near_back, *near_front, *far; } mi355rt_probe_survey;   /* 48 bytes; records: npoints x 4 */
typedef struct mi355rt_probe_place_config { float back_share, max_offset, min_front, max_distance; } mi355rt_probe_place_config;   /* 16 bytes */
void mi355rt_probes_survey_default_config(mi355rt_probe_survey_config* cfg);   /* spp 64, first_sample 0, accumulate 0, flags 0; max_distance 0: to be set */
void mi355rt_probes_place_default_config(mi355rt_probe_place_config* cfg);     /* back_share 0.25, max_offset 0.45; min_front 0 and max_distance 0: to be set */
int  mi355rt_probes_survey(mi355rt_handle* h, const float* points3, const uint32_t* ids /* NULL: i */, size_t npoints, const mi355rt_probe_survey_config* cfg, uint32_t where,
                           const mi355rt_probe_survey* out);
int  mi355rt_probes_place(mi355rt_handle* h, const mi355rt_probe_grid* grid, const mi355rt_probe_survey* survey, const mi355rt_probe_place_config* cfg,
                          const float* offsets /* may be NULL: zero */, uint32_t where, float* new_offsets /* may be NULL */, uint8_t* verdict /* may be NULL */,
                          uint8_t* state /* may be NULL */);
int  mi355rt_probe_place_one(const mi355rt_probe_grid* grid, const mi355rt_probe_place_config* cfg, const uint32_t counts3[3], const float records12[12],
                             const float offset[3] /* may be NULL: zero */, float new_offset[3], uint32_t* verdict, uint32_t* state);
int  mi355rt_probes_lookup_placed(mi355rt_handle* h, const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable /* may be NULL */,
                                  const mi355rt_probe_depth* depth, const mi355rt_probe_vis_config* vc, const float* offsets /* may be NULL */, const float* points3,
                                  const float* dirs3, const float* normals3 /* may be NULL */, size_t npoints, uint32_t mode, uint32_t where, float* rgb3,
                                  uint8_t* ok /* may be NULL */);
int  mi355rt_probes_lookup_placed_one(const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable /* may be NULL */,
                                      const mi355rt_probe_depth* depth, const mi355rt_probe_vis_config* vc, const float* offsets /* may be NULL */, const float point[3],
                                      const float dir[3], const float normal[3] /* may be NULL */, uint32_t mode, float rgb[3], uint32_t* ok /* may be NULL */);

/* ---- PROBE-LIT: the radiance along caller-given rays with the whole bounce tree replaced by one lookup in a probe volume, and that lookup at caller-given
 * surface points.  The reference's compute_radiance (mod.rs:132-176) returns shade() + (1 / num_sub) * sum of the children's radiance: the
 * bounce term is the UNIFORM mean of the radiance arriving over the hemisphere of the triangle normal — not cosine-weighted, not multiplied by albedo; what
 * mi355rt_gather estimates under MI355RT_GATHER_MEAN.  For a field given as SH coefficients that mean is a zonal convolution with the band factors 1, 1/2, 0,
 * so only coefficients 0 .. 3 of a probe are read.  raytracer-rs_amd/probe_lit.py states all of it in numpy; everything is f32, unfused, in the order written.
 *
 * A VOLUME is what mi355rt_probes_lookup_placed takes of a grid: grid, n, sh, optional usable, optional depth with vc, optional offsets.  With depth NULL, vc
 * and offsets must be NULL too, and the corner weights are LOOKUP's t_j.
 *
 * HEMI, the hemisphere mean at a point p with normal N (used as given).  The corners, their skipping rules, wsum and the weight w_j = (t_j * vis) * face are
 * exactly those of LOOKUP_PLACED for (p, dir = N, normal = N) (of LOOKUP without depth).  Per used corner, in j order from +0.0f:
 *     s_j = w_j * (12.566370614f / (float)n_j);   C[k][c] += s_j * sh_j[k][c]   for k = 0 .. 3 only   (coefficients 4 .. 8 are never read)
 *     m_c = ((C[0][c] * b_0 + (0.5f * C[1][c]) * b_1(N)) + (0.5f * C[2][c]) * b_2(N)) + (0.5f * C[3][c]) * b_3(N)     (THE BASIS; the sum from +0.0f in k order)
 *     x_c = m_c / wsum;   indirect_c = x_c >= 0.0f ? x_c : 0.0f with MI355RT_PROBE_LIT_CLAMP (a NaN becomes 0), x_c without;   ok = 1
 * No corner used: indirect = 0, ok = 0.  A band-1 mean can ring below zero next to a strong light: hence the clamp.
 *
 * SHADE, the reference's shade() (mod.rs:207-261) at a hit of ray (pos, dir) at (t, u, v) of triangle prim: P = pos + t * dir (one multiply and one add per
 * axis); N the triangle's normal and the diffuse colour as the feature film has them.  Per light, in scene order, from +0.0f: l = light - P, ln = normalized(l),
 * ndl = dot(N, ln); ndl < 0: skipped; the shadow ray (P + l * 0.01f, l) blocked by the rule of mi355rt_occluded_rays: skipped; otherwise
 * refl = (2 * ndl) * N - ln, spec = pow32(dot(normalized(dir), refl)) (five squarings in f64, one rounding), light += (diffuse * ndl + spec) * colour.
 * This is the root light sum: `direct` of mi355rt_trace_rays for the same ray, bit for bit.
 *
 * mi355rt_probe_lit_rays, per ray: (tuv, prim) is what mi355rt_intersect_rays gives in the handle's semantics.  A miss: rgb = light = indirect = 0, ok = 0,
 * prim MISS, tuv untouched.  A hit: light = SHADE, (indirect, ok) = HEMI at (P, N) with N NOT flipped towards the viewer (the reference's bounce rays go to
 * the normal's side, whichever side the ray came from), rgb_c = light_c + indirect_c.  Any output may be NULL, not all; every subset gives the same bits.
 * Around the call mi355rt_probes_survey's rules hold: a queued or speculative frame is settled first; films, camera, lens, current row and guides are
 * untouched; a striped handle serves it; mi355rt_last_counts reports nrays primary rays, no bounce ray — and, as for `direct` of mi355rt_gather, NO shadow
 * ray: the shadow rays go through the launch of mi355rt_occluded_rays, which counts nothing.  shade()'s light maps are not consulted: every (hit, light) pair
 * is traced.  The rays run in chunks of at most min(pass samples, 4 Mi / max(nlights, 1)); the chunk temporaries (16 + 25 * nlights bytes per ray) are freed
 * by the end of the call.
 * mi355rt_probe_lit_points: HEMI at npoints caller-given points and normals.  It traces nothing; mi355rt_probes_lookup's rules hold around it.
 * `where` covers every pointer of a call, the volume's arrays included (the struct itself is host memory).
 * ERRORS.  MI355RT_E_INVALID, the argument named in mi355rt_last_error and nothing written, for: a device group; an unknown where; volume NULL; everything
 * mi355rt_probes_lookup_placed refuses of the volume's members; depth NULL with vc or offsets given; unknown flag bits; out NULL or all its pointers NULL
 * (indirect3 NULL); NULL rays6, points3 or normals3 with a non-zero count; nrays * max(nlights, 1) >= 2^32; host offsets that hold a non-finite value.  A
 * count of 0 succeeds and writes nothing.
 * Host only, no handle, the same header the kernels compile (csrc/probe_lit_math.hpp): mi355rt_probe_lit_one (HEMI of one query); the message of a refusal is
 * in mi355rt_last_error(NULL). */
#define MI355RT_PROBE_LIT_CLAMP 1u
typedef struct mi355rt_probe_volume { const mi355rt_probe_grid* grid; const uint32_t* n; const float* sh; const uint8_t* usable /* may be NULL */;
    const mi355rt_probe_depth* depth /* may be NULL */; const mi355rt_probe_vis_config* vc /* NULL iff depth is */; const float* offsets /* may be NULL; NULL if depth is */; } mi355rt_probe_volume;  /* 56 bytes */
typedef struct mi355rt_probe_lit_outputs { float *rgb, *light, *indirect, *tuv; uint32_t* prim; uint8_t* ok; } mi355rt_probe_lit_outputs;  /* 48 bytes; any may be NULL, not all */
int  mi355rt_probe_lit_points(mi355rt_handle* h, const mi355rt_probe_volume* volume, const float* points3, const float* normals3, size_t npoints, uint32_t flags, uint32_t where,
                              float* indirect3, uint8_t* ok /* may be NULL */);
int  mi355rt_probe_lit_rays(mi355rt_handle* h, const mi355rt_probe_volume* volume, const float* rays6, size_t nrays, uint32_t flags, uint32_t where,
                            const mi355rt_probe_lit_outputs* out);
int  mi355rt_probe_lit_one(const mi355rt_probe_volume* volume, const float point[3], const float normal[3], uint32_t flags, float indirect[3], uint32_t* ok /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MI355RT_H */
