// kernels.hpp — host-callable launchers of kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "device_types.hpp"

namespace mi355rt {

hipError_t launch_trace(hipStream_t stream, int num_cus, bool primary, bool count, bool confirm, const DScene& sc, const DCamera& cam, const DPass& ps,
                        const void* in_q, const void* in_counts, void* hits, uint32_t* cursor,
                        float* slot_L, const uint32_t* film_n, DCounters* counters, uint32_t rays = kFeedCamera);   // rays: the feed of the primary round, a kFeed* of device_types.hpp
// culling verdicts of the pass's pixel blocks (DPass::block_culled): out[b] = chunk b (first sample group) is culled
hipError_t launch_cull_blocks(hipStream_t stream, const DCamera& cam, const DPass& ps, uint32_t nblocks, uint32_t* out);
hipError_t launch_trace_octree(hipStream_t stream, int num_cus, bool primary, const DScene& sc, const DCamera& cam, const DPass& ps,
                               const void* in_q, const void* in_counts, void* hits, float* slot_L, const uint32_t* film_n, uint32_t rays = kFeedCamera);
hipError_t launch_shade(hipStream_t stream, int num_cus, bool primary, bool walk, const DScene& sc, const DCamera& cam, const DPass& ps, uint32_t level,
                        const void* in_q, const void* in_counts, const void* hits, void* out_q, void* out_counts, uint32_t* cursor,
                        float* slot_L, uint32_t* sample_slot, const uint32_t* film_n, DCounters* counters, bool raster = false,   // raster: primary round, hits through the tile bins inside the launch
                        uint32_t rays = kFeedCamera);                                                                              // rays: as launch_trace
hipError_t launch_resolve(hipStream_t stream, const DPass& ps, uint32_t width, uint32_t nlights, const float* slot_L, const uint32_t* sample_slot,
                          float* film_sum, float* film_sumsq, uint32_t* film_n, float* film_direct, float* debug_color, uint32_t* ctrl,    // ctrl != null: zero the pass's work cursors on the way out
                          float* film_lights = nullptr, uint32_t lights_stride = 0);   // film_lights: the light films (below), null without MI355RT_FLAG_LIGHT_FILMS: the kernels without them
// mi355rt_trace_rays: per-ray results of a ray-fed pass whose sample i is ray i; rgb / direct / tuv / prim: the pass's part of the outputs, any may be null
hipError_t launch_resolve_rays(hipStream_t stream, const DPass& ps, uint32_t nlights, const float* slot_L, const uint32_t* sample_slot,
                               float* rgb, float* direct, float* tuv, uint32_t* prim, uint32_t* ctrl);
// film_direct (here and below): the handle's direct film (MI355RT_FLAG_DIRECT_FILM), null without the flag: the kernels of a three-plane film
// one 50-row frame (1 sample per pixel) in a single launch: every wave takes a 64-sample chunk through all rounds
bool kernels_walk_wide_nodes();      // this build's trace loops read BvhNode4 slots (MI355RT_WIDE), not BvhNode
uint32_t fused_pass_lds_rows(uint32_t stack_depth, uint32_t max_level_nodes, uint32_t records_per_sample);
// reference-default semantics: true closest hits of a round -> the octree intersector's answers (+ the shadow predicate)
hipError_t launch_confirm(hipStream_t stream, int num_cus, bool primary, bool shadow_only, const DScene& sc, const DCamera& cam, const DPass& ps,
                          const void* in_q, const void* in_counts, void* hits, uint32_t* cursor, float* slot_L, const uint32_t* film_n);
hipError_t launch_fused_pass(hipStream_t stream, int num_cus, bool confirm, const DScene& sc, const DCamera& cam, const DPass& ps, uint32_t max_level_nodes, uint32_t records_per_sample,
                             void* q0, void* q1, void* hits, float* slot_L, uint32_t* sample_slot,
                             float* film_sum, float* film_sumsq, uint32_t* film_n, float* film_direct, DCounters* counters);
// rows == null: the contiguous rows row_base .. row_base + nrows - 1
hipError_t launch_tonemap(hipStream_t stream, const uint32_t* rows, uint32_t row_base, uint32_t nrows, uint32_t width, bool packed,
                          const float* film_sum, const uint32_t* film_n, uint32_t* out);
hipError_t launch_intersect(hipStream_t stream, const DScene& sc, uint32_t stack_depth, int mode, const float* rays6, uint32_t n, bool shadow_mode,
                            float* tuv, uint32_t* prim, uint8_t* blocked);
// multi-GPU gather on the root: world slots of slot_rows packed rows each -> full frame
hipError_t launch_place_stripes(hipStream_t stream, const uint32_t* gathered, uint32_t* frame, uint32_t width, uint32_t height,
                                uint32_t stripe_rows, uint32_t world, uint32_t slot_rows);
// Film::clear restricted to the listed rows (a striped handle's own rows)
hipError_t launch_film_clear_rows(hipStream_t stream, const uint32_t* rows, uint32_t nrows, uint32_t width, float* film_sum, float* film_sumsq, uint32_t* film_n, float* film_direct);
// film entries of `total` rows of the owned-row list (cyclic from entry `first`) -> packed backup, or back
hipError_t launch_film_rows_copy(hipStream_t stream, const uint32_t* rows, uint32_t first, uint32_t total, uint32_t nown, uint32_t width,
                                 float* film_sum, float* film_sumsq, uint32_t* film_n, float* film_direct,
                                 float* bk_sum, float* bk_sumsq, uint32_t* bk_n, float* bk_direct, bool restore);
// mi355rt_film_set / mi355rt_film_add: the staged planes (device memory; in_sum / in_sumsq / in_direct npix * 3 floats, in_n npix) stored
// (add == false: bits unchanged) or added (film + in) into the rows with (row / stripe_rows) % stripe_world == stripe_rank; the other rows are not written
hipError_t launch_film_merge(hipStream_t stream, bool add, const float* in_sum, const float* in_sumsq, const uint32_t* in_n, const float* in_direct,
                             uint32_t npix, uint32_t width, uint32_t stripe_rows, uint32_t stripe_world, uint32_t stripe_rank,
                             float* film_sum, float* film_sumsq, uint32_t* film_n, float* film_direct);
constexpr uint32_t kMaxLightFilms = 8;      // MI355RT_LIGHT_FILMS_MAX_LIGHTS: the planes resolve_kernel keeps running sums for (LDS)
// light films (MI355RT_FLAG_LIGHT_FILMS): nlights planes of lights_stride == 3 * width * height floats, each laid out like film_sum
hipError_t launch_light_films_clear_rows(hipStream_t stream, const uint32_t* rows, uint32_t nrows, uint32_t width, uint32_t nlights, float* film_lights, uint32_t lights_stride);
// mi355rt_light_films_set / _add: as launch_film_merge, `in` laid out like film_lights (device memory)
hipError_t launch_light_films_merge(hipStream_t stream, bool add, const float* in, uint32_t nlights, uint32_t npix, uint32_t width,
                                    uint32_t stripe_rows, uint32_t stripe_world, uint32_t stripe_rank, float* film_lights, uint32_t lights_stride);
// mi355rt_get_relit_pixels: rgb[p] = sum over the lights of weights[li] * (light[li][p] / n[p]); weights: nlights * 3 floats on the device
hipError_t launch_relit(hipStream_t stream, uint32_t npix, uint32_t nlights, const float* film_lights, uint32_t lights_stride, const uint32_t* film_n, const float* weights, float* rgb);
hipError_t launch_slab(hipStream_t stream, const float* inv_rays6, const float* cubes6, uint32_t n, uint8_t* hit, float* tmin);
// adaptive sampling: out[tile] = the tile is active; *count (zeroed by the caller) += (owned pixels << 32) | 1 per active tile
hipError_t launch_adaptive_tiles(hipStream_t stream, const AdaptiveArgs& a, const float* film_sum, const float* film_sumsq, const uint32_t* film_n,
                                 uint8_t* out, unsigned long long* count);
hipError_t launch_film_stat(hipStream_t stream, bool variances, size_t npix, const float* film_sum, const float* film_sumsq, const uint32_t* film_n, float* out);
// denoised read-out: the guides of the camera cam (cam.width x cam.height pixels; flags bit 0: FIX_ROW_INDEX), mode as launch_intersect
hipError_t launch_guides(hipStream_t stream, const DScene& sc, const DCamera& cam, uint32_t flags, uint32_t stack_depth, int mode, float4* g0, float4* g1);   // cam.lens: whose centre rays
// mi355rt_lens_rays: the rays of the next render(spp) under cam.lens, width * height * spp x (pos3, dir3) in mi355rt_render_rays layout, device memory
hipError_t launch_lens_rays(hipStream_t stream, const DCamera& cam, uint32_t flags, uint32_t seed, uint32_t spp, const uint32_t* film_n, float* rays6);
// gather.  A chunk: cp points from point0 on x cs samples numbered from `first` on, entry s * cp + i; every pointer is device memory, points /
// normals / ids / out_* the caller's whole arrays, the rest chunk buffers.  launch_gather_rays: the rays (6 floats), keys (2 words) and validity bytes of the chunk
hipError_t launch_gather_rays(hipStream_t stream, const DScene& sc, uint32_t seed, const float* points, const float* normals, const uint32_t* ids,
                              uint32_t point0, uint32_t cp, uint32_t cs, uint32_t first, float* rays6, uint32_t* keys2, uint8_t* valid);
// per point the chunk's samples in order into n / hits / near / sum / sumsq (any may be null; fresh: they start from 0); weight: MI355RT_GATHER_*; rgb (read for
// sum / sumsq) and tuv / prim (read for hits / near): the results of the chunk's ray-fed pass
hipError_t launch_gather_reduce(hipStream_t stream, uint32_t point0, uint32_t cp, uint32_t cs, uint32_t weight, bool fresh, float near_distance, const float* normals,
                                const float* rays6, const uint8_t* valid, const float* rgb, const float* tuv, const uint32_t* prim,
                                uint32_t* out_n, uint32_t* out_hits, uint32_t* out_near, float* out_sum, float* out_sumsq);
// `direct`: the shadow rays of cp points x sc.nlights lights (entry li * cp + i) for launch_intersect's shadow mode, then the sum over the lights per point
hipError_t launch_gather_shadow_rays(hipStream_t stream, const DScene& sc, const float* points, uint32_t point0, uint32_t cp, float* rays6);
hipError_t launch_gather_direct(hipStream_t stream, const DScene& sc, const float* points, const float* normals, uint32_t point0, uint32_t cp, const uint8_t* blocked, float* direct);
// feature film: spp samples of every pixel of the listed rows accumulated into f in sample order; rays6 null: the rays of cam.lens for the keys
// (p, f.n[p] + s) (flags bit 0: FIX_ROW_INDEX), else the caller's rays in mi355rt_render_rays layout (device memory); mode as launch_intersect
hipError_t launch_features(hipStream_t stream, const DScene& sc, const DCamera& cam, uint32_t flags, uint32_t seed, uint32_t stack_depth, int mode,
                           const uint32_t* rows, uint32_t nrows, uint32_t spp, const float* rays6, const FeaturePlanes& f);
hipError_t launch_features_clear(hipStream_t stream, const uint32_t* rows, uint32_t nrows, uint32_t width, const FeaturePlanes& f);
// the feature film's means as guides (g0 = (normal, t), g1 = (albedo, prim bits): what launch_denoise reads); alpha[p] = hits / n
hipError_t launch_features_guides(hipStream_t stream, uint32_t npix, const FeaturePlanes& f, float4* g0, float4* g1);
hipError_t launch_features_alpha(hipStream_t stream, uint32_t npix, const FeaturePlanes& f, float* alpha);
// film -> `iterations` filter iterations ping-ponging ping / pong (npix float4 each; flags: npix u32) -> rgb (npix * 3 floats) and / or packed (npix u32);
// film_direct non-null: the split read-out (the indirect part is filtered, the direct part added back)
hipError_t launch_denoise(hipStream_t stream, const DenoiseArgs& args, uint32_t iterations, const float* film_sum, const float* film_sumsq, const uint32_t* film_n,
                          const float* film_direct, const float4* g0, const float4* g1, uint32_t* flags, float4* ping, float4* pong, float* rgb, uint32_t* packed);
// display read-out.  The source image: film == true: img = the film's sums (c = s * (1 / n)); false: img = the denoiser's rgb on the device.
// hist: the kDisplayHistWords words of mi355rt_luminance_histogram, zeroed by the caller; at most num_cus blocks
hipError_t launch_display_hist(hipStream_t stream, int num_cus, uint32_t npix, const float* img, const uint32_t* film_n, bool film, uint32_t* hist);
// table: 256 floats, [k] = T[k] of mi355rt_display_srgb_thresholds (k = 1..255; [0] unused), read with TRANSFER_SRGB only
hipError_t launch_display_pack(hipStream_t stream, const DisplayArgs& args, uint32_t npix, const float* img, const uint32_t* film_n, bool film, const float* table,
                               uint32_t* packed);
// the gather microbenchmark behind bench.py's roofline: num_cus * 8 blocks walk `steps` random nodes of `table` each
hipError_t launch_gather_rate(hipStream_t stream, int num_cus, const void* table, uint32_t nnodes, uint32_t steps, uint32_t* sink);
hipError_t launch_numerics(hipStream_t stream, const float* a, const float* b, uint32_t n, float* q, float* r, float* p);

}  // namespace mi355rt
