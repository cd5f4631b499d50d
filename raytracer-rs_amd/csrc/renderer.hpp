// renderer.hpp — host side of the device render path: owns the HIP buffers, the camera and the
// film of one RayTracer (raytracer/mod.rs:32-47) and schedules the wavefront passes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <array>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "../../include/mi355rt.h"
#include "bvh.hpp"
#include "camera.hpp"
#include "device_buffer.hpp"
#include "device_types.hpp"
#include "scene.hpp"

namespace mi355rt {

class Renderer {
public:
    static std::unique_ptr<Renderer> create(const SceneData& scene, const mi355rt_config& cfg, std::string& err, int& code);
    ~Renderer();

    uint32_t trace_frame_additive();                                   // mod.rs:80-117
    bool render(uint32_t spp, bool wait = true);                        // wait == false: queued only (mi355rt_render_async)
    // adaptive sampling: rounds of ac.batch_spp samples in the active tiles until none is left; ac is validated by the caller
    bool render_adaptive(const mi355rt_adaptive_config& ac, mi355rt_adaptive_stats& st);
    bool adaptive_tile_mask(const mi355rt_adaptive_config& ac, uint8_t* out, uint32_t& active);     // the next round's verdict, tiles_x() * tiles_y() bytes
    // mi355rt_render_tiles: spp samples into the tiles of the caller's mask (tiles_x() * tiles_y() bytes), under whatever lens the handle has; the caller
    // has checked the arguments.  device: the mask is device memory of this handle's device, read in place
    bool render_tiles(const uint8_t* mask, uint32_t spp, bool device);
    uint32_t tiles_x() const { return (cfg.width + kAdaptiveTile - 1) / kAdaptiveTile; }
    uint32_t tiles_y() const { return (cfg.height + kAdaptiveTile - 1) / kAdaptiveTile; }
    bool get_tonemapped(uint32_t* out, size_t n);                       // mod.rs:120-128
    bool tonemap_owned_rows_device(uint32_t* device_out, size_t n, hipStream_t caller_stream = nullptr);
    bool last_counts(mi355rt_ray_counts& out);
    bool film_get(float* sum, float* sumsq, uint32_t* n);
    bool film_get_direct(float* sum);                                   // the direct film (MI355RT_FLAG_DIRECT_FILM), width * height * 3 floats
    bool set_seed(uint64_t seed);
    bool set_flags(uint32_t flags);
    bool film_clear();                                                  // film.rs:37-41
    // mi355rt_film_set / mi355rt_film_add: whole-image host planes -> the owned rows of the film; the caller has checked the arguments
    struct FilmPlanes { const float* sum; const float* sumsq; const uint32_t* n; const float* direct; };
    bool film_put(const FilmPlanes& in, bool add);
    bool intersect(const float* rays6, size_t n, float* tuv, uint32_t* prim, uint8_t* blocked);
    // caller-supplied rays; the caller has checked the arguments.  device: every pointer is device memory of this handle's device
    bool trace_rays(const float* rays6, const uint32_t* keys2, size_t n, bool device, const mi355rt_ray_outputs& out);
    bool render_rays(const float* rays6, uint32_t spp, bool device);
    // gather: light arriving at npoints caller-given points; the caller has checked the arguments.  device: every pointer is device memory
    bool gather(const float* points3, const float* normals3, const uint32_t* ids, size_t npoints, const mi355rt_gather_config& gc, bool device, const mi355rt_gather_outputs& out);
    // probes; the caller has checked the arguments.  probes_gather: gather's sphere-mode samples projected onto nine SH coefficients per point;
    // probes_lookup: a read-out of such a grid that traces nothing and touches neither films nor counters.  device: every pointer is device memory
    bool probes_gather(const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_config& pc, bool device, const mi355rt_probe_outputs& out);
    bool probes_lookup(const mi355rt_probe_grid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const float* points3, const float* dirs3, size_t npoints,
                       uint32_t mode, bool device, float* rgb3, uint8_t* ok);
    // probe visibility; the caller has checked the arguments.  probes_gather_depth: probes_gather (out may hold no pointer) with the depth film
    // of the same traced pass; probes_lookup_vis: probes_lookup with each corner's weight multiplied by the probe's visibility and facing
    bool probes_gather_depth(const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_config& pc, bool device, const mi355rt_probe_outputs& out,
                             const mi355rt_probe_depth& depth);
    bool probes_lookup_vis(const mi355rt_probe_grid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth& depth,
                           const mi355rt_probe_vis_config& vc, const float* points3, const float* dirs3, const float* normals3, size_t npoints, uint32_t mode, bool device,
                           float* rgb3, uint8_t* ok);
    // probe placement; the caller has checked the arguments.  probes_survey: the closest hits of probes_gather's samples reduced to counts and
    // three records per point; probes_place: the move and the state of every probe of a grid; probes_lookup_placed: probes_lookup_vis with the probes' offsets
    bool probes_survey(const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_survey_config& sc, bool device, const mi355rt_probe_survey& out);
    bool probes_place(const mi355rt_probe_grid& grid, const mi355rt_probe_survey& survey, const mi355rt_probe_place_config& pc, const float* offsets, bool device,
                      float* new_offsets, uint8_t* verdict, uint8_t* state);
    bool probes_lookup_placed(const mi355rt_probe_grid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth& depth,
                              const mi355rt_probe_vis_config& vc, const float* offsets, const float* points3, const float* dirs3, const float* normals3, size_t npoints,
                              uint32_t mode, bool device, float* rgb3, uint8_t* ok);
    // probe-lit shading; the caller has checked the arguments.  probe_lit_points: the hemisphere mean of a probe volume at surface points, under
    // probes_lookup's rules; probe_lit_rays: closest hit, shade() with shadow rays and that mean along caller-given rays, under probes_survey's rules.
    // depth, vc null: no depth films (then offsets is null too).  device: every pointer, the volume's arrays included, is device memory
    bool probe_lit_points(const mi355rt_probe_volume& vol, const float* points3, const float* normals3, size_t npoints, uint32_t flags, bool device, float* indirect3, uint8_t* ok);
    bool probe_lit_rays(const mi355rt_probe_volume& vol, const float* rays6, size_t nrays, uint32_t flags, bool device, const mi355rt_probe_lit_outputs& out);
    // bake; the caller has checked the arguments.  device: every pointer but ncovered is device memory.  Neither touches films, camera, counters
    bool bake_texels(const float* uv, uint32_t width, uint32_t height, bool flip, bool device, const mi355rt_bake_texel_outputs& out, uint32_t* ncovered);
    bool bake_atlas(const uint32_t* ids, const float* values3, uint32_t n, uint32_t width, uint32_t height, uint32_t dilate, bool device, float* atlas, uint8_t* valid, uint32_t& verdict);
    // lens models; the caller has checked the arguments.  set_lens keeps the film, the caller-ray mark, the counters and current_row
    bool set_lens(const mi355rt_lens& l);
    const mi355rt_lens& lens() const { return lens_; }
    bool has_lens() const { return lens_.model != MI355RT_LENS_PINHOLE; }
    bool lens_rays(uint32_t spp, bool device, float* rays6);            // width * height * spp rays of the next render(spp); a read-out: nothing of the handle changes
    bool caller_ray_film() const { return caller_ray_film_; }           // the film holds samples of mi355rt_render_rays: the camera's guides do not describe it
    bool synchronize();                                                 // wait for everything queued on this handle
    // ---- multi-GPU gather of the packed u32 stripes into the root's frame.  Two transports end in the
    // same place: the in-process device group (hipMemcpyPeerAsync, csrc/group.cpp) and RCCL between processes (comm_*).
    uint32_t slot_rows() const;                                         // rows of one rank's slot: ceil(stripes / world) * stripe_rows
    uint32_t rows_of_rank(uint32_t rank) const;
    bool gather_prepare(bool root);                                     // root: world slots, others: their own slot
    uint32_t* gather_slot(uint32_t rank) { return d_gather_ ? d_gather_.get() + (gather_is_root_ ? (size_t)rank : 0) * slot_rows() * cfg.width : nullptr; }
    bool tonemap_to_gather_slot();                                      // own rows, packed, into the own slot (on the handle's stream)
    bool finish_gather(uint32_t* host_out, size_t n);                   // root: slots -> frame (+ copy to the host when host_out != null)
    hipStream_t stream() const { return stream_; }
    hipEvent_t gather_event() const { return ev_gather_; }
    bool comm_available();                                              // local pre-check of comm_init (no communication)
    bool comm_init(const uint8_t* id128);                               // RCCL communicator over the stripe ranks (collective)
    bool comm_gather(uint32_t root, uint32_t* host_out, size_t n);      // collective: grouped ncclSend / ncclRecv to the root, then finish_gather there
    void comm_destroy();
    uint32_t comm_ranks();                                              // ncclCommCount of the live communicator, 0 without one
    long check_guards();                                                // MI355RT_DEBUG_GUARD: corrupted guard bytes behind the pass buffers
    size_t hbm_allocated_bytes() const { return hbm_bytes_; }           // device memory this handle holds: every DeviceBuffer that counts into hbm_bytes_
    bool debug_gather_rate(uint32_t table_nodes, uint32_t steps, double out[3]);
    bool debug_slab(const float* inv_rays6, const float* cubes6, size_t n, uint8_t* hit, float* tmin);
    bool film_stat(bool variances, float* rgb);
    // denoised read-out; the caller has checked the arguments (a whole image on one device, a valid config)
    bool get_guides(float* depth, float* normal3, float* albedo3, uint32_t* prim);
    bool get_denoised(const mi355rt_denoise_config& dc, float* rgb, uint32_t* packed, bool split = false);   // split: the indirect part is filtered
    bool has_direct_film() const { return (cfg.flags & MI355RT_FLAG_DIRECT_FILM) != 0; }
    // light films (MI355RT_FLAG_LIGHT_FILMS); the caller has checked the flag and the arguments.  planes: nlights() * width * height * 3 floats
    bool has_light_films() const { return (cfg.flags & MI355RT_FLAG_LIGHT_FILMS) != 0; }
    uint32_t nlights() const { return nlights_; }
    bool light_films_get(float* planes);
    bool light_films_put(const float* planes, bool add);
    // mi355rt_get_relit_pixels: weights3 nlights() * 3 floats; dc null: the reference's tone map; rgb / packed: either may be null
    bool get_relit(const float* weights3, const mi355rt_display_config* dc, float* rgb, uint32_t* packed, float& exposure_used);
    // feature film; the caller has checked the arguments.  rays6 null: spp samples under the handle's lens, else along the caller's rays
    bool features_render(const float* rays6, uint32_t spp, bool device);
    bool features_get(uint32_t* n, uint32_t* hits, float* depth, float* normal3, float* albedo3);
    bool features_alpha(float* alpha);
    bool features_clear();
    enum FeatureStamp { kFeatEmpty = 0, kFeatCamera = 1, kFeatRays = 2 };     // what made the rays of the feature film's samples
    FeatureStamp feature_stamp() const { return feat_stamp_; }
    bool feature_view_current();                                         // a camera-stamped feature film: its stamp is the handle's current view
    uint32_t guide_source() const { return guide_source_; }
    void set_guide_source(uint32_t s) { guide_source_ = s; }
    // display read-out; the caller has checked the arguments.  source: MI355RT_DISPLAY_SOURCE_*; dn is read for the denoised sources only
    bool display_histogram(uint32_t source, const mi355rt_denoise_config& dn, mi355rt_luminance_histogram& out);
    bool get_display(const mi355rt_display_config& dc, const mi355rt_denoise_config& dn, uint32_t* packed, float& exposure_used);
    // mi355rt_display_image: DISPLAY MAPPING of the caller's image (host memory, npix x 3 floats) with a fixed exposure; dc null: the reference's tone map.  Every
    // buffer is a temporary: nothing of the handle changes
    bool display_image(const float* rgb3, size_t npix, const mi355rt_display_config* dc, uint32_t* packed);
    void speculation_stats(uint64_t out[2]) const { out[0] = spec_launched_; out[1] = spec_adopted_; }
    bool debug_numerics(const float* a, const float* b, size_t n, float* q, float* r, float* p);
    bool debug_sample(uint32_t pixel, uint32_t sampleno, float* color3, float* node_L, size_t nodes);

    Camera camera;
    mi355rt_config cfg;
    mi355rt_ray_counts counts{};
    std::string last_error;
    std::vector<float> table;            // 65536 x 3
    std::vector<uint32_t> owned_rows;
    Bvh bvh;
    uint32_t ntri = 0;
    uint32_t current_row = 0;
    uint32_t slices = 1;                  // concurrent frame slices of render() (1..8), MI355RT_SLICES / mi355rt_set_slices.  Round 2 ran 3: they filled the
                                          // tails of each other's trace launches; with the tail chunks handed out in parts one slice is as fast and holds a third of the memory
    bool slices_explicit = false;         // set through the API: used as given, also for small frames
    uint32_t nodes_per_sample = 1;
    uint32_t level_first[kMaxLevels + 1] = { 0 };
    std::vector<std::array<float, 6>> cull_boxes_;   // top BVH subtree boxes for primary-chunk culling
    size_t hbm_bytes_ = 0;               // device bytes held by the DeviceBuffers below (declared before them: they count into it until they are destroyed)
    DeviceBuffer<uint32_t> d_cull_mask_; // kCullGrid x kCullGrid coverage bits (device_types.hpp), rebuilt when the camera changes
    std::vector<float> mask_key_;        // the camera the mask on the device was built for (rot, origin, max_x, max_y); empty: none
    float mask_dom_[4] = { 0, 0, 0, 0 }; // its domain: x0, y0, 1 / cell width, 1 / cell height
    bool mask_valid_ = false;
    DeviceBuffer<uint2> d_tile_ofs_, d_tile_entries_;     // screen-space triangle bins of the primary rays (device_types.hpp), rebuilt with the mask
    std::vector<float> bins_key_;        // camera + layout the bins on the device were built for
    uint32_t bins_layout_[3] = { 0, 0, 0 };   // tile_cols, tile_rg, tile_nblocks
    bool bins_valid_ = false;
    double bins_ms_ = 0.0; size_t bins_entries_ = 0;
    uint32_t oct_stats_[8] = { 0 };       // the reference's octree: nodes, inner, leaves, empty, depth, triangle refs
    double build_ms_[2] = { 0.0, 0.0 };   // build times inside create (wall): BVH (host binned SAH, or the device build), octree (SAT, host)
    double light_map_ms_ = 0.0;           // build time of the lights' depth cube maps inside create
    uint64_t rays_read_ = 0;              // MI355RT_FLAG_COUNT_STEPS: rays the trace launches of the last call took from their queues (DCounters::refill_rays)
    double reflect_mask_info_[4] = { 0.0, 0.0, 0.0, 0.0 };   // the triangles' direction masks: bins per face edge (0: none), build ms inside create, share of clear bits, bytes on the device
    bool bvh_on_device_ = false;          // MI355RT_FLAG_DEVICE_LBVH and the device build served the scene
    bool wide_ = false;                   // the device holds the 4-wide tree (bvh.nodes4): this build's kernels walk it
    uint32_t traversal_rows() const { return (wide_ ? bvh.stack_need4 : bvh.max_depth) + 1u; }       // stack rows the trace loops need (kernels.hip, stack_bytes)
    double lbvh_device_ms_ = 0.0;         // its device time (kernels + sort)
    enum Mode { kModeConfirm = 0, kModeOctreeWalk = 1, kModeTrueClosest = 2 };
    Mode mode_ = kModeConfirm;            // intersector semantics, fixed at creation
    static_assert(kModeConfirm == 0 && kModeOctreeWalk == 1 && kModeTrueClosest == 2, "the launches take (int)mode_ (kernels.hpp, launch_intersect)");

private:
    Renderer() = default;
    bool init(const SceneData& scene, std::string& err, int& code);
    bool bind();
    bool quiet();                         // bind() and settle_speculation()
    bool fail(hipError_t e, const char* what);
    // the host path of every read-out of a probe grid: launch(volume, points, dirs, normals, rgb, ok) queues its kernel on the staged arrays
    template <class Launch>
    bool volume_readout(const mi355rt_probe_volume& vol, const float* points3, const float* dirs3, const float* normals3, size_t npoints, bool device, float* rgb3, uint8_t* ok,
                        Launch launch);
    // A frame slice: an interleaved share of the owned rows with its own stream and pass buffers.  The
    // slices of one render() call run concurrently, so that the drain window at the end of one slice's
    // (persistent) trace launch is filled by the other slices' kernels.  Pixels of different slices are
    // disjoint, so the film needs no ordering between them.
    struct Slice {
        hipStream_t stream = nullptr;            // slice 0 runs on the renderer's main stream
        hipEvent_t done = nullptr;
        std::vector<uint32_t> rows;              // this slice's rows (host copy of d_rows)
        DeviceBuffer<uint32_t> d_rows;
        DeviceBuffer<uint32_t> d_ctrl;           // per round: chunk cursors
        bool ctrl_clean = true;                  // the cursors are zero (creation, or the last pass's resolve kernel left them so)
        // the pass buffers, sized for `capacity` samples (ensure_pass_capacity)
        DeviceBuffer<> d_queue[2];
        DeviceBuffer<uint32_t> d_chunk_counts[2];   // rays per chunk in each queue
        DeviceBuffer<> d_hits;
        DeviceBuffer<uint32_t> d_hit_prim;       // hit records of the round being processed (16 B per queue record)
        DeviceBuffer<float> d_slot_L;
        DeviceBuffer<> d_slot_ps;                // light-term slot -> (pixel, sample number) of its sample (uint2)
        DeviceBuffer<uint32_t> d_sample_slot;    // primary sample -> slot of its light terms (0xFFFFFFFF: the primary ray missed)
        DeviceBuffer<uint32_t> d_live;           // live-chunk lists of the pass, one per work cursor (DPass::live)
        DeviceBuffer<uint32_t> d_block_culled;   // cached culling verdicts of the pass's pixel blocks (DPass::block_culled) for the camera / layout of cull_key
        std::vector<float> cull_key;
        size_t capacity = 0;                     // samples
        size_t queue_records = 0;
        size_t count_entries = 0;                // entries of each d_chunk_counts array
        template <class F> void for_each_pass_buffer(F f) { f(d_queue[0]); f(d_queue[1]); f(d_chunk_counts[0]); f(d_chunk_counts[1]); f(d_hits); f(d_hit_prim); f(d_slot_L); f(d_slot_ps); f(d_sample_slot); f(d_live); }
        void release_pass_buffers() { for_each_pass_buffer([](auto& b) { b.reset(); }); capacity = 0; }
    };
    bool ensure_pass_capacity(Slice& sl, size_t nsamples);
    size_t pass_sample_budget() const;                                  // samples per pass: the default or MI355RT_PASS_SAMPLES (config.samples_per_pass is the callers' matter)
    bool fit_ray_pass(Slice& sl, size_t& per);                          // ensure_pass_capacity(sl, per), per halved while the device is out of memory
    void free_pass_buffers();
    // The chunk loop of gather and probes_gather: the samples of npoints points in chunks of cp points x cs samples sized by the pass
    // capacity; per chunk launch_gather_rays, one ray-fed pass when `traced`, then reduce(chunk).  The sample chunks of a point range come in ascending order.
    struct GatherChunk { uint32_t point0, cp, sample0, cs; const float* rays; const uint8_t* valid; const float* rgb; const float* tuv; const uint32_t* prim; };
    bool gather_chunks(const float* d_points, const float* d_normals, const uint32_t* d_ids, size_t npoints, uint32_t spp, uint32_t first_sample, bool traced, bool want_rgb,
                       bool want_hits, const std::function<hipError_t(const GatherChunk&)>& reduce);
    bool assign_slice_rows(uint32_t nslices);
    // A ray-fed pass (DPass::ray_in ...).  mode (device_types.hpp) kRaysOfPixels: the film's pixels with the caller's rays (base: the call's sample
    // number of the pass's first sample, set per pass by enqueue_frame); kRaysFree: `count` free rays, one sample each, resolved into the out pointers (device memory,
    // the pass's part); kRaysOfLens: no buffer at all — the film's pixels with the rays of the handle's lens, made by the kernels (DCamera::lens)
    struct RayFeed { uint32_t mode; const float* rays; const uint32_t* keys; uint32_t base; uint32_t count; float4* hit; float* rgb; float* direct; float* tuv; uint32_t* prim; };
    // What run_pass is asked for: nrows rows of the list d_rows from entry row0 on (cyclic over row_wrap entries), spp samples per pixel
    static constexpr uint32_t kNoRowWrap = 0xFFFFFFFFu;                // DPass::row_wrap: the row list is not cyclic
    struct PassRequest {
        const uint32_t* d_rows = nullptr; uint32_t row0 = 0, nrows = 0, spp = 1, row_wrap = kNoRowWrap;
        const uint8_t* tile_active = nullptr;                           // DPass::tile_active
        const RayFeed* feed = nullptr;                                  // null: the pinhole camera
        bool explicit_sample = false; uint32_t epixel = 0, esample = 0; // debug_sample: the pass is this one sample
    };
    bool run_pass(Slice& sl, const PassRequest& rq);
    bool cached_cull_verdicts(Slice& sl, const DCamera& cam, DPass& ps, uint32_t nrows);          // run_pass: DPass::block_culled for this camera and layout
    bool balance_debug_reset();                                                                  // run_pass, MI355RT_DEBUG_UTIL: before a trace launch,
    bool balance_debug_report(hipStream_t st, uint32_t round);                                   // and after it (synchronises)
    // the owned rows x spp as wavefront passes on the slices (pass planning, OOM halving), forked behind `fork` on the main stream; tile_active: DPass::tile_active;
    // feed (kRaysOfPixels): the frame's primary rays are the caller's
    bool enqueue_frame(uint32_t spp, hipEvent_t fork, const uint8_t* tile_active, const RayFeed* feed = nullptr);
    bool caller_ray_film_ = false;
    mi355rt_lens lens_{ MI355RT_LENS_PINHOLE, 0.0f, 1.0f, 0.0f };    // the handle's lens; not PINHOLE: render() runs lens passes (RayFeed kRaysOfLens), the guides take its centre rays
    bool join_slices();                                                 // the main stream waits for the slices of the call in flight
    bool adaptive_verdict(const mi355rt_adaptive_config& ac, uint32_t& tiles, uint64_t& pixels);    // d_tile_active_ <- the verdict of the current film
    DeviceBuffer<uint8_t> d_tile_active_;                               // adaptive sampling: one byte per tile (DPass::tile_active); render_tiles: the device copy of a host mask
    DeviceBuffer<unsigned long long> d_tile_count_;                     // (owned pixels of the active tiles << 32) + active tiles
    // Denoised read-out, allocated on first use: the guides (g0 = (normal, t), g1 = (albedo, prim bits)) for the camera and row-index
    // flag of guides_key_, and the per-call buffers of the filter
    bool refresh_guides();
    DeviceBuffer<float4> d_guide0_, d_guide1_;
    std::vector<float> guides_key_;      // rot, origin, max_x, max_y, FIX_ROW_INDEX bit and the lens (model and the fields it reads) of the guides on the device; empty: none
    // Feature film, allocated on first use: one buffer of 36 bytes per pixel (feat_ points into it); its view stamp; the guides converted from
    // it (MI355RT_GUIDES_FEATURES), buffers of their own beside the centre-ray guides so that each source keeps its cache, rebuilt when feat_version_ moves on
    bool ensure_features();
    std::vector<float> view_key();       // the key of guides_key_ for the handle's current camera, FIX_ROW_INDEX bit and lens
    bool refresh_feature_guides();
    const float4* guide0() const { return guide_source_ == MI355RT_GUIDES_FEATURES ? d_fguide0_.get() : d_guide0_.get(); }
    const float4* guide1() const { return guide_source_ == MI355RT_GUIDES_FEATURES ? d_fguide1_.get() : d_guide1_.get(); }
    DeviceBuffer<uint8_t> d_features_;
    FeaturePlanes feat_{};
    FeatureStamp feat_stamp_ = kFeatEmpty;
    std::vector<float> feat_key_;        // kFeatCamera: the view of the samples
    uint64_t feat_version_ = 0, fguides_version_ = 0;      // fguides_version_ == feat_version_: d_fguide*_ hold the current feature film
    DeviceBuffer<float4> d_fguide0_, d_fguide1_;
    uint32_t guide_source_ = MI355RT_GUIDES_CENTRE;
    DeviceBuffer<float4> d_dn_ping_, d_dn_pong_;
    DeviceBuffer<uint32_t> d_dn_flags_, d_dn_packed_;
    DeviceBuffer<float> d_dn_rgb_;
    bool run_denoise(const mi355rt_denoise_config& dc, bool rgb, bool packed, bool split);   // the filter, queued: d_dn_rgb_ / d_dn_packed_ hold the read-out
    // Display read-out, allocated on first use: the histogram's 260 words, the 256-entry sRGB threshold table, the packed image
    bool display_source(uint32_t source, const mi355rt_denoise_config& dn, const float*& img, bool& film);   // queues the denoiser for sources 1 and 2
    bool display_hist_queue(const float* img, bool film, mi355rt_luminance_histogram& out);                    // kernel + read-back, synchronous
    DeviceBuffer<uint32_t> d_disp_hist_, d_disp_packed_;
    DeviceBuffer<float> d_disp_table_;
    void describe_pass(DPass& ps, const Slice& sl, const PassRequest& rq, uint32_t npix, size_t nsamples, uint32_t chunk) const;
    bool begin_call();
    bool end_call(uint64_t primary, bool wait = true);
    bool fetch_counts(uint64_t primary, bool timed_call);
    bool queue_counts_copy();
    void mark_dirty_window(uint32_t first, uint32_t total);
    // layout + rows: the pass whose primary rays the tile bins are for and the (host copy of the) row list it walks (null: no bins needed)
    DCamera device_camera(const DPass* layout = nullptr, const std::vector<uint32_t>* rows = nullptr);
    bool refresh_tile_bins(DCamera& c, const double inv[3][3], double pad, double zmin, const DPass& ps, const std::vector<uint32_t>& rows);
    bool refresh_cull_mask(DCamera& c, const double inv[3][3], double pad, double zmin, bool build);
    bool project_triangles(const DCamera& c, const double inv[3][3], double pad, double zmin);
    struct TriRect { double x0, x1, y0, y1; };
    std::vector<TriRect> tri_rects_;     // padded screen rectangles of the triangles (BVH order) for the camera of rects_key_
    std::vector<float> rects_key_;
    bool rects_ok_ = false;
    void collect_cull_boxes();
    void build_sample_table(std::vector<float>& table4);
    template <class T> bool upload(DeviceBuffer<T>& buf, const void* src, size_t bytes);
    template <class T> bool upload(T*& dptr, const void* src, size_t bytes);     // a scene array: owned by scene_bufs_

    int num_cus_ = 0;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_begin_ = nullptr, ev_end_ = nullptr;
    std::vector<hipEvent_t> ev_pool_;
    size_t ev_used_ = 0;
    std::vector<uint8_t> ev_secondary_;  // per event pair: the launch traced secondary rays (rounds >= 1)
    std::vector<DeviceBuffer<>> scene_bufs_;   // scene and acceleration structures (dscene_ points into them)

    DScene dscene_{};
    DeviceBuffer<float> d_film_sum_, d_film_sumsq_; DeviceBuffer<uint32_t> d_film_n_;
    DeviceBuffer<float> d_film_direct_;  // MI355RT_FLAG_DIRECT_FILM: per pixel, the sum of its samples' root light terms (null without the flag)
    DeviceBuffer<float> d_film_lights_;  // MI355RT_FLAG_LIGHT_FILMS: nlights_ planes of width * height * 3 floats, per pixel the sum of its samples' light radiances (null without the flag or without lights)
    uint32_t lights_stride() const { return cfg.width * cfg.height * 3u; }      // floats per plane
    DeviceBuffer<float> d_relit_rgb_, d_relit_weights_;   // mi355rt_get_relit_pixels, allocated on first use: the relit image (12 bytes per pixel; d_disp_packed_ takes the packed one), the weights
    bool ensure_display_buffers(bool hist_and_table);     // d_disp_packed_ [, d_disp_hist_, d_disp_table_], on first use
    DeviceBuffer<float> d_bake_tris_;    // bake: per triangle in SCENE order (A, B - A, C - A), 36 bytes, made from bvh.tris by the first mi355rt_bake_texels that asks for points and kept
    DeviceBuffer<uint32_t> d_owned_rows_, d_all_rows_, d_tmp_rows_;
    DeviceBuffer<uint32_t> d_ldr_;
    PinnedBuffer<uint32_t> h_ldr_;       // host mirror of d_ldr_ (get_tonemapped_pixels)
    std::vector<uint8_t> ldr_dirty_;     // per row: film changed since the row was last tone-mapped into d_ldr_ / h_ldr_
    hipEvent_t ev_tonemap_ = nullptr, ev_gather_ = nullptr;
    DeviceBuffer<uint32_t> d_gather_;    // gather slots (see gather_prepare)
    bool gather_is_root_ = false;
    void* comm_ = nullptr;               // ncclComm_t
    bool counts_pending_ = false;        // the last call was an asynchronous 50-row frame: counters not fetched yet
    uint64_t pending_primary_ = 0;
    bool pending_timed_ = false;         // the pending call was a whole frame: its HIP-event time is read with the counters
    DeviceBuffer<DCounters> d_counters_;
    // Speculation of the drop-in loop (trace_frame_additive): the NEXT 50-row frame is launched right behind the one just asked for, so that the device
    // traces it while the host reads out the current one (main.rs:197-207 alternates the two calls; one frame keeps the chip busy for 0.25 ms of latency,
    // not of work).  The rows it changes are backed up first; a next call that is not the predicted one (camera moved, film cleared, anything else
    // touched) puts them back.  Read-outs of the finished frame run on read_stream_, beside the speculative launch.
    struct Speculation { bool valid = false; uint32_t row = 0, first = 0, total = 0, next_row = 0; std::vector<float> cam_key; uint64_t seed = 0; uint32_t flags = 0; } spec_;
    DeviceBuffer<DCounters> d_counters_spec_; PinnedBuffer<DCounters> h_counters_spec_;
    DeviceBuffer<float> d_bk_sum_, d_bk_sumsq_; DeviceBuffer<uint32_t> d_bk_n_;
    DeviceBuffer<float> d_bk_direct_;    // with d_film_direct_ only
    hipStream_t read_stream_ = nullptr;
    hipEvent_t ev_call_done_ = nullptr, ev_spec_done_ = nullptr;      // behind the kernel (and the counters' copy) of the frame last asked for / of the speculative one
    bool call_done_valid_ = false;        // ev_call_done_ marks the last 50-row frame: read-outs wait for it, not for the stream
    uint64_t spec_launched_ = 0, spec_adopted_ = 0;
    bool settle_speculation();            // put the speculative frame's rows back (if one is out)
    bool launch_fused_window(uint32_t first, uint32_t total, const DCamera& cam, DCounters* dcounters);
    PinnedBuffer<DCounters> h_counters_; // host mirror (queue_counts_copy)
    DeviceBuffer<float> d_debug_color_;
    static constexpr uint32_t kMaxSlices = 8;
    Slice slices_[kMaxSlices];
    uint32_t rows_assigned_for_ = 0;     // number of slices the row lists were last split into
    uint32_t active_slices_ = 1;         // slices used by the call in flight (begin_call .. end_call)
    // primary samples per work chunk of the wavefront passes: 256 / 128 / 64 -> 23.1 / 24.6 / 28.4 ms per frame, smaller chunks cost more per chunk than
    // they balance (profiles/r03_notes.md)
    static constexpr uint32_t kChunk = 256;
    static constexpr size_t kGuardBytes = 256;
    static constexpr uint32_t kMinChunk = 16;   // smallest chunk any launcher cuts a pass into (the fused 50-row launch: 16 / 32 / 64)
    uint32_t max_level_nodes_ = 1;
    bool alloc_failed_ = false;          // the last ensure_pass_capacity failure was an out-of-memory
    uint32_t records_per_sample_ = 1;
    uint32_t nlights_ = 0;
    uint64_t launches_ = 0;
};

}  // namespace mi355rt
