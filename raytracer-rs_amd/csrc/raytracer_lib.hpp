// raytracer_lib.hpp — C++ mirror of the reference crate's public surface (raytracer_lib/src/lib.rs)
// over the C ABI of libmi355rt.so.  Same names, argument order and error behaviour:
//   create_raytracer(collada_doc, triangles_per_leaf, width, height) -> Result<RayTracer, String>   lib.rs:15-20
//   create_raytracer_from_file(collada_filename, ...)                                               lib.rs:22-27
//   RayTracer::trace_frame_additive() -> u32, get_tonemapped_pixels() -> Vec<u32>                   raytracer/mod.rs:80,120
//   RayTracer::camera.{move_rel, add_x_angle, add_y_angle}, RayTracer::film.clear()                 camera.rs:63-78, film.rs:37
//   stats::Stats::{new, stats, mean_stats}                                                          stats.rs:11-39
//   DEFAULT_TRIANGLES_PER_LEAF                                                                      lib.rs:7
// Err(String) becomes a thrown std::runtime_error carrying the same text.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/mi355rt.h"

namespace raytracer_lib {

constexpr size_t DEFAULT_TRIANGLES_PER_LEAF = MI355RT_DEFAULT_TRIANGLES_PER_LEAF;

class RayTracer;

class Camera {            // scene/camera.rs (pub methods used by raytracer/src/main.rs:125-161)
public:
    void move_rel(float x, float y, float z) { mi355rt_camera_move_rel(h_, x, y, z); }
    void add_x_angle(float radians) { mi355rt_camera_add_x_angle(h_, radians); }
    void add_y_angle(float radians) { mi355rt_camera_add_y_angle(h_, radians); }
private:
    friend class RayTracer;
    mi355rt_handle* h_ = nullptr;
};

class Film {              // raytracer/film.rs
public:
    void clear() { mi355rt_film_clear(h_); }
    std::vector<float> get_pixels() const
    {
        std::vector<float> out((size_t)mi355rt_width(h_) * mi355rt_height(h_) * 3);
        mi355rt_film_get_pixels(h_, out.data());
        return out;
    }
    // the direct film of a handle created with MI355RT_FLAG_DIRECT_FILM (include/mi355rt.h): width*height*3 sums
    std::vector<float> direct_sums() const
    {
        std::vector<float> out((size_t)mi355rt_width(h_) * mi355rt_height(h_) * 3);
        if (mi355rt_film_get_direct(h_, out.data()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return out;
    }
    // film set, add, save and load (include/mi355rt.h).  The planes are whole images in the layout of mi355rt_film_get; direct is
    // non-null exactly for a handle created with MI355RT_FLAG_DIRECT_FILM; only the rows the handle owns are written.
    void set(const float* sum_rgb, const float* sumsq_rgb, const uint32_t* n, const float* direct_rgb = nullptr)
    {
        if (mi355rt_film_set(h_, sum_rgb, sumsq_rgb, n, direct_rgb, (size_t)mi355rt_width(h_) * mi355rt_height(h_)) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
    }
    void add(const float* sum_rgb, const float* sumsq_rgb, const uint32_t* n, const float* direct_rgb = nullptr)
    {
        if (mi355rt_film_add(h_, sum_rgb, sumsq_rgb, n, direct_rgb, (size_t)mi355rt_width(h_) * mi355rt_height(h_)) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
    }
    void save(const std::string& path) const
    {
        if (mi355rt_film_save(h_, path.c_str()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
    }
    void load(const std::string& path, bool add = false)
    {
        if (mi355rt_film_load(h_, path.c_str(), add ? 1 : 0) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
    }
private:
    friend class RayTracer;
    mi355rt_handle* h_ = nullptr;
};

// The feature film (include/mi355rt.h "FEATURE FILM"): the primary hits' depth, normal and albedo summed over jittered samples, and coverage
struct FeaturePlanes { std::vector<uint32_t> n, hits; std::vector<float> depth, normal, albedo; };   // npix, npix, npix, npix * 3, npix * 3
class Features {
public:
    // spp samples per owned pixel under the handle's lens: the rays a cleared film's render(spp) takes
    void render(uint32_t spp) { if (mi355rt_features_render(h_, spp) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_)); }
    // the same along the caller's rays (host memory, the layout of RayTracer::render_rays)
    void render_rays(const std::vector<float>& rays6, uint32_t spp)
    {
        if (mi355rt_features_render_rays(h_, rays6.data(), rays6.size() / 6, spp, MI355RT_RAYS_HOST) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
    }
    FeaturePlanes get() const
    {
        const size_t npix = (size_t)mi355rt_width(h_) * mi355rt_height(h_);
        FeaturePlanes p;
        p.n.resize(npix); p.hits.resize(npix); p.depth.resize(npix); p.normal.resize(npix * 3); p.albedo.resize(npix * 3);
        if (mi355rt_features_get(h_, p.n.data(), p.hits.data(), p.depth.data(), p.normal.data(), p.albedo.data(), npix) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return p;
    }
    // hits / n per pixel (0 where n == 0): the share of a pixel's samples that hit the scene
    std::vector<float> alpha() const
    {
        std::vector<float> a((size_t)mi355rt_width(h_) * mi355rt_height(h_));
        if (mi355rt_features_alpha(h_, a.data(), a.size()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return a;
    }
    void clear() { if (mi355rt_features_clear(h_) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_)); }
private:
    friend class RayTracer;
    mi355rt_handle* h_ = nullptr;
};

// The light films of a handle created with MI355RT_FLAG_LIGHT_FILMS (include/mi355rt.h "LIGHT FILMS"): nlights planes of width * height * 3
// sums, plane li the film of the scene with every other light black; layout [(li * npix + p) * 3 + c]
class LightFilms {
public:
    size_t nlights() const { return mi355rt_light_count(h_); }
    std::vector<float> get() const
    {
        const size_t npix = (size_t)mi355rt_width(h_) * mi355rt_height(h_), nl = nlights();
        std::vector<float> a(nl * npix * 3);
        if (mi355rt_light_films_get(h_, a.data(), nl, npix) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return a;
    }
    // the planes' bits as they are / handle + a, on the rows the handle owns
    void set(const std::vector<float>& a) { put(a, false); }
    void add(const std::vector<float>& a) { put(a, true); }
private:
    void put(const std::vector<float>& a, bool add)
    {
        const size_t npix = (size_t)mi355rt_width(h_) * mi355rt_height(h_), nl = nlights();
        if (a.size() != nl * npix * 3) throw std::runtime_error("light films: nlights * width * height * 3 floats are required");
        if ((add ? mi355rt_light_films_add : mi355rt_light_films_set)(h_, a.data(), nl, npix) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
    }
    friend class RayTracer;
    mi355rt_handle* h_ = nullptr;
};

class RayTracer {         // raytracer/mod.rs:32-47
public:
    Camera camera;
    Film film;
    Features features;
    LightFilms light_films;
    explicit RayTracer(mi355rt_handle* h) : h_(h) { camera.h_ = h; film.h_ = h; features.h_ = h; light_films.h_ = h; }
    RayTracer(RayTracer&& o) noexcept : camera(o.camera), film(o.film), features(o.features), light_films(o.light_films), h_(o.h_) { o.h_ = nullptr; }
    RayTracer(const RayTracer&) = delete;
    RayTracer& operator=(const RayTracer&) = delete;
    ~RayTracer() { mi355rt_destroy(h_); }

    uint32_t trace_frame_additive()
    {
        uint32_t n = mi355rt_trace_frame_additive(h_);
        if (n == 0) throw std::runtime_error(mi355rt_last_error(h_));
        return n;
    }
    std::vector<uint32_t> get_tonemapped_pixels() const
    {
        std::vector<uint32_t> out((size_t)mi355rt_width(h_) * mi355rt_height(h_));
        if (mi355rt_get_tonemapped_pixels(h_, out.data(), out.size()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return out;
    }
    // additions without a reference counterpart
    mi355rt_ray_counts render(uint32_t spp)
    {
        mi355rt_ray_counts c{};
        if (mi355rt_render(h_, spp, &c) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return c;
    }
    // adaptive sampling (include/mi355rt.h): rounds of cfg.batch_spp samples in the tiles whose noise is above the target until none is left
    mi355rt_adaptive_stats render_adaptive(const mi355rt_adaptive_config& cfg)
    {
        mi355rt_adaptive_stats st{};
        if (mi355rt_render_adaptive(h_, &cfg, &st) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return st;
    }
    // mi355rt_render_tiles (include/mi355rt.h, RENDER TILES): spp samples into the tiles of `mask` (tiles_x * tiles_y bytes, host memory), under whatever lens the handle has
    mi355rt_ray_counts render_tiles(const std::vector<uint8_t>& mask, uint32_t spp)
    {
        mi355rt_ray_counts c{};
        if (mi355rt_render_tiles(h_, mask.data(), mask.size(), spp, MI355RT_RAYS_HOST, &c) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return c;
    }
    // the tiles a half-open pixel rectangle [x0, x1) x [y0, y1) touches, clipped to the image (the mask of render_tiles; adaptive.region_mask of the Python package)
    std::vector<uint8_t> region_mask(long long x0, long long y0, long long x1, long long y1) const
    {
        const long long w = mi355rt_width(h_), h = mi355rt_height(h_), T = MI355RT_ADAPTIVE_TILE, tx = (w + T - 1) / T, ty = (h + T - 1) / T;
        std::vector<uint8_t> m((size_t)(tx * ty), 0);
        x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0; x1 = x1 > w ? w : x1; y1 = y1 > h ? h : y1;
        if (x0 < x1 && y0 < y1)
            for (long long t = y0 / T; t <= (y1 - 1) / T; ++t)
                for (long long x = x0 / T; x <= (x1 - 1) / T; ++x) m[(size_t)(t * tx + x)] = 1;
        return m;
    }
    // The loop of mi355rt_render_adaptive on the caller's side, from two calls that work under any lens: the verdict (mi355rt_adaptive_tile_mask), then render_tiles,
    // until no tile is active or cfg.max_rounds rounds have run.  samples_added is the sum of the calls' primary; `sum` (optional) receives the rounds' summed
    // primary, bounce, shadow, primary_hits and total_ms.
    mi355rt_adaptive_stats refine(const mi355rt_adaptive_config& cfg, mi355rt_ray_counts* sum = nullptr)
    {
        const uint32_t T = MI355RT_ADAPTIVE_TILE, tx = (mi355rt_width(h_) + T - 1) / T, ty = (mi355rt_height(h_) + T - 1) / T;
        mi355rt_adaptive_stats st{};
        mi355rt_ray_counts total{};
        std::vector<uint32_t> rows(mi355rt_owned_rows(h_));
        if (!rows.empty() && mi355rt_owned_row_list(h_, rows.data(), rows.size()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        std::vector<uint8_t> tile_row(ty, 0), mask((size_t)tx * ty);
        for (uint32_t r : rows) tile_row[r / T] = 1;
        for (uint8_t t : tile_row) st.tiles += t ? tx : 0u;
        for (;;) {
            const int active = mi355rt_adaptive_tile_mask(h_, &cfg, mask.data(), mask.size());
            if (active < 0) throw std::runtime_error(mi355rt_last_error(h_));
            if (st.rounds == 0) st.tiles_active_first = (uint32_t)active;
            st.tiles_active_last = (uint32_t)active;
            if (active == 0 || (cfg.max_rounds && st.rounds >= cfg.max_rounds)) break;
            const mi355rt_ray_counts c = render_tiles(mask, cfg.batch_spp);
            ++st.rounds;
            total.primary += c.primary; total.bounce += c.bounce; total.shadow += c.shadow; total.primary_hits += c.primary_hits; total.total_ms += c.total_ms;
        }
        st.samples_added = total.primary;
        if (sum) *sum = total;
        return st;
    }
    mi355rt_ray_counts last_counts()
    {
        mi355rt_ray_counts c{};
        if (mi355rt_last_counts(h_, &c) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return c;
    }
    // denoised read-out (include/mi355rt.h): width*height u32 0xAARRGGBB, like get_tonemapped_pixels
    std::vector<uint32_t> get_denoised_pixels(const mi355rt_denoise_config& cfg) const
    {
        std::vector<uint32_t> out((size_t)mi355rt_width(h_) * mi355rt_height(h_));
        if (mi355rt_get_denoised_pixels(h_, &cfg, nullptr, out.data(), out.size()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return out;
    }
    // the same with only the indirect part filtered (a handle created with MI355RT_FLAG_DIRECT_FILM)
    std::vector<uint32_t> get_denoised_pixels_split(const mi355rt_denoise_config& cfg) const
    {
        std::vector<uint32_t> out((size_t)mi355rt_width(h_) * mi355rt_height(h_));
        if (mi355rt_get_denoised_pixels_split(h_, &cfg, nullptr, out.data(), out.size()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return out;
    }
    // display read-out (include/mi355rt.h): exposure, tone curve and transfer on the film or a denoised image; dn == nullptr: the
    // default denoise config; exposure_used receives the exposure the call applied (the derived one with cfg.auto_exposure)
    std::vector<uint32_t> get_display_pixels(const mi355rt_display_config& cfg, const mi355rt_denoise_config* dn = nullptr, float* exposure_used = nullptr) const
    {
        std::vector<uint32_t> out((size_t)mi355rt_width(h_) * mi355rt_height(h_));
        if (mi355rt_get_display_pixels(h_, &cfg, dn, out.data(), out.size(), exposure_used) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return out;
    }
    mi355rt_luminance_histogram display_histogram(uint32_t source = MI355RT_DISPLAY_SOURCE_FILM, const mi355rt_denoise_config* dn = nullptr) const
    {
        mi355rt_luminance_histogram hist{};
        if (mi355rt_display_histogram(h_, source, dn, &hist) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return hist;
    }
    // caller-supplied rays (include/mi355rt.h), host memory.  render_rays: rays6 holds width*height*spp rays, the ray of the call's
    // sample s of film pixel p at (s * npix + p) * 6; trace_rays: the radiance (n x 3) of n arbitrary rays, keys2 (n x (pixel, sampleno)) may be null
    mi355rt_ray_counts render_rays(const std::vector<float>& rays6, uint32_t spp)
    {
        mi355rt_ray_counts c{};
        if (mi355rt_render_rays(h_, rays6.data(), rays6.size() / 6, spp, MI355RT_RAYS_HOST, &c) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return c;
    }
    std::vector<float> trace_rays(const std::vector<float>& rays6, const uint32_t* keys2 = nullptr)
    {
        std::vector<float> rgb(rays6.size() / 6 * 3);
        mi355rt_ray_outputs out{};
        out.rgb = rgb.data();
        if (mi355rt_trace_rays(h_, rays6.data(), keys2, rays6.size() / 6, MI355RT_RAYS_HOST, &out) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return rgb;
    }
    // gather (include/mi355rt.h "GATHER"), host memory: light arriving at points3.size() / 3 points.  normals3 empty: sphere mode; ids empty: i.
    // The result's vectors are sized for the outputs `direct` asks for beyond n, sum and sumsq; prev non-null: accumulate onto it (cfg.accumulate is set)
    struct Gathered { std::vector<uint32_t> n; std::vector<float> sum, sumsq, direct; };
    Gathered gather(const std::vector<float>& points3, const std::vector<float>& normals3, mi355rt_gather_config cfg, bool direct = false,
                    const std::vector<uint32_t>& ids = {}, const Gathered* prev = nullptr)
    {
        const size_t np = points3.size() / 3;
        Gathered g = prev ? *prev : Gathered{};
        g.n.resize(np); g.sum.resize(np * 3); g.sumsq.resize(np * 3);
        if (direct) g.direct.resize(np * 3);
        cfg.accumulate = prev ? 1u : 0u;
        mi355rt_gather_outputs out{};
        out.n = g.n.data(); out.sum = g.sum.data(); out.sumsq = g.sumsq.data(); out.direct = direct ? g.direct.data() : nullptr;
        if (mi355rt_gather(h_, points3.data(), normals3.empty() ? nullptr : normals3.data(), ids.empty() ? nullptr : ids.data(), np, &cfg, MI355RT_RAYS_HOST, &out) != MI355RT_OK)
            throw std::runtime_error(mi355rt_last_error(h_));
        return g;
    }
    // probes (include/mi355rt.h "PROBES"), host memory.  probes_gather: n and the 9 x 3 SH sums of points3.size() / 3 probes; ids empty: i;
    // prev non-null: accumulate onto it (cfg.accumulate is set).  probes_lookup: the grid `probes` was gathered on (mi355rt_probe_grid_points) interpolated at
    // points3 and evaluated for dirs3; usable empty: every probe counts.  Returns rgb, 3 floats per query
    struct Probes { std::vector<uint32_t> n; std::vector<float> sh; };
    Probes probes_gather(const std::vector<float>& points3, mi355rt_probe_config cfg, const std::vector<uint32_t>& ids = {}, const Probes* prev = nullptr)
    {
        const size_t np = points3.size() / 3;
        Probes p = prev ? *prev : Probes{};
        p.n.resize(np); p.sh.resize(np * 27);
        cfg.accumulate = prev ? 1u : 0u;
        mi355rt_probe_outputs out{};
        out.n = p.n.data(); out.sh = p.sh.data();
        if (mi355rt_probes_gather(h_, points3.data(), ids.empty() ? nullptr : ids.data(), np, &cfg, MI355RT_RAYS_HOST, &out) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return p;
    }
    std::vector<float> probes_lookup(const mi355rt_probe_grid& grid, const Probes& probes, const std::vector<float>& points3, const std::vector<float>& dirs3,
                                     uint32_t mode = MI355RT_SH_IRRADIANCE, const std::vector<uint8_t>& usable = {})
    {
        std::vector<float> rgb(points3.size());
        if (mi355rt_probes_lookup(h_, &grid, probes.n.data(), probes.sh.data(), usable.empty() ? nullptr : usable.data(), points3.data(), dirs3.data(), points3.size() / 3, mode,
                                  MI355RT_RAYS_HOST, rgb.data(), nullptr) != MI355RT_OK)
            throw std::runtime_error(mi355rt_last_error(h_));
        return rgb;
    }
    // lens models (include/mi355rt.h): the ray generator of render(); lens_rays: the width*height*spp rays of the next render(spp), host memory
    void set_lens(const mi355rt_lens& lens) { if (mi355rt_set_lens(h_, &lens) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_)); }
    mi355rt_lens lens() const
    {
        mi355rt_lens l{};
        if (mi355rt_get_lens(h_, &l) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return l;
    }
    std::vector<float> lens_rays(uint32_t spp) const
    {
        std::vector<float> rays((size_t)mi355rt_width(h_) * mi355rt_height(h_) * spp * 6);
        if (mi355rt_lens_rays(h_, spp, MI355RT_RAYS_HOST, rays.data(), rays.size() / 6) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_));
        return rays;
    }
    // where guides(), the denoised and the display read-outs take their guides from: MI355RT_GUIDES_CENTRE (the state at creation) or MI355RT_GUIDES_FEATURES
    // mi355rt_get_relit_pixels: the frame with light li's colour scaled by weights3[li * 3 + c], mixed from the light films without tracing; display null:
    // the reference's tone map.  Returns the packed 0xAARRGGBB pixels; rgb (may be null) receives width * height * 3 floats, exposure_used the exposure applied.
    std::vector<uint32_t> get_relit_pixels(const std::vector<float>& weights3, const mi355rt_display_config* display = nullptr, std::vector<float>* rgb = nullptr,
                                           float* exposure_used = nullptr)
    {
        const size_t npix = (size_t)mi355rt_width(h_) * mi355rt_height(h_);
        std::vector<uint32_t> packed(npix);
        if (rgb) rgb->resize(npix * 3);
        if (mi355rt_get_relit_pixels(h_, weights3.data(), weights3.size(), display, rgb ? rgb->data() : nullptr, packed.data(), npix, exposure_used) != MI355RT_OK)
            throw std::runtime_error(mi355rt_last_error(h_));
        return packed;
    }
    void set_guide_source(uint32_t source) { if (mi355rt_set_guide_source(h_, source) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(h_)); }
    uint32_t guide_source() const { return mi355rt_get_guide_source(h_); }
    mi355rt_handle* handle() const { return h_; }
private:
    mi355rt_handle* h_;
};

inline mi355rt_config make_config(size_t triangles_per_leaf, size_t width, size_t height)
{
    mi355rt_config cfg;
    mi355rt_default_config(&cfg);
    cfg.triangles_per_leaf = (uint32_t)triangles_per_leaf; cfg.width = (uint32_t)width; cfg.height = (uint32_t)height;
    return cfg;
}
inline RayTracer create_raytracer(const std::string& collada_doc, size_t triangles_per_leaf, size_t width, size_t height,
                                  const mi355rt_config* cfg_override = nullptr)
{
    mi355rt_config cfg = cfg_override ? *cfg_override : make_config(triangles_per_leaf, width, height);
    mi355rt_handle* h = nullptr;
    if (mi355rt_create_from_collada_str(collada_doc.data(), collada_doc.size(), nullptr, &cfg, &h) != MI355RT_OK)
        throw std::runtime_error(mi355rt_last_error(nullptr));
    return RayTracer(h);
}
inline RayTracer create_raytracer_from_file(const std::string& collada_filename, size_t triangles_per_leaf, size_t width, size_t height,
                                            const mi355rt_config* cfg_override = nullptr)
{
    mi355rt_config cfg = cfg_override ? *cfg_override : make_config(triangles_per_leaf, width, height);
    mi355rt_handle* h = nullptr;
    const bool scene_file = collada_filename.size() > 6 && collada_filename.compare(collada_filename.size() - 6, 6, ".scene") == 0;
    int rc = scene_file ? mi355rt_create_from_scene_file(collada_filename.c_str(), &cfg, &h)
                        : mi355rt_create_from_collada_file(collada_filename.c_str(), &cfg, &h);
    if (rc != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(nullptr));
    return RayTracer(h);
}
// the ray of a pixel under a lens, host code (mi355rt_lens_ray): rot16, orient16, max_xy as mi355rt_camera_get returns them; flags bit 0: FIX_ROW_INDEX
inline std::vector<float> lens_ray(const float rot16[16], const float orient16[16], const float max_xy[2], size_t width, size_t height, uint32_t flags,
                                   const mi355rt_lens& lens, uint32_t pixel, float xi1 = 0.5f, float xi2 = 0.5f, float l1 = 0.5f, float l2 = 0.5f)
{
    std::vector<float> ray(6);
    if (mi355rt_lens_ray(rot16, orient16, max_xy, (uint32_t)width, (uint32_t)height, flags, &lens, pixel, xi1, xi2, l1, l2, ray.data()) != MI355RT_OK)
        throw std::runtime_error(mi355rt_last_error(nullptr));
    return ray;
}
// header of a film file, checked without a device (mi355rt_film_file_info): version, width, height, planes, seed low, seed high, flags, 0
inline std::vector<uint32_t> film_file_info(const std::string& path)
{
    std::vector<uint32_t> out(8);
    if (mi355rt_film_file_info(path.c_str(), out.data()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(nullptr));
    return out;
}

namespace stats {
class Stats {             // stats.rs:3-40
public:
    Stats() : last_iteration_(std::chrono::steady_clock::now()) {}
    std::string stats(uint32_t num_primary_rays)
    {
        auto now = std::chrono::steady_clock::now();
        float secs = std::chrono::duration<float>(now - last_iteration_).count();
        last_iteration_ = now;
        float fps = 1.0f / secs;
        fps_sum_ += fps;
        float prs = (float)num_primary_rays / secs;
        primrays_per_sec_sum_ += prs;
        num_measurements_ += 1;
        char buf[128];
        std::snprintf(buf, sizeof buf, "fps: %g  primary rays/s: %u", fps, (unsigned)prs);
        return buf;
    }
    std::string mean_stats() const
    {
        char buf[128];
        std::snprintf(buf, sizeof buf, "mean fps: %g  mean primary rays/s: %g", fps_sum_ / (float)num_measurements_,
                      primrays_per_sec_sum_ / (float)num_measurements_);
        return buf;
    }
private:
    std::chrono::steady_clock::time_point last_iteration_;
    float fps_sum_ = 0.0f, primrays_per_sec_sum_ = 0.0f;
    uint32_t num_measurements_ = 0;
};
}  // namespace stats

}  // namespace raytracer_lib
