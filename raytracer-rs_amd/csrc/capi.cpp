// capi.cpp — the extern "C" surface declared in include/mi355rt.h.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>
#include "display.hpp"
#include "lightmap.hpp"
#include "octree.hpp"
#include "reflmask.hpp"
#include "../../include/mi355rt.h"
#include "bake_raster.hpp"
#include "gather_walk.hpp"
#include "group.hpp"
#include "lens.hpp"
#include "renderer.hpp"
#include "sh9.hpp"
#include "oct_vis.hpp"
#include "probe_place.hpp"
#include "probe_lit_math.hpp"

using namespace mi355rt;

namespace mi355rt { bool comm_unique_id(uint8_t* id128, std::string& err); }

// A handle is a device group (csrc/group.hpp): one renderer per HIP device of this process, usually exactly one.
// `r` is the primary renderer (device 0 of the group): entry points that do not depend on the decomposition use it.
struct mi355rt_handle {
    std::unique_ptr<DeviceGroup> g;
    Renderer* r;
    std::string error;      // error text of group-level failures
};

namespace {
thread_local std::string g_create_error;

int finish_create(const SceneData& scene, const mi355rt_config* cfg, mi355rt_handle** out)
{
    int code = MI355RT_E_INVALID;
    std::string err;
    std::unique_ptr<DeviceGroup> g = DeviceGroup::create(scene, *cfg, err, code);
    if (!g) { g_create_error = err; return code; }
    Renderer* r = g->primary();
    *out = new mi355rt_handle{ std::move(g), r, std::string() };
    return MI355RT_OK;
}
int bad(const char* msg) { g_create_error = msg; return MI355RT_E_INVALID; }
// No C++ exception leaves a C entry point: what `body` throws (std::bad_alloc or std::length_error from a size a file or the caller gave)
// becomes `code` and a message, as the reference's Err(String).
template <class Body> int no_throw(const char* fn, int code, Body&& body)
{
    try { return body(); }
    catch (const std::exception& e) { g_create_error = std::string(fn) + ": " + e.what(); }
    catch (...) { g_create_error = std::string(fn) + ": unknown exception"; }
    return code;
}

// What the entries that take `where` share: they serve one device, and `where` is one of its two constants.  Null: fine, else the refusal, which the caller
// prefixes with its name.  An entry that checks `where` later, or takes none, passes MI355RT_RAYS_HOST.
const char* single_device_ok(const mi355rt_handle* h, uint32_t where)
{
    if (h->g->size() > 1) return "not available on a device group (config.device_count > 1)";
    if (where > MI355RT_RAYS_DEVICE) return "unknown `where` (MI355RT_RAYS_HOST or MI355RT_RAYS_DEVICE)";
    return nullptr;
}

// the checks of mi355rt_render_adaptive / mi355rt_adaptive_tile_mask (include/mi355rt.h); on failure the handle's last_error names the field
bool adaptive_args_ok(mi355rt_handle* h, const mi355rt_adaptive_config* c)
{
    if (!h) return false;
    const char* e = nullptr;
    if (h->g->size() > 1) e = "adaptive sampling: not available on a device group (config.device_count > 1)";
    else if (!c) e = "adaptive sampling: null config";
    else if (c->min_spp < 2) e = "adaptive sampling: min_spp must be >= 2";
    else if (c->max_spp < c->min_spp) e = "adaptive sampling: max_spp must be >= min_spp";
    else if (c->batch_spp < 1) e = "adaptive sampling: batch_spp must be >= 1";
    else if (!std::isfinite(c->rel_error) || c->rel_error < 0.0f) e = "adaptive sampling: rel_error must be finite and >= 0";
    else if (!std::isfinite(c->abs_floor) || c->abs_floor < 0.0f) e = "adaptive sampling: abs_floor must be finite and >= 0";
    if (!e) return true;
    h->r->last_error = e;
    return false;
}

// the checks shared by mi355rt_get_denoised_pixels / mi355rt_get_guides (include/mi355rt.h): one device, every row, enough room
bool denoise_handle_ok(mi355rt_handle* h, size_t npix)
{
    if (!h) return false;
    const char* e = nullptr;
    if (h->g->size() > 1) e = "denoise: not available on a device group (config.device_count > 1)";
    else if (h->r->cfg.stripe_world > 1) e = "denoise: not available on a striped handle (stripe_world > 1): a stripe's neighbours belong to other ranks";
    else if (npix < (size_t)h->r->cfg.width * h->r->cfg.height) e = "denoise: output buffer too small: npix must be >= width * height";
    if (!e) return true;
    h->r->last_error = e;
    return false;
}
bool denoise_config_ok(mi355rt_handle* h, const mi355rt_denoise_config* c)
{
    const char* e = nullptr;
    auto sigma_ok = [](float s) { return std::isfinite(s) && s > 0.0f; };
    if (!c) e = "denoise: null config";
    else if (c->iterations > 10) e = "denoise: iterations must be <= 10";
    else if (c->normal_power_log2 > 10) e = "denoise: normal_power_log2 must be <= 10";
    else if (!sigma_ok(c->sigma_luminance)) e = "denoise: sigma_luminance must be finite and > 0";
    else if (!sigma_ok(c->sigma_depth)) e = "denoise: sigma_depth must be finite and > 0";
    else if (!sigma_ok(c->sigma_albedo)) e = "denoise: sigma_albedo must be finite and > 0";
    if (!e) return true;
    h->r->last_error = e;
    return false;
}
// the checks of the display read-out (include/mi355rt.h, "ERRORS"): one device, every row; the source, and the flag the split source needs
bool display_handle_ok(mi355rt_handle* h, uint32_t source)
{
    if (!h) return false;
    const char* e = nullptr;
    if (h->g->size() > 1) e = "display: not available on a device group (config.device_count > 1)";
    else if (h->r->cfg.stripe_world > 1) e = "display: not available on a striped handle (stripe_world > 1): add the stripes into one handle first";
    else if (source > MI355RT_DISPLAY_SOURCE_DENOISED_SPLIT) e = "display: unknown source";
    else if (source == MI355RT_DISPLAY_SOURCE_DENOISED_SPLIT && !h->r->has_direct_film()) e = "display: source DENOISED_SPLIT needs a handle created with MI355RT_FLAG_DIRECT_FILM";
    if (!e) return true;
    h->r->last_error = e;
    return false;
}
// key, low, high of the auto-exposure rule; null: fine, else the message that names the field
const char* display_key_range_error(float key, float low, float high)
{
    if (!std::isfinite(key) || !(key > 0.0f)) return "display: key must be finite and > 0";
    if (!(low >= 0.0f) || !(low < 1.0f)) return "display: low must be in [0, 1) and below high";
    if (!(high > low) || !(high <= 1.0f)) return "display: high must be in (low, 1]";
    return nullptr;
}
const char* display_config_error(const mi355rt_display_config* c)
{
    auto positive = [](float s) { return std::isfinite(s) && s > 0.0f; };
    if (!c) return "display: null config";
    if (c->curve > MI355RT_CURVE_CLAMP) return "display: unknown curve";
    if (c->transfer > MI355RT_TRANSFER_SRGB) return "display: unknown transfer";
    if (c->auto_exposure > 1u) return "display: auto_exposure must be 0 or 1";
    if (!c->auto_exposure && !positive(c->exposure)) return "display: exposure must be finite and > 0";
    if (!positive(c->white)) return "display: white must be finite and > 0";
    return display_key_range_error(c->key, c->low, c->high);
}
// dn of a display entry point: ignored for the film, NULL = the default config, else validated; false: last_error names the field
bool display_denoise_config(mi355rt_handle* h, uint32_t source, const mi355rt_denoise_config* dn, mi355rt_denoise_config& out)
{
    mi355rt_denoise_default_config(&out);
    if (source == MI355RT_DISPLAY_SOURCE_FILM || !dn) return true;
    if (!denoise_config_ok(h, dn)) return false;
    out = *dn;
    return true;
}
// the checks of mi355rt_film_set / mi355rt_film_add (include/mi355rt.h); on failure the handle's last_error names the argument
bool film_put_args_ok(mi355rt_handle* h, const char* fn, const float* sum, const float* sumsq, const uint32_t* n, const float* direct, size_t npix)
{
    if (!h) return false;
    const char* e = nullptr;
    if (npix != (size_t)h->r->cfg.width * h->r->cfg.height) e = "npix must equal width * height";
    else if (!sum) e = "sum_rgb is NULL";
    else if (!sumsq) e = "sumsq_rgb is NULL";
    else if (!n) e = "n is NULL";
    else if (direct && !h->r->has_direct_film()) e = "direct_rgb given, but the handle was not created with MI355RT_FLAG_DIRECT_FILM";
    else if (!direct && h->r->has_direct_film()) e = "direct_rgb is NULL, but the handle was created with MI355RT_FLAG_DIRECT_FILM";
    if (!e) return true;
    h->r->last_error = std::string(fn) + ": " + e;
    return false;
}

// the checks of mi355rt_light_films_get / _set / _add (include/mi355rt.h, "LIGHT FILMS"); on failure the handle's last_error names the flag or the argument
bool light_films_args_ok(mi355rt_handle* h, const char* fn, const float* light_rgb, size_t nlights, size_t npix)
{
    if (!h) return false;
    const char* e = nullptr;
    if (!h->r->has_light_films()) e = "the handle was not created with MI355RT_FLAG_LIGHT_FILMS";
    else if (nlights != h->r->nlights()) e = "nlights must equal the scene's number of lights";
    else if (npix != (size_t)h->r->cfg.width * h->r->cfg.height) e = "npix must equal width * height";
    else if (nlights && !light_rgb) e = "light_rgb is NULL";
    if (!e) return true;
    h->r->last_error = std::string(fn) + ": " + e;
    return false;
}

// the guard of the read-outs built on the camera's guides (include/mi355rt.h, "CALLER-SUPPLIED RAYS"): false while the film holds caller-ray samples
bool camera_film_ok(mi355rt_handle* h, const char* fn)
{
    if (!h->r->caller_ray_film()) return true;
    h->r->last_error = std::string(fn) + ": the film holds samples of mi355rt_render_rays, which the camera's guides and tiles do not describe; mi355rt_film_clear or mi355rt_film_set first";
    return false;
}
// The guard of everything that reads guides (include/mi355rt.h, "FEATURE FILM", GUIDE SOURCE).  MI355RT_GUIDES_CENTRE: camera_film_ok for the read-outs of the
// film (film_readout), nothing for mi355rt_get_guides — what it always was.  MI355RT_GUIDES_FEATURES: the feature film must hold samples, a camera-stamped one
// of the handle's current view; a film of caller rays is served exactly when the feature film is caller-stamped.
bool guides_ok(mi355rt_handle* h, const char* fn, bool film_readout)
{
    Renderer* r = h->r;
    if (r->guide_source() != MI355RT_GUIDES_FEATURES) return !film_readout || camera_film_ok(h, fn);
    std::string e;
    if (r->feature_stamp() == Renderer::kFeatEmpty) e = "the guide source is MI355RT_GUIDES_FEATURES and the feature film is empty; mi355rt_features_render or mi355rt_features_render_rays first";
    else if (r->feature_stamp() == Renderer::kFeatCamera && !r->feature_view_current())
        e = "the feature film was accumulated under another camera, FIX_ROW_INDEX bit or lens than the handle has now; mi355rt_features_clear and accumulate again";
    else if (film_readout && r->caller_ray_film() && r->feature_stamp() != Renderer::kFeatRays)
        e = "the film holds samples of mi355rt_render_rays, which a camera's feature film does not describe; mi355rt_features_clear, then mi355rt_features_render_rays with the same rays";
    if (e.empty()) return true;
    r->last_error = std::string(fn) + ": " + e;
    return false;
}
// the checks of mi355rt_features_render / mi355rt_features_render_rays (include/mi355rt.h, "FEATURE FILM"); on failure last_error names the argument
bool features_call_ok(mi355rt_handle* h, const char* fn, bool rays, const float* rays6, size_t nrays, uint32_t spp, uint32_t where)
{
    if (!h) return false;
    Renderer* r = h->r;
    std::string e;
    if (const char* refusal = single_device_ok(h, rays ? where : MI355RT_RAYS_HOST)) e = refusal;
    else if (spp == 0) e = "spp must be >= 1";
    else if (rays && nrays != (size_t)r->cfg.width * r->cfg.height * spp) e = "nrays must equal width * height * spp";
    else if (rays && !rays6) e = "rays6 is NULL";
    else if (rays && r->feature_stamp() == Renderer::kFeatCamera) e = "the feature film holds camera samples, caller rays cannot be mixed in; mi355rt_features_clear first";
    else if (!rays && r->feature_stamp() == Renderer::kFeatRays) e = "the feature film holds caller-ray samples, camera samples cannot be mixed in; mi355rt_features_clear first";
    else if (!rays && r->feature_stamp() == Renderer::kFeatCamera && !r->feature_view_current())
        e = "the feature film was accumulated under another camera, FIX_ROW_INDEX bit or lens than the handle has now; mi355rt_features_clear first";
    if (e.empty()) return true;
    r->last_error = std::string(fn) + ": " + e;
    return false;
}
// the checks mi355rt_features_get / _alpha / _clear share: one device, a whole image
bool features_handle_ok(mi355rt_handle* h, const char* fn, bool sized, size_t npix)
{
    if (!h) return false;
    const char* e = nullptr;
    if (h->g->size() > 1) e = "not available on a device group (config.device_count > 1)";
    else if (sized && npix != (size_t)h->r->cfg.width * h->r->cfg.height) e = "npix must equal width * height";
    if (!e) return true;
    h->r->last_error = std::string(fn) + ": " + e;
    return false;
}
// the checks mi355rt_trace_rays and mi355rt_render_rays share
bool ray_call_ok(mi355rt_handle* h, const char* fn, const float* rays6, size_t n, uint32_t where)
{
    if (!h) return false;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if(n && !rays6) e = "rays6 is NULL";
    if (!e) return true;
    h->r->last_error = std::string(fn) + ": " + e;
    return false;
}

// the checks of a lens (include/mi355rt.h, "LENS MODELS"): only the fields the model reads; null: fine, else the message that names the field
const char* lens_error(const mi355rt_lens* l)
{
    if (!l) return "lens is NULL";
    if (l->model == MI355RT_LENS_PINHOLE) return nullptr;
    if (l->model == MI355RT_LENS_THIN) {
        if (!std::isfinite(l->radius) || l->radius < 0.0f) return "lens: radius must be finite and >= 0";
        if (!std::isfinite(l->focus) || !(l->focus > 0.0f)) return "lens: focus must be finite and > 0";
        return nullptr;
    }
    if (l->model == MI355RT_LENS_ORTHO) {
        if (!std::isfinite(l->width_world) || !(l->width_world > 0.0f)) return "lens: width_world must be finite and > 0";
        return nullptr;
    }
    return "lens: unknown model (MI355RT_LENS_PINHOLE, MI355RT_LENS_THIN or MI355RT_LENS_ORTHO)";
}
// the guard of the entries whose launches rest on the pinhole path (the fused 50-row frame, the adaptive sampler's tile masks): false under any other lens
bool pinhole_lens_ok(mi355rt_handle* h, const char* fn)
{
    if (!h->r->has_lens()) return true;
    h->r->last_error = std::string(fn) + ": not available under a lens other than MI355RT_LENS_PINHOLE; mi355rt_set_lens(PINHOLE) first";
    return false;
}

// ---- film files (include/mi355rt.h, "FILM FILE"): a 64-byte little-endian header, then the planes n, sum, sumsq [, direct]
constexpr size_t kFilmHeaderBytes = 64;
constexpr char kFilmMagic[9] = "MI355FLM";
struct FilmFileHeader { uint32_t version, width, height, planes; uint64_t seed; uint32_t flags; };
uint32_t get_le32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
void put_le32(unsigned char* p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }
uint64_t film_plane_bytes(const FilmFileHeader& f) { return (uint64_t)f.width * f.height * ((f.planes & 1u) ? 40u : 28u); }

// Reads and checks the header and the file's length; with `planes` also the planes (file order).  False: err names the reason.
bool read_film_file(const char* path, FilmFileHeader& f, std::vector<unsigned char>* planes, std::string& err)
{
    const std::string where = std::string("film file ") + path + ": ";
    FILE* fp = std::fopen(path, "rb");
    if (!fp) { err = where + "cannot open"; return false; }
    unsigned char hd[kFilmHeaderBytes];
    bool ok = false;
    do {
        if (std::fread(hd, 1, kFilmHeaderBytes, fp) != kFilmHeaderBytes) { err = where + "wrong file length: shorter than the 64-byte header"; break; }
        if (std::memcmp(hd, kFilmMagic, 8) != 0) { err = where + "bad magic (not a film file)"; break; }
        f.version = get_le32(hd + 8); f.width = get_le32(hd + 12); f.height = get_le32(hd + 16); f.planes = get_le32(hd + 20);
        f.seed = (uint64_t)get_le32(hd + 24) | (uint64_t)get_le32(hd + 28) << 32; f.flags = get_le32(hd + 32);
        if (f.version != 1u) { err = where + "unsupported version " + std::to_string(f.version); break; }
        if (f.planes & ~1u) { err = where + "unknown bits in the planes field"; break; }
        if (f.width == 0 || f.height == 0) { err = where + "width and height must be non-zero"; break; }
        if (std::fseek(fp, 0, SEEK_END) != 0) { err = where + "cannot seek"; break; }
        const long long len = (long long)std::ftell(fp);
        const uint64_t want = kFilmHeaderBytes + film_plane_bytes(f);
        if (len < 0 || (uint64_t)len != want) { err = where + "wrong file length: " + std::to_string(len) + " bytes, the header asks for " + std::to_string(want); break; }
        if (planes) {
            planes->resize((size_t)film_plane_bytes(f));
            if (std::fseek(fp, (long)kFilmHeaderBytes, SEEK_SET) != 0 || std::fread(planes->data(), 1, planes->size(), fp) != planes->size()) { err = where + "read error"; break; }
        }
        ok = true;
    } while (false);
    std::fclose(fp);
    return ok;
}
}  // namespace

extern "C" {

void mi355rt_default_config(mi355rt_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->width = 1024; cfg->height = 768;                         // DEFAULT_WIDTH / DEFAULT_HEIGHT, main.rs:13-14
    cfg->triangles_per_leaf = MI355RT_DEFAULT_TRIANGLES_PER_LEAF;
    cfg->recursions = 2; cfg->spread = 1;                         // mod.rs:81-82
    cfg->seed = 1; cfg->device = 0;
    cfg->stripe_rows = MI355RT_DEFAULT_STRIPE_ROWS; cfg->stripe_rank = 0; cfg->stripe_world = 1;     // 4-row stripes: measured against 8 / 2 / 1 (profiles/r02_notes.md)
    cfg->device_count = 1;
}

int mi355rt_create(const mi355rt_scene_desc* s, const mi355rt_config* cfg, mi355rt_handle** out)
{
    if (!s || !cfg || !out) return bad("null argument");
    *out = nullptr;
    if ((s->ntri && (!s->tri_verts || !s->tri_geom)) || (s->nmaterials && !s->materials) || (s->nlights && !s->lights) || (s->ntextures && !s->textures))
        return bad("null array with a non-zero count");
    return no_throw("mi355rt_create", MI355RT_E_INVALID, [&]() -> int {
        SceneData sd;
        sd.tri_verts.assign(s->tri_verts, s->tri_verts + (size_t)s->ntri * 9);
        sd.tri_geom.assign(s->tri_geom, s->tri_geom + s->ntri);
        for (uint32_t i = 0; i < s->nmaterials; ++i) {
            MaterialData m;
            m.kind = s->materials[i].kind; std::memcpy(m.rgb, s->materials[i].rgb, 12); m.tex_id = s->materials[i].tex_id;
            if (m.kind > 1) return bad("material kind must be 0 (colour) or 1 (texture)");
            sd.materials.push_back(m);
        }
        for (uint32_t i = 0; i < s->nlights; ++i) {
            LightData l;
            std::memcpy(l.pos, s->lights[i].pos, 12); std::memcpy(l.color, s->lights[i].color, 12);
            sd.lights.push_back(l);
        }
        for (uint32_t i = 0; i < s->ntextures; ++i) {
            TextureData t;
            t.width = s->textures[i].width; t.height = s->textures[i].height;
            if (!s->textures[i].rgb || !t.width || !t.height) { g_create_error = "empty texture: texture " + std::to_string(i) + " has width 0, height 0 or a NULL rgb array"; return MI355RT_E_INVALID; }
            t.rgb.assign(s->textures[i].rgb, s->textures[i].rgb + (size_t)t.width * t.height * 3);
            sd.textures.push_back(std::move(t));
        }
        CameraData c;
        std::memcpy(c.orientation, s->camera_orientation, 64); c.fov_deg = s->camera_fov_deg;
        sd.cameras.push_back(c);
        return finish_create(sd, cfg, out);
    });
}

int mi355rt_create_from_collada_str(const char* doc, size_t len, const char* data_dir, const mi355rt_config* cfg, mi355rt_handle** out)
{
    if (!doc || !cfg || !out) return bad("null argument");
    *out = nullptr;
    return no_throw("mi355rt_create_from_collada_str", MI355RT_E_LOAD, [&]() -> int {
        SceneData sd; std::string err;
        if (!load_collada_str(std::string(doc, len), data_dir, sd, err)) { g_create_error = err; return MI355RT_E_LOAD; }
        return finish_create(sd, cfg, out);
    });
}

int mi355rt_create_from_collada_file(const char* path, const mi355rt_config* cfg, mi355rt_handle** out)
{
    if (!path || !cfg || !out) return bad("null argument");
    *out = nullptr;
    return no_throw("mi355rt_create_from_collada_file", MI355RT_E_LOAD, [&]() -> int {
        SceneData sd; std::string err;
        if (!load_collada_file(path, sd, err)) { g_create_error = err; return MI355RT_E_LOAD; }
        return finish_create(sd, cfg, out);
    });
}

int mi355rt_create_from_scene_file(const char* path, const mi355rt_config* cfg, mi355rt_handle** out)
{
    if (!path || !cfg || !out) return bad("null argument");
    *out = nullptr;
    return no_throw("mi355rt_create_from_scene_file", MI355RT_E_LOAD, [&]() -> int {
        SceneData sd; std::string err;
        if (!read_scene_file(path, sd, err)) { g_create_error = err; return MI355RT_E_LOAD; }
        return finish_create(sd, cfg, out);
    });
}

void mi355rt_destroy(mi355rt_handle* h) { delete h; }

const char* mi355rt_last_error(const mi355rt_handle* h) { return h ? h->g->last_error().c_str() : g_create_error.c_str(); }

uint32_t mi355rt_trace_frame_additive(mi355rt_handle* h)
{
    if (!h || !pinhole_lens_ok(h, "mi355rt_trace_frame_additive")) return 0u;
    return h->g->trace_frame_additive();
}

int mi355rt_render(mi355rt_handle* h, uint32_t spp, mi355rt_ray_counts* counts)
{
    if (!h) return MI355RT_E_INVALID;
    bool ok = h->g->render(spp);
    if (counts) { if (h->g->size() == 1) *counts = h->r->counts; else (void)h->g->last_counts(*counts); }
    return ok ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_render_async(mi355rt_handle* h, uint32_t spp)
{
    if (!h) return MI355RT_E_INVALID;
    return h->g->render(spp, false) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_last_counts(mi355rt_handle* h, mi355rt_ray_counts* counts)
{
    if (!h || !counts) return MI355RT_E_INVALID;
    return h->g->last_counts(*counts) ? MI355RT_OK : MI355RT_E_HIP;
}

void mi355rt_adaptive_default_config(mi355rt_adaptive_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof *cfg);
    // tools/adaptive_probe.py on thai2 1920x1080: batches of 16 reach the RMSE of batches of 8 (0.01365 / 0.01372) in 18.7 ms
    // instead of 22.1 (4 rounds instead of 8); rel_error 0.03 / 0.1 and abs_floor 0.05 bought nothing better per ms
    cfg->min_spp = 16; cfg->max_spp = 64; cfg->batch_spp = 16; cfg->max_rounds = 0;
    cfg->rel_error = 0.05f; cfg->abs_floor = 0.02f;
}

int mi355rt_render_adaptive(mi355rt_handle* h, const mi355rt_adaptive_config* cfg, mi355rt_adaptive_stats* stats)
{
    if (!adaptive_args_ok(h, cfg) || !camera_film_ok(h, "mi355rt_render_adaptive") || !pinhole_lens_ok(h, "mi355rt_render_adaptive")) return MI355RT_E_INVALID;
    mi355rt_adaptive_stats st{};
    const bool ok = h->r->render_adaptive(*cfg, st);
    if (stats) *stats = st;
    return ok ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_render_tiles(mi355rt_handle* h, const uint8_t* tile_mask, size_t ntiles, uint32_t spp, uint32_t where, mi355rt_ray_counts* counts)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, MI355RT_RAYS_HOST)) != nullptr) {}       // the group first; `where` is this entry's last check
    else if (!tile_mask) e = "tile_mask is NULL";
    else if (ntiles != (size_t)h->r->tiles_x() * h->r->tiles_y()) e = "ntiles must equal tiles_x * tiles_y";
    else if (spp == 0) e = "spp must be >= 1";
    else e = single_device_ok(h, where);
    if (e) { h->r->last_error = std::string("mi355rt_render_tiles: ") + e; return MI355RT_E_INVALID; }
    const bool ok = h->r->render_tiles(tile_mask, spp, where == MI355RT_RAYS_DEVICE);
    if (counts) *counts = h->r->counts;
    return ok ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_adaptive_tile_mask(mi355rt_handle* h, const mi355rt_adaptive_config* cfg, uint8_t* out, size_t ntiles)
{
    if (!adaptive_args_ok(h, cfg)) return MI355RT_E_INVALID;
    if (!out || ntiles < (size_t)h->r->tiles_x() * h->r->tiles_y()) { h->r->last_error = "output buffer too small: tiles_x * tiles_y bytes"; return MI355RT_E_INVALID; }
    uint32_t active = 0;
    if (!h->r->adaptive_tile_mask(*cfg, out, active)) return MI355RT_E_HIP;
    return (int)active;
}

void mi355rt_denoise_default_config(mi355rt_denoise_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof *cfg);
    // tools/denoise_probe.py on thai2 1920x1080: sigma_luminance 1 instead of the first guess 4 takes 17-22 % off the tone-mapped RMSE
    // at 8 and 16 spp; the other fields' best values in the sweep bought under 5 % and are left at the first guess
    cfg->iterations = 5; cfg->normal_power_log2 = 7;
    cfg->sigma_luminance = 1.0f; cfg->sigma_depth = 0.1f; cfg->sigma_albedo = 0.1f;
}

int mi355rt_get_denoised_pixels(mi355rt_handle* h, const mi355rt_denoise_config* cfg, float* rgb, uint32_t* packed, size_t npix)
{
    if (!denoise_handle_ok(h, npix) || !denoise_config_ok(h, cfg)) return MI355RT_E_INVALID;
    if (!rgb && !packed) { h->r->last_error = "denoise: rgb and packed are both NULL"; return MI355RT_E_INVALID; }
    if (!guides_ok(h, "mi355rt_get_denoised_pixels", true)) return MI355RT_E_INVALID;
    return h->r->get_denoised(*cfg, rgb, packed) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_get_denoised_pixels_split(mi355rt_handle* h, const mi355rt_denoise_config* cfg, float* rgb, uint32_t* packed, size_t npix)
{
    if (!denoise_handle_ok(h, npix) || !denoise_config_ok(h, cfg)) return MI355RT_E_INVALID;
    if (!rgb && !packed) { h->r->last_error = "denoise: rgb and packed are both NULL"; return MI355RT_E_INVALID; }
    if (!h->r->has_direct_film()) { h->r->last_error = "denoise: the split read-out needs a handle created with MI355RT_FLAG_DIRECT_FILM"; return MI355RT_E_INVALID; }
    if (!guides_ok(h, "mi355rt_get_denoised_pixels_split", true)) return MI355RT_E_INVALID;
    return h->r->get_denoised(*cfg, rgb, packed, true) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_get_guides(mi355rt_handle* h, float* depth, float* normal3, float* albedo3, uint32_t* prim, size_t npix)
{
    if (!denoise_handle_ok(h, npix)) return MI355RT_E_INVALID;
    if (!guides_ok(h, "mi355rt_get_guides", false)) return MI355RT_E_INVALID;
    return h->r->get_guides(depth, normal3, albedo3, prim) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_features_render(mi355rt_handle* h, uint32_t spp)
{
    if (!features_call_ok(h, "mi355rt_features_render", false, nullptr, 0, spp, 0u)) return MI355RT_E_INVALID;
    return h->r->features_render(nullptr, spp, false) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_features_render_rays(mi355rt_handle* h, const float* rays6, size_t nrays, uint32_t spp, uint32_t where)
{
    if (!features_call_ok(h, "mi355rt_features_render_rays", true, rays6, nrays, spp, where)) return MI355RT_E_INVALID;
    return h->r->features_render(rays6, spp, where == MI355RT_RAYS_DEVICE) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_features_get(mi355rt_handle* h, uint32_t* n, uint32_t* hits, float* depth, float* normal3, float* albedo3, size_t npix)
{
    if (!features_handle_ok(h, "mi355rt_features_get", true, npix)) return MI355RT_E_INVALID;
    if (!n && !hits && !depth && !normal3 && !albedo3) { h->r->last_error = "mi355rt_features_get: every output pointer is NULL"; return MI355RT_E_INVALID; }
    return h->r->features_get(n, hits, depth, normal3, albedo3) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_features_clear(mi355rt_handle* h)
{
    if (!features_handle_ok(h, "mi355rt_features_clear", false, 0)) return MI355RT_E_INVALID;
    return h->r->features_clear() ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_features_alpha(mi355rt_handle* h, float* alpha, size_t npix)
{
    if (!features_handle_ok(h, "mi355rt_features_alpha", true, npix)) return MI355RT_E_INVALID;
    if (!alpha) { h->r->last_error = "mi355rt_features_alpha: alpha is NULL"; return MI355RT_E_INVALID; }
    return h->r->features_alpha(alpha) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_set_guide_source(mi355rt_handle* h, uint32_t source)
{
    if (!features_handle_ok(h, "mi355rt_set_guide_source", false, 0)) return MI355RT_E_INVALID;
    if (source > MI355RT_GUIDES_FEATURES) { h->r->last_error = "mi355rt_set_guide_source: unknown source (MI355RT_GUIDES_CENTRE or MI355RT_GUIDES_FEATURES)"; return MI355RT_E_INVALID; }
    h->r->set_guide_source(source);
    return MI355RT_OK;
}

uint32_t mi355rt_get_guide_source(const mi355rt_handle* h) { return h ? h->r->guide_source() : 0u; }

int mi355rt_light_films_get(mi355rt_handle* h, float* light_rgb, size_t nlights, size_t npix)
{
    if (!light_films_args_ok(h, "mi355rt_light_films_get", light_rgb, nlights, npix)) return MI355RT_E_INVALID;
    return h->r->light_films_get(light_rgb) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_light_films_set(mi355rt_handle* h, const float* light_rgb, size_t nlights, size_t npix)
{
    if (!light_films_args_ok(h, "mi355rt_light_films_set", light_rgb, nlights, npix)) return MI355RT_E_INVALID;
    return h->r->light_films_put(light_rgb, false) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_light_films_add(mi355rt_handle* h, const float* light_rgb, size_t nlights, size_t npix)
{
    if (!light_films_args_ok(h, "mi355rt_light_films_add", light_rgb, nlights, npix)) return MI355RT_E_INVALID;
    return h->r->light_films_put(light_rgb, true) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_get_relit_pixels(mi355rt_handle* h, const float* weights3, size_t nweights, const mi355rt_display_config* display,
                             float* rgb, uint32_t* packed, size_t npix, float* exposure_used)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if (!h->r->has_light_films()) e = "the handle was not created with MI355RT_FLAG_LIGHT_FILMS";
    else if (nweights != (size_t)h->r->nlights() * 3) e = "nweights must equal nlights * 3";
    else if (nweights && !weights3) e = "weights3 is NULL";
    else if (npix != (size_t)h->r->cfg.width * h->r->cfg.height) e = "npix must equal width * height";
    else if (!rgb && !packed) e = "rgb and packed are both NULL";
    else if (display && display->source != MI355RT_DISPLAY_SOURCE_FILM) e = "display->source must be MI355RT_DISPLAY_SOURCE_FILM: the relit image has no denoised source";
    else if (display) e = display_config_error(display);
    if (e) { h->r->last_error = std::string("mi355rt_get_relit_pixels: ") + e; return MI355RT_E_INVALID; }
    float used = 1.0f;
    if (!h->r->get_relit(weights3, display, rgb, packed, used)) return MI355RT_E_HIP;
    if (exposure_used) *exposure_used = used;
    return MI355RT_OK;
}

void mi355rt_display_default_config(mi355rt_display_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->source = MI355RT_DISPLAY_SOURCE_FILM; cfg->curve = MI355RT_CURVE_REINHARD; cfg->transfer = MI355RT_TRANSFER_REFERENCE;
    cfg->auto_exposure = 0u; cfg->exposure = 1.0f; cfg->white = 4.0f;
    cfg->key = 0.18f; cfg->low = 0.0f; cfg->high = 1.0f;
}

int mi355rt_display_histogram(mi355rt_handle* h, uint32_t source, const mi355rt_denoise_config* dn, mi355rt_luminance_histogram* out)
{
    if (!display_handle_ok(h, source)) return MI355RT_E_INVALID;
    if (!out) { h->r->last_error = "display: null histogram output"; return MI355RT_E_INVALID; }
    mi355rt_denoise_config dcfg;
    if (!display_denoise_config(h, source, dn, dcfg)) return MI355RT_E_INVALID;
    if (source != MI355RT_DISPLAY_SOURCE_FILM && !guides_ok(h, "mi355rt_display_histogram", true)) return MI355RT_E_INVALID;
    mi355rt_luminance_histogram hist;
    if (!h->r->display_histogram(source, dcfg, hist)) return MI355RT_E_HIP;
    *out = hist;
    return MI355RT_OK;
}

int mi355rt_display_auto_exposure(const mi355rt_luminance_histogram* hist, float key, float low, float high, float* exposure)
{
    if (!hist || !exposure) return bad("mi355rt_display_auto_exposure: null argument");
    if (const char* e = display_key_range_error(key, low, high)) return bad(e);
    *exposure = display_auto_exposure(*hist, key, low, high);
    return MI355RT_OK;
}

int mi355rt_display_srgb_thresholds(float out[255])
{
    if (!out) return bad("mi355rt_display_srgb_thresholds: null output");
    display_srgb_thresholds(out);
    return MI355RT_OK;
}

int mi355rt_get_display_pixels(mi355rt_handle* h, const mi355rt_display_config* cfg, const mi355rt_denoise_config* dn, uint32_t* packed, size_t npix, float* exposure_used)
{
    if (!h) return MI355RT_E_INVALID;
    if (!cfg) { h->r->last_error = "display: null config"; return MI355RT_E_INVALID; }
    if (!display_handle_ok(h, cfg->source)) return MI355RT_E_INVALID;
    const char* e = display_config_error(cfg);
    if (!e && !packed) e = "display: null packed output";
    if (!e && npix != (size_t)h->r->cfg.width * h->r->cfg.height) e = "display: npix must equal width * height";
    if (e) { h->r->last_error = e; return MI355RT_E_INVALID; }
    mi355rt_denoise_config dcfg;
    if (!display_denoise_config(h, cfg->source, dn, dcfg)) return MI355RT_E_INVALID;
    if (cfg->source != MI355RT_DISPLAY_SOURCE_FILM && !guides_ok(h, "mi355rt_get_display_pixels", true)) return MI355RT_E_INVALID;
    float used = 0.0f;
    if (!h->r->get_display(*cfg, dcfg, packed, used)) return MI355RT_E_HIP;
    if (exposure_used) *exposure_used = used;
    return MI355RT_OK;
}

int mi355rt_display_image(mi355rt_handle* h, const float* rgb3, size_t npix, const mi355rt_display_config* cfg, uint32_t* packed)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if (h->g->size() > 1) e = "not available on a device group (config.device_count > 1)";
    else if (cfg && (e = display_config_error(cfg)) != nullptr) {}
    else if (cfg && cfg->auto_exposure) e = "auto_exposure reads the histogram of a film source; an image takes a fixed exposure";
    else if (npix && !rgb3) e = "rgb3 is NULL";
    else if (npix && !packed) e = "packed is NULL";
    else if (npix > ((size_t)1 << 28)) e = "npix must be <= 2^28";
    if (e) { h->r->last_error = std::string("mi355rt_display_image: ") + e; return MI355RT_E_INVALID; }
    if (npix == 0) return MI355RT_OK;
    return h->r->display_image(rgb3, npix, cfg, packed) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_get_tonemapped_pixels(mi355rt_handle* h, uint32_t* out, size_t n)
{
    if (!h) return MI355RT_E_INVALID;
    return h->g->get_tonemapped(out, n) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_tonemap_owned_rows_device(mi355rt_handle* h, uint32_t* device_out, size_t n)
{
    if (!h) return MI355RT_E_INVALID;
    if (h->g->size() > 1) { h->r->last_error = "not available on a device group: use mi355rt_get_tonemapped_pixels"; return MI355RT_E_INVALID; }
    return h->r->tonemap_owned_rows_device(device_out, n) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_tonemap_owned_rows_device_on_stream(mi355rt_handle* h, uint32_t* device_out, size_t n, void* hip_stream)
{
    if (!h) return MI355RT_E_INVALID;
    if (!hip_stream) { h->r->last_error = "null stream: use mi355rt_tonemap_owned_rows_device"; return MI355RT_E_INVALID; }
    if (h->g->size() > 1) { h->r->last_error = "not available on a device group: use mi355rt_get_tonemapped_pixels"; return MI355RT_E_INVALID; }
    return h->r->tonemap_owned_rows_device(device_out, n, (hipStream_t)hip_stream) ? MI355RT_OK : MI355RT_E_HIP;
}

// a device group owns every row of the frame (its devices share them out among themselves)
uint32_t mi355rt_owned_rows(const mi355rt_handle* h) { return !h ? 0u : h->g->size() > 1 ? h->r->cfg.height : (uint32_t)h->r->owned_rows.size(); }

int mi355rt_owned_row_list(const mi355rt_handle* h, uint32_t* rows, size_t n)
{
    if (!h || !rows || n < mi355rt_owned_rows(h)) return MI355RT_E_INVALID;
    if (h->g->size() > 1) { for (uint32_t r = 0; r < h->r->cfg.height; ++r) rows[r] = r; return MI355RT_OK; }
    std::memcpy(rows, h->r->owned_rows.data(), h->r->owned_rows.size() * 4);
    return MI355RT_OK;
}

int mi355rt_film_get(mi355rt_handle* h, float* sum_rgb, float* sumsq_rgb, uint32_t* n)
{
    if (!h) return MI355RT_E_INVALID;
    return h->g->film_get(sum_rgb, sumsq_rgb, n) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_film_get_direct(mi355rt_handle* h, float* sum_rgb)
{
    if (!h) return MI355RT_E_INVALID;
    if (!sum_rgb) { h->r->last_error = "mi355rt_film_get_direct: null output"; return MI355RT_E_INVALID; }
    if (!h->r->has_direct_film()) { h->r->last_error = "mi355rt_film_get_direct: the handle was not created with MI355RT_FLAG_DIRECT_FILM"; return MI355RT_E_INVALID; }
    return h->g->film_get_direct(sum_rgb) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_film_clear(mi355rt_handle* h)
{
    if (!h) return MI355RT_E_INVALID;
    return h->g->film_clear() ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_film_set(mi355rt_handle* h, const float* sum_rgb, const float* sumsq_rgb, const uint32_t* n, const float* direct_rgb, size_t npix)
{
    if (!film_put_args_ok(h, "mi355rt_film_set", sum_rgb, sumsq_rgb, n, direct_rgb, npix)) return MI355RT_E_INVALID;
    return h->g->film_put({ sum_rgb, sumsq_rgb, n, direct_rgb }, false) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_film_add(mi355rt_handle* h, const float* sum_rgb, const float* sumsq_rgb, const uint32_t* n, const float* direct_rgb, size_t npix)
{
    if (!film_put_args_ok(h, "mi355rt_film_add", sum_rgb, sumsq_rgb, n, direct_rgb, npix)) return MI355RT_E_INVALID;
    return h->g->film_put({ sum_rgb, sumsq_rgb, n, direct_rgb }, true) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_film_save(mi355rt_handle* h, const char* path)
{
    if (!h) return MI355RT_E_INVALID;
    if (!path) { h->r->last_error = "mi355rt_film_save: path is NULL"; return MI355RT_E_INVALID; }
    const bool direct = h->r->has_direct_film();
    const size_t npix = (size_t)h->r->cfg.width * h->r->cfg.height;
    std::vector<uint32_t> n(npix);
    std::vector<float> sum(npix * 3), sumsq(npix * 3), dsum(direct ? npix * 3 : 0);
    if (!h->g->film_get(sum.data(), sumsq.data(), n.data()) || (direct && !h->g->film_get_direct(dsum.data()))) return MI355RT_E_HIP;
    unsigned char hd[kFilmHeaderBytes] = { 0 };
    std::memcpy(hd, kFilmMagic, 8);
    put_le32(hd + 8, 1u); put_le32(hd + 12, h->r->cfg.width); put_le32(hd + 16, h->r->cfg.height); put_le32(hd + 20, direct ? 1u : 0u);
    put_le32(hd + 24, (uint32_t)h->r->cfg.seed); put_le32(hd + 28, (uint32_t)(h->r->cfg.seed >> 32)); put_le32(hd + 32, h->r->cfg.flags);
    FILE* fp = std::fopen(path, "wb");
    bool ok = fp != nullptr;
    ok = ok && std::fwrite(hd, 1, kFilmHeaderBytes, fp) == kFilmHeaderBytes && std::fwrite(n.data(), 4, npix, fp) == npix
         && std::fwrite(sum.data(), 4, npix * 3, fp) == npix * 3 && std::fwrite(sumsq.data(), 4, npix * 3, fp) == npix * 3
         && (!direct || std::fwrite(dsum.data(), 4, npix * 3, fp) == npix * 3);
    if (fp && std::fclose(fp) != 0) ok = false;
    if (!ok) { h->r->last_error = std::string("mi355rt_film_save: cannot write ") + path; return MI355RT_E_LOAD; }
    return MI355RT_OK;
}

int mi355rt_film_load(mi355rt_handle* h, const char* path, int add)
{
    if (!h) return MI355RT_E_INVALID;
    if (!path) { h->r->last_error = "mi355rt_film_load: path is NULL"; return MI355RT_E_INVALID; }
    FilmFileHeader f{};
    std::vector<unsigned char> planes;
    std::string err;
    const mi355rt_config& c = h->r->cfg;
    if (read_film_file(path, f, &planes, err)) {
        const std::string where = std::string("film file ") + path + ": ";
        if (f.width != c.width || f.height != c.height)
            err = where + "it is " + std::to_string(f.width) + " x " + std::to_string(f.height) + ", the handle " + std::to_string(c.width) + " x " + std::to_string(c.height) + " (width / height differ)";
        else if ((f.flags ^ c.flags) & MI355RT_FLAG_FIX_ROW_INDEX) err = where + "its MI355RT_FLAG_FIX_ROW_INDEX bit differs from the handle's: the pixel -> ray mapping differs";
        else if (h->r->has_direct_film() && !(f.planes & 1u)) err = where + "it has no direct plane, the handle was created with MI355RT_FLAG_DIRECT_FILM";
    }
    if (!err.empty()) { h->r->last_error = "mi355rt_film_load: " + err; return MI355RT_E_LOAD; }
    static_assert(sizeof(float) == 4 && sizeof(uint32_t) == 4, "plane layout");
    const size_t npix = (size_t)c.width * c.height;
    // the planes in file order; a little-endian host reads them in place (planes.data() is aligned for any fundamental type)
    const uint32_t* n = reinterpret_cast<const uint32_t*>(planes.data());
    const float* sum = reinterpret_cast<const float*>(planes.data() + npix * 4);
    const float* sumsq = sum + npix * 3;
    const float* direct = h->r->has_direct_film() ? sumsq + npix * 3 : nullptr;        // a direct plane the handle has no use for is skipped
    return h->g->film_put({ sum, sumsq, n, direct }, add != 0) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_film_file_info(const char* path, uint32_t out[8])
{
    if (!path || !out) return bad("mi355rt_film_file_info: null argument");
    FilmFileHeader f{};
    std::string err;
    if (!read_film_file(path, f, nullptr, err)) { g_create_error = "mi355rt_film_file_info: " + err; return MI355RT_E_LOAD; }
    out[0] = f.version; out[1] = f.width; out[2] = f.height; out[3] = f.planes;
    out[4] = (uint32_t)f.seed; out[5] = (uint32_t)(f.seed >> 32); out[6] = f.flags; out[7] = 0u;
    return MI355RT_OK;
}

int mi355rt_film_get_pixels(mi355rt_handle* h, float* rgb)
{
    if (!h || !rgb) return MI355RT_E_INVALID;
    return h->g->film_stat(false, rgb) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_film_get_estimated_variances(mi355rt_handle* h, float* rgb)
{
    if (!h || !rgb) return MI355RT_E_INVALID;
    return h->g->film_stat(true, rgb) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_camera_move_rel(mi355rt_handle* h, float x, float y, float z)
{
    if (!h) return MI355RT_E_INVALID;
    h->g->camera_move_rel(x, y, z);
    return MI355RT_OK;
}
int mi355rt_camera_add_x_angle(mi355rt_handle* h, float radians)
{
    if (!h) return MI355RT_E_INVALID;
    h->g->camera_add_x_angle(radians);
    return MI355RT_OK;
}
int mi355rt_camera_add_y_angle(mi355rt_handle* h, float radians)
{
    if (!h) return MI355RT_E_INVALID;
    h->g->camera_add_y_angle(radians);
    return MI355RT_OK;
}
int mi355rt_camera_get(const mi355rt_handle* h, float rot16[16], float orient16[16], float max_xy[2])
{
    if (!h) return MI355RT_E_INVALID;
    if (rot16) std::memcpy(rot16, h->r->camera.rotation().e, 64);
    if (orient16) std::memcpy(orient16, h->r->camera.orientation().e, 64);
    if (max_xy) { max_xy[0] = h->r->camera.max_x(); max_xy[1] = h->r->camera.max_y(); }
    return MI355RT_OK;
}
int mi355rt_camera_get_ray(const mi355rt_handle* h, uint32_t u, uint32_t v, float xi1, float xi2, float ray6[6])
{
    if (!h || !ray6) return MI355RT_E_INVALID;
    Ray r = h->r->camera.get_ray(u, v, xi1, xi2);
    ray6[0] = r.pos.x; ray6[1] = r.pos.y; ray6[2] = r.pos.z; ray6[3] = r.dir.x; ray6[4] = r.dir.y; ray6[5] = r.dir.z;
    return MI355RT_OK;
}

int mi355rt_set_seed(mi355rt_handle* h, uint64_t seed)
{
    if (!h) return MI355RT_E_INVALID;
    return h->g->set_seed(seed) ? MI355RT_OK : MI355RT_E_HIP;
}
int mi355rt_set_flags(mi355rt_handle* h, uint32_t flags)
{
    if (!h) return MI355RT_E_INVALID;
    return h->g->set_flags(flags) ? MI355RT_OK : MI355RT_E_INVALID;
}

int mi355rt_set_slices(mi355rt_handle* h, uint32_t slices)
{
    if (!h || slices < 1 || slices > 8) return MI355RT_E_INVALID;
    h->g->set_slices(slices);
    return MI355RT_OK;
}
uint32_t mi355rt_get_slices(const mi355rt_handle* h) { return h ? h->r->slices : 0; }

int mi355rt_intersect_rays(mi355rt_handle* h, const float* rays6, size_t n, float* tuv, uint32_t* prim)
{
    if (!h || (n && (!rays6 || !tuv || !prim))) return MI355RT_E_INVALID;
    return h->r->intersect(rays6, n, tuv, prim, nullptr) ? MI355RT_OK : MI355RT_E_HIP;
}
int mi355rt_occluded_rays(mi355rt_handle* h, const float* rays6, size_t n, uint8_t* blocked)
{
    if (!h || (n && (!rays6 || !blocked))) return MI355RT_E_INVALID;
    return h->r->intersect(rays6, n, nullptr, nullptr, blocked) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_trace_rays(mi355rt_handle* h, const float* rays6, const uint32_t* keys2, size_t n, uint32_t where, const mi355rt_ray_outputs* out)
{
    if (!ray_call_ok(h, "mi355rt_trace_rays", rays6, n, where)) return MI355RT_E_INVALID;
    if (!out || (!out->rgb && !out->direct && !out->tuv && !out->prim)) { h->r->last_error = "mi355rt_trace_rays: out is NULL or every output pointer in it is NULL"; return MI355RT_E_INVALID; }
    if (n > 0xFFFFFFFFull) { h->r->last_error = "mi355rt_trace_rays: n must fit 32 bits"; return MI355RT_E_INVALID; }
    return h->r->trace_rays(rays6, keys2, n, where == MI355RT_RAYS_DEVICE, *out) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_render_rays(mi355rt_handle* h, const float* rays6, size_t nrays, uint32_t spp, uint32_t where, mi355rt_ray_counts* counts)
{
    if (!ray_call_ok(h, "mi355rt_render_rays", rays6, nrays, where)) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if (spp == 0) e = "mi355rt_render_rays: spp must be >= 1";
    else if (nrays != (size_t)h->r->cfg.width * h->r->cfg.height * spp) e = "mi355rt_render_rays: nrays must equal width * height * spp";
    if (e) { h->r->last_error = e; return MI355RT_E_INVALID; }
    const bool ok = h->r->render_rays(rays6, spp, where == MI355RT_RAYS_DEVICE);
    if (counts) *counts = h->r->counts;
    return ok ? MI355RT_OK : MI355RT_E_HIP;
}

void mi355rt_gather_default_config(mi355rt_gather_config* cfg)
{
    if (!cfg) return;
    cfg->spp = 16; cfg->first_sample = 0; cfg->weight = MI355RT_GATHER_MEAN; cfg->accumulate = 0; cfg->near_distance = INFINITY;
}

int mi355rt_gather(mi355rt_handle* h, const float* points3, const float* normals3, const uint32_t* ids, size_t npoints, const mi355rt_gather_config* cfg, uint32_t where,
                   const mi355rt_gather_outputs* out)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    const bool sampled = out && (out->n || out->hits || out->near || out->sum || out->sumsq);
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if(!cfg) e = "cfg is NULL";
    else if (!out || (!sampled && !out->direct)) e = "out is NULL or every output pointer in it is NULL";
    else if (npoints && !points3) e = "points3 is NULL";
    else if (cfg->weight > MI355RT_GATHER_COSINE) e = "unknown weight (MI355RT_GATHER_MEAN or MI355RT_GATHER_COSINE)";
    else if (cfg->weight == MI355RT_GATHER_COSINE && !normals3) e = "weight MI355RT_GATHER_COSINE needs normals3";
    else if (out->direct && !normals3) e = "the direct output needs normals3";
    else if (sampled && cfg->spp == 0) e = "spp must be >= 1 when n, hits, near, sum or sumsq is asked for";
    else if (std::isnan(cfg->near_distance)) e = "near_distance is NaN";
    else if ((uint64_t)cfg->first_sample + cfg->spp > 0xFFFFFFFFull) e = "first_sample + spp must fit 32 bits";
    else if (npoints > 0xFFFFFFFFull || (uint64_t)npoints * std::max(cfg->spp, 1u) >= (1ull << 32)) e = "npoints * spp must be < 2^32";
    if (e) { h->r->last_error = std::string("mi355rt_gather: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    return h->r->gather(points3, normals3, ids, npoints, *cfg, where == MI355RT_RAYS_DEVICE, *out) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_gather_ray(const float* table3, uint32_t seed, const float point[3], const float* normal3, uint32_t id, uint32_t sampleno, float ray6[6], uint32_t* valid)
{
    if (!table3) return bad("mi355rt_gather_ray: table3 is NULL");
    if (!point) return bad("mi355rt_gather_ray: point is NULL");
    if (!ray6) return bad("mi355rt_gather_ray: ray6 is NULL");
    GatherDir d;
    const bool ok = gather_walk([table3](uint32_t j) { GatherDir g; g.x = table3[3 * (size_t)j]; g.y = table3[3 * (size_t)j + 1]; g.z = table3[3 * (size_t)j + 2]; return g; },
                                normal3 != nullptr, normal3 ? normal3[0] : 0.0f, normal3 ? normal3[1] : 0.0f, normal3 ? normal3[2] : 0.0f, gather_start(id, sampleno, seed), d);
    gather_ray_from(point, d, ray6);
    ray6[3] = d.x; ray6[4] = d.y; ray6[5] = d.z;
    if (valid) *valid = ok ? 1u : 0u;
    return MI355RT_OK;
}

int mi355rt_bake_texels(mi355rt_handle* h, const float* uv, uint32_t width, uint32_t height, uint32_t flip, uint32_t where, const mi355rt_bake_texel_outputs* out, uint32_t* ncovered)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if(width == 0 || height == 0 || width > 16384u || height > 16384u) e = "width and height must be 1 .. 16384";
    else if (!uv && h->r->ntri) e = "uv is NULL";
    else if (!ncovered && (!out || (!out->owner && !out->bary && !out->ids && !out->points && !out->normals && !out->albedo))) e = "out is NULL or every output pointer in it is NULL, and ncovered is NULL";
    if (e) { h->r->last_error = std::string("mi355rt_bake_texels: ") + e; return MI355RT_E_INVALID; }
    const mi355rt_bake_texel_outputs none{};
    return h->r->bake_texels(uv, width, height, flip != 0, where == MI355RT_RAYS_DEVICE, out ? *out : none, ncovered) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_bake_atlas(mi355rt_handle* h, const uint32_t* ids, const float* values3, size_t n, uint32_t width, uint32_t height, uint32_t dilate, uint32_t where, float* atlas, uint8_t* valid)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if(width == 0 || height == 0 || width > 16384u || height > 16384u) e = "width and height must be 1 .. 16384";
    else if (!atlas && !valid) e = "atlas and valid are both NULL";
    else if (n && !ids) e = "ids is NULL";
    else if (n && !values3) e = "values3 is NULL";
    else if (n > (size_t)width * height) e = "more ids than the atlas has texels: one is named twice";
    if (e) { h->r->last_error = std::string("mi355rt_bake_atlas: ") + e; return MI355RT_E_INVALID; }
    uint32_t verdict = 0;
    if (!h->r->bake_atlas(ids, values3, (uint32_t)n, width, height, dilate, where == MI355RT_RAYS_DEVICE, atlas, valid, verdict)) return MI355RT_E_HIP;
    if (verdict) {
        h->r->last_error = (verdict & 1u) ? "mi355rt_bake_atlas: an id is >= width * height" : "mi355rt_bake_atlas: an id is named twice (the order of the two would decide the texel)";
        return MI355RT_E_INVALID;
    }
    return MI355RT_OK;
}

int mi355rt_bake_texel(const float uv6[6], uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t* covered, float bary2[2])
{
    if (!uv6) return bad("mi355rt_bake_texel: uv6 is NULL");
    if (!covered) return bad("mi355rt_bake_texel: covered is NULL");
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return bad("mi355rt_bake_texel: width and height must be 1 .. 16384");
    if (x >= width || y >= height) return bad("mi355rt_bake_texel: the texel is outside the atlas");
    const BakeTri t = bake_tri(uv6, width, height);
    const BakeEdges e = bake_edges(t, x, y);
    *covered = bake_in_box(t, width, height, x, y) && bake_covered(e) ? 1u : 0u;
    if (*covered && bary2) { bary2[0] = e.e1 / e.s; bary2[1] = e.e2 / e.s; }
    return MI355RT_OK;
}

float mi355rt_bake_point(float a, float e1, float e2, float u, float v) { return bake_point(a, e1, e2, u, v); }

uint32_t mi355rt_bake_dilate_texel(const float* atlas3, const uint8_t* valid, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float rgb3[3])
{
    if (!atlas3 || !valid || !rgb3 || x >= width || y >= height) return 0u;
    return bake_dilate_texel([valid](size_t i) { return valid[i] != 0; }, [atlas3](size_t i, int c) { return atlas3[3 * i + c]; }, width, height, x, y, rgb3);
}

int mi355rt_bake_auto_atlas(uint32_t ntri, uint32_t width, uint32_t height, uint32_t gutter, float* uv, uint32_t* cell)
{
    if (!uv) return bad("mi355rt_bake_auto_atlas: uv is NULL");
    if (const char* why = bake_auto_atlas(ntri, width, height, gutter, uv, cell)) { g_create_error = std::string("mi355rt_bake_auto_atlas: ") + why; return MI355RT_E_INVALID; }
    return MI355RT_OK;
}

namespace {
// The sample rules of the ray-making entries (probes_gather, probes_gather_depth, probes_survey).  between: the verdict of the entry's own config checks, which
// come after spp's and before the sizes'
const char* probe_samples_error(uint32_t spp, uint32_t first_sample, size_t npoints, const char* between)
{
    if (spp == 0) return "spp must be >= 1";
    if (between) return between;
    if ((uint64_t)first_sample + spp > 0xFFFFFFFFull) return "first_sample + spp must fit 32 bits";
    if (npoints > 0xFFFFFFFFull || (uint64_t)npoints * spp >= (1ull << 32)) return "npoints * spp must be < 2^32";
    return nullptr;
}
}  // namespace

void mi355rt_probes_default_config(mi355rt_probe_config* cfg)
{
    if (!cfg) return;
    cfg->spp = 64; cfg->first_sample = 0; cfg->accumulate = 0; cfg->near_distance = INFINITY;
}

int mi355rt_probes_gather(mi355rt_handle* h, const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_config* cfg, uint32_t where,
                          const mi355rt_probe_outputs* out)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if (!cfg) e = "cfg is NULL";
    else if (!out || (!out->n && !out->hits && !out->near && !out->sh)) e = "out is NULL or every output pointer in it is NULL";
    else if (npoints && !points3) e = "points3 is NULL";
    else e = probe_samples_error(cfg->spp, cfg->first_sample, npoints, std::isnan(cfg->near_distance) ? "near_distance is NaN" : nullptr);
    if (e) { h->r->last_error = std::string("mi355rt_probes_gather: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    return h->r->probes_gather(points3, ids, npoints, *cfg, where == MI355RT_RAYS_DEVICE, *out) ? MI355RT_OK : MI355RT_E_HIP;
}

namespace {
// the checks of a probe grid (include/mi355rt.h, "PROBES"); null: fine, else the message that names the field
const char* probe_grid_error(const mi355rt_probe_grid* g)
{
    if (!g) return "grid is NULL";
    uint64_t product = 1;
    for (int a = 0; a < 3; ++a) {
        if (g->counts[a] == 0) return "grid.counts: a count is 0";
        product *= g->counts[a];
        if (product >= (1ull << 31)) return "grid.counts: the product must be < 2^31";
    }
    for (int a = 0; a < 3; ++a) {
        if (!(std::isfinite(g->spacing[a]) && g->spacing[a] > 0.0f)) return "grid.spacing must be finite and positive";
        if (!std::isfinite(g->origin[a])) return "grid.origin must be finite";
    }
    return nullptr;
}
// defined with the entries that came with them, below
const char* probe_depth_error(const mi355rt_probe_depth* d);
const char* probe_vis_error(const mi355rt_probe_vis_config* vc, bool has_normals);
bool all_finite(const float* a, size_t n);
size_t grid_probes(const mi355rt_probe_grid* g);
// The arguments of mi355rt_probes_lookup, _vis and _placed.  weighted: the entry has depth films and a visibility config (and normals3 may back them);
// host: offsets (may be null) is host memory and is inspected
const char* probes_lookup_error(const mi355rt_handle* h, uint32_t where, const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, bool weighted, const mi355rt_probe_depth* depth,
                                const mi355rt_probe_vis_config* vc, const float* offsets, const float* points3, const float* dirs3, const float* normals3, size_t npoints, uint32_t mode,
                                const float* rgb3)
{
    if (const char* e = single_device_ok(h, where)) return e;
    if (const char* e = probe_grid_error(grid)) return e;
    if (!n) return "n is NULL";
    if (!sh) return "sh is NULL";
    if (weighted) {
        if (const char* e = probe_depth_error(depth)) return e;
        if (const char* e = probe_vis_error(vc, normals3 != nullptr)) return e;
    }
    if (!rgb3) return "rgb3 is NULL";
    if (npoints && !points3) return "points3 is NULL";
    if (npoints && !dirs3) return "dirs3 is NULL";
    if (mode > MI355RT_SH_IRRADIANCE) return "unknown mode (MI355RT_SH_RADIANCE or MI355RT_SH_IRRADIANCE)";
    if (npoints > 0xFFFFFFFFull) return "npoints must fit 32 bits";
    if (offsets && where == MI355RT_RAYS_HOST && !all_finite(offsets, grid_probes(grid) * 3)) return "offsets holds a value that is not finite";
    return nullptr;
}
// The arguments of mi355rt_probes_lookup_one, _vis_one and _placed_one
const char* probes_lookup_one_error(const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, bool weighted, const mi355rt_probe_depth* depth, const mi355rt_probe_vis_config* vc,
                                    const float* offsets, const float* point, const float* dir, const float* normal, uint32_t mode, const float* rgb)
{
    if (const char* e = probe_grid_error(grid)) return e;
    if (!n) return "n is NULL";
    if (!sh) return "sh is NULL";
    if (weighted) {
        if (const char* e = probe_depth_error(depth)) return e;
        if (const char* e = probe_vis_error(vc, normal != nullptr)) return e;
    }
    if (const char* e = !point ? "point is NULL" : !dir ? "dir is NULL" : !rgb ? "rgb is NULL" : mode > MI355RT_SH_IRRADIANCE ? "unknown mode" : nullptr) return e;
    if (offsets && !all_finite(offsets, grid_probes(grid) * 3)) return "offsets holds a value that is not finite";
    return nullptr;
}
// A probe volume in host memory as the statements of sh9.hpp read it: the accessors of the _one entries.  depth, offsets: may be null
struct HostVolume {
    ShGrid grid; const uint32_t* n; const float* sh; const uint8_t* usable; uint32_t R; size_t RR; const uint32_t* count; const float* moments; const float* offsets;
    HostVolume(const mi355rt_probe_grid* g, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth* depth, const float* offsets)
        : n(n), sh(sh), usable(usable), R(depth ? depth->res : 0u), RR((size_t)R * R), count(depth ? depth->count : nullptr), moments(depth ? depth->moments : nullptr), offsets(offsets)
    {
        std::memcpy(&grid, g, sizeof grid);
    }
    auto n_of() const { return [p = n](size_t j) { return p[j]; }; }
    auto sh_of() const { return [p = sh](size_t j, int c) { return p[27 * j + c]; }; }
    auto usable_of() const { return [p = usable](size_t j) { return p[j] != 0; }; }
    auto count_of() const { return [p = count, RR = RR](size_t j, uint32_t k) { return p[j * RR + k]; }; }
    auto moment_of() const { return [p = moments, RR = RR](size_t j, uint32_t k, int m) { return p[2 * (j * RR + k) + m]; }; }
    auto offset_of() const { return [p = offsets](size_t j, int a) { return p[3 * j + a]; }; }
};
const float kNoNormal[3] = { 0.0f, 0.0f, 0.0f };        // what a statement is handed for a normal it will not read
}  // namespace

int mi355rt_probes_lookup(mi355rt_handle* h, const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable, const float* points3, const float* dirs3,
                          size_t npoints, uint32_t mode, uint32_t where, float* rgb3, uint8_t* ok)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = probes_lookup_error(h, where, grid, n, sh, false, nullptr, nullptr, nullptr, points3, dirs3, nullptr, npoints, mode, rgb3);
    if (e) { h->r->last_error = std::string("mi355rt_probes_lookup: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    return h->r->probes_lookup(*grid, n, sh, usable, points3, dirs3, npoints, mode, where == MI355RT_RAYS_DEVICE, rgb3, ok) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_sh9_basis(const float dir[3], float b[9])
{
    if (!dir) return bad("mi355rt_sh9_basis: dir is NULL");
    if (!b) return bad("mi355rt_sh9_basis: b is NULL");
    sh9_basis(dir[0], dir[1], dir[2], b);
    return MI355RT_OK;
}

int mi355rt_probes_lookup_one(const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable, const float point[3], const float dir[3], uint32_t mode,
                              float rgb[3], uint32_t* ok)
{
    const char* e = probes_lookup_one_error(grid, n, sh, false, nullptr, nullptr, nullptr, point, dir, nullptr, mode, rgb);
    if (e) { g_create_error = std::string("mi355rt_probes_lookup_one: ") + e; return MI355RT_E_INVALID; }
    const HostVolume v(grid, n, sh, usable, nullptr, nullptr);
    const bool used = sh9_lookup(v.grid, v.n_of(), v.sh_of(), usable != nullptr, v.usable_of(), point, dir, mode, rgb);
    if (ok) *ok = used ? 1u : 0u;
    return MI355RT_OK;
}

int mi355rt_probe_grid_points(const mi355rt_probe_grid* grid, float* points3)
{
    const char* e = probe_grid_error(grid);
    if (!e && !points3) e = "points3 is NULL";
    if (e) { g_create_error = std::string("mi355rt_probe_grid_points: ") + e; return MI355RT_E_INVALID; }
    float* o = points3;
    for (uint32_t iz = 0; iz < grid->counts[2]; ++iz)
        for (uint32_t iy = 0; iy < grid->counts[1]; ++iy)
            for (uint32_t ix = 0; ix < grid->counts[0]; ++ix, o += 3) {
                o[0] = sh9_probe_pos(grid->origin[0], grid->spacing[0], ix);
                o[1] = sh9_probe_pos(grid->origin[1], grid->spacing[1], iy);
                o[2] = sh9_probe_pos(grid->origin[2], grid->spacing[2], iz);
            }
    return MI355RT_OK;
}

// ---- probe visibility (include/mi355rt.h, "PROBE VISIBILITY") ------------------------------------------------------------------------------
namespace {
// the checks of a depth film and of a visibility config; null: fine, else the message that names the field
const char* probe_depth_error(const mi355rt_probe_depth* d)
{
    if (!d) return "depth is NULL";
    if (d->res < kOctResMin || d->res > kOctResMax) return "depth.res must be 2 .. 16";
    if (!(std::isfinite(d->max_distance) && d->max_distance > 0.0f && d->max_distance <= kOctMaxDistanceTop)) return "depth.max_distance must be finite, > 0 and <= 1e12";
    if (!d->count) return "depth.count is NULL";
    if (!d->moments) return "depth.moments is NULL";
    return nullptr;
}
const char* probe_vis_error(const mi355rt_probe_vis_config* vc, bool has_normals)
{
    if (!vc) return "vc is NULL";
    if (vc->flags & ~(MI355RT_VIS_CHEBYSHEV | MI355RT_VIS_FACING)) return "vc.flags: unknown bits (MI355RT_VIS_CHEBYSHEV, MI355RT_VIS_FACING)";
    if (!std::isfinite(vc->normal_bias)) return "vc.normal_bias must be finite";
    if (!has_normals && (vc->flags & MI355RT_VIS_FACING)) return "MI355RT_VIS_FACING needs normals3, which is NULL";
    if (!has_normals && vc->normal_bias != 0.0f) return "a non-zero normal_bias needs normals3, which is NULL";
    return nullptr;
}
}  // namespace

void mi355rt_probes_vis_default_config(mi355rt_probe_vis_config* vc)
{
    if (!vc) return;
    vc->flags = MI355RT_VIS_CHEBYSHEV | MI355RT_VIS_FACING; vc->normal_bias = 0.0f;
}

int mi355rt_probes_gather_depth(mi355rt_handle* h, const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_config* cfg, uint32_t where,
                                const mi355rt_probe_outputs* out, const mi355rt_probe_depth* depth)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if (!cfg) e = "cfg is NULL";
    else if (out && !out->n && !out->hits && !out->near && !out->sh) e = "every output pointer in out is NULL (pass out as NULL for the depth film alone)";
    else if ((e = probe_depth_error(depth)) != nullptr) {}
    else if (npoints && !points3) e = "points3 is NULL";
    else e = probe_samples_error(cfg->spp, cfg->first_sample, npoints, std::isnan(cfg->near_distance) ? "near_distance is NaN" : nullptr);
    if (e) { h->r->last_error = std::string("mi355rt_probes_gather_depth: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    const mi355rt_probe_outputs none{};
    return h->r->probes_gather_depth(points3, ids, npoints, *cfg, where == MI355RT_RAYS_DEVICE, out ? *out : none, *depth) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_probes_lookup_vis(mi355rt_handle* h, const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth* depth,
                              const mi355rt_probe_vis_config* vc, const float* points3, const float* dirs3, const float* normals3, size_t npoints, uint32_t mode, uint32_t where,
                              float* rgb3, uint8_t* ok)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = probes_lookup_error(h, where, grid, n, sh, true, depth, vc, nullptr, points3, dirs3, normals3, npoints, mode, rgb3);
    if (e) { h->r->last_error = std::string("mi355rt_probes_lookup_vis: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    return h->r->probes_lookup_vis(*grid, n, sh, usable, *depth, *vc, points3, dirs3, normals3, npoints, mode, where == MI355RT_RAYS_DEVICE, rgb3, ok) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_oct_encode(const float dir[3], float uv[2])
{
    if (!dir) return bad("mi355rt_oct_encode: dir is NULL");
    if (!uv) return bad("mi355rt_oct_encode: uv is NULL");
    oct_encode(dir[0], dir[1], dir[2], uv[0], uv[1]);
    return MI355RT_OK;
}

int mi355rt_oct_texel(const float dir[3], uint32_t res, uint32_t ixy[2])
{
    if (!dir) return bad("mi355rt_oct_texel: dir is NULL");
    if (!ixy) return bad("mi355rt_oct_texel: ixy is NULL");
    if (res < kOctResMin || res > kOctResMax) return bad("mi355rt_oct_texel: res must be 2 .. 16");
    const uint32_t k = oct_texel(dir[0], dir[1], dir[2], res);
    ixy[0] = k % res; ixy[1] = k / res;
    return MI355RT_OK;
}

int mi355rt_probe_visibility_one(const mi355rt_probe_depth* depth, const float v[3], float* weight)
{
    const char* e = probe_depth_error(depth);
    if (!e) e = !v ? "v is NULL" : !weight ? "weight is NULL" : nullptr;
    if (e) { g_create_error = std::string("mi355rt_probe_visibility_one: ") + e; return MI355RT_E_INVALID; }
    const uint32_t* count = depth->count; const float* moments = depth->moments;
    *weight = oct_visibility(depth->res, [count](uint32_t k) { return count[k]; }, [moments](uint32_t k, int m) { return moments[2 * (size_t)k + m]; }, v[0], v[1], v[2],
                             oct_length(v[0], v[1], v[2]));
    return MI355RT_OK;
}

int mi355rt_probes_lookup_vis_one(const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth* depth,
                                  const mi355rt_probe_vis_config* vc, const float point[3], const float dir[3], const float normal[3], uint32_t mode, float rgb[3], uint32_t* ok)
{
    const char* e = probes_lookup_one_error(grid, n, sh, true, depth, vc, nullptr, point, dir, normal, mode, rgb);
    if (e) { g_create_error = std::string("mi355rt_probes_lookup_vis_one: ") + e; return MI355RT_E_INVALID; }
    const HostVolume v(grid, n, sh, usable, depth, nullptr);
    const bool used = sh9_lookup_vis(v.grid, v.n_of(), v.sh_of(), usable != nullptr, v.usable_of(), v.R, v.count_of(), v.moment_of(), vc->flags, vc->normal_bias, point, dir,
                                     normal != nullptr, normal ? normal : kNoNormal, mode, rgb);
    if (ok) *ok = used ? 1u : 0u;
    return MI355RT_OK;
}

void mi355rt_lens_default(mi355rt_lens* lens)
{
    if (!lens) return;
    lens->model = MI355RT_LENS_PINHOLE; lens->radius = 0.0f; lens->focus = 1.0f; lens->width_world = 0.0f;
}

int mi355rt_set_lens(mi355rt_handle* h, const mi355rt_lens* lens)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = lens_error(lens);
    if (!e && lens->model != MI355RT_LENS_PINHOLE && h->g->size() > 1) e = "mi355rt_set_lens: a lens other than MI355RT_LENS_PINHOLE is not available on a device group (config.device_count > 1)";
    if (e) { h->r->last_error = e; return MI355RT_E_INVALID; }
    return h->r->set_lens(*lens) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_get_lens(const mi355rt_handle* h, mi355rt_lens* lens)
{
    if (!h || !lens) return MI355RT_E_INVALID;
    *lens = h->r->lens();
    return MI355RT_OK;
}

int mi355rt_lens_ray(const float rot16[16], const float orient16[16], const float max_xy[2], uint32_t width, uint32_t height, uint32_t flags,
                     const mi355rt_lens* lens, uint32_t pixel, float xi1, float xi2, float l1, float l2, float ray6[6])
{
    const char* e = nullptr;
    if (!rot16) e = "mi355rt_lens_ray: rot16 is NULL";
    else if (!orient16) e = "mi355rt_lens_ray: orient16 is NULL";
    else if (!max_xy) e = "mi355rt_lens_ray: max_xy is NULL";
    else if (!ray6) e = "mi355rt_lens_ray: ray6 is NULL";
    else if (width == 0 || height == 0) e = "mi355rt_lens_ray: width and height must be non-zero";
    else if ((uint64_t)pixel >= (uint64_t)width * height) e = "mi355rt_lens_ray: pixel must be < width * height";
    else e = lens_error(lens);
    if (e) return bad(e);
    // orientation * (0, 0, 0, 1), camera.rs:88, in vecmath's operand order
    float origin[3];
    for (int k = 0; k < 3; ++k) origin[k] = 0.0f * orient16[k] + 0.0f * orient16[4 + k] + 0.0f * orient16[8 + k] + 1.0f * orient16[12 + k];
    const DLens dl = lens_derive(lens->model, lens->radius, lens->focus, lens->width_world, rot16, max_xy[0], max_xy[1], width, height);
    lens_ray(rot16, origin, max_xy[0], max_xy[1], width, height, flags, dl, pixel, xi1, xi2, l1, l2, ray6[0], ray6[1], ray6[2], ray6[3], ray6[4], ray6[5]);
    return MI355RT_OK;
}

int mi355rt_lens_rays(mi355rt_handle* h, uint32_t spp, uint32_t where, float* rays6, size_t nrays)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if (spp == 0) e = "spp must be >= 1";
    else if (nrays != (size_t)h->r->cfg.width * h->r->cfg.height * spp) e = "nrays must equal width * height * spp";
    else if (!rays6) e = "rays6 is NULL";
    if (e) { h->r->last_error = std::string("mi355rt_lens_rays: ") + e; return MI355RT_E_INVALID; }
    return h->r->lens_rays(spp, where == MI355RT_RAYS_DEVICE, rays6) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_get_sample_table(const mi355rt_handle* h, float* out)
{
    if (!h || !out) return MI355RT_E_INVALID;
    std::memcpy(out, h->r->table.data(), h->r->table.size() * sizeof(float));
    return MI355RT_OK;
}

int mi355rt_debug_sample(mi355rt_handle* h, uint32_t pixel, uint32_t sampleno, float color3[3], float* node_L, size_t nodes)
{
    if (!h || !color3 || !node_L) return MI355RT_E_INVALID;
    return h->r->debug_sample(pixel, sampleno, color3, node_L, nodes) ? MI355RT_OK : MI355RT_E_HIP;
}
int mi355rt_debug_numerics(mi355rt_handle* h, const float* a, const float* b, size_t n, float* quot, float* root, float* pow32)
{
    if (!h || (n && (!a || !b || !quot || !root || !pow32))) return MI355RT_E_INVALID;
    return h->r->debug_numerics(a, b, n, quot, root, pow32) ? MI355RT_OK : MI355RT_E_HIP;
}
int mi355rt_debug_slab(mi355rt_handle* h, const float* inv_rays6, const float* cubes6, size_t n, uint8_t* hit, float* tmin)
{
    if (!h || (n && (!inv_rays6 || !cubes6 || !hit || !tmin))) return MI355RT_E_INVALID;
    return h->r->debug_slab(inv_rays6, cubes6, n, hit, tmin) ? MI355RT_OK : MI355RT_E_HIP;
}
uint32_t mi355rt_tree_nodes(const mi355rt_handle* h) { return h ? h->r->nodes_per_sample : 0u; }
int mi355rt_debug_speculation(const mi355rt_handle* h, uint64_t out[2])
{
    if (!h || !out) return MI355RT_E_INVALID;
    h->r->speculation_stats(out);
    return MI355RT_OK;
}
int mi355rt_debug_light_map(const float* tri_verts, uint32_t ntri, const float light[3], double pad, uint32_t res, float* out_dist2, double* nearest)
{
    if ((ntri && !tri_verts) || !light || !out_dist2 || res == 0 || res > 4096 || !(pad >= 0.0)) return MI355RT_E_INVALID;
    mi355rt::LightMap lm;
    mi355rt::build_light_map(tri_verts, ntri, light, pad, res, lm);
    std::memcpy(out_dist2, lm.dist2.data(), lm.dist2.size() * sizeof(float));
    if (nearest) *nearest = lm.nearest;
    return MI355RT_OK;
}
int mi355rt_debug_reflect_mask(const float* tri_verts, uint32_t ntri, double pad, uint32_t bins, uint64_t work_budget, uint32_t* out_words, double info[8])
{
    if ((ntri && !tri_verts) || !info || !(pad >= 0.0)) return MI355RT_E_INVALID;
    mi355rt::ReflMask m;
    const double min_cos = info[4] > 0.0 ? info[4] : mi355rt::kReflMinCos, pad_angle = info[5] > 0.0 ? info[5] : mi355rt::kReflPadAngle;     // in: the census's margins
    const bool built = ntri != 0 && mi355rt::build_reflect_mask(tri_verts, ntri, pad, bins, work_budget ? work_budget : ~0ull, m, min_cos, pad_angle);
    info[0] = (double)mi355rt::refl_mask_stride(bins); info[1] = m.build_ms; info[2] = (double)m.work; info[3] = (double)m.clear_bits;
    info[4] = min_cos; info[5] = pad_angle; info[6] = (double)mi355rt::kReflBary; info[7] = built ? 1.0 : 0.0;
    if (built && out_words) std::memcpy(out_words, m.words.data(), m.words.size() * sizeof(uint32_t));
    return MI355RT_OK;
}

namespace {
// bounds of every vertex below a reference of the wide tree; counts what the walk reaches and which child boxes fail to hold their subtree
struct WideWalk {
    const mi355rt::Bvh& b; std::vector<uint32_t> seen; uint32_t children = 0, bad_boxes = 0;
    void below(int32_t ref, double mn[3], double mx[3])
    {
        for (int a = 0; a < 3; ++a) { mn[a] = 1e300; mx[a] = -1e300; }
        if (ref < 0) {
            const uint32_t code = ~(uint32_t)ref, first = code >> 3, cnt = (code & 7u) + 1u;
            for (uint32_t t = first; t < first + cnt && t < b.tris.size(); ++t) {
                const mi355rt::BvhTri& r = b.tris[t];
                if (r.prim < seen.size()) ++seen[r.prim];
                for (int v = 0; v < 3; ++v) for (int a = 0; a < 3; ++a) {
                    const double x = (double)r.v0[a] + (v == 1 ? (double)r.e1[a] : v == 2 ? (double)r.e2[a] : 0.0);
                    mn[a] = std::min(mn[a], x); mx[a] = std::max(mx[a], x);
                }
            }
            return;
        }
        const mi355rt::BvhNode4& o = b.nodes4[(size_t)ref];
        const uint32_t cbm = (o.bases & 0xFFFFFu) - 128u, nb = ~(((o.bases >> 20) | ((o.ew >> 24) << 12)) << 3);      // traverse.hpp, wide_children
        const uint32_t lo[3] = { o.lox, o.loy, o.loz }, hi[3] = { o.hix, o.hiy, o.hiz };
        for (int i = 0; i < 4; ++i) {
            if (((lo[0] >> (8 * i)) & 0xFFu) > ((hi[0] >> (8 * i)) & 0xFFu)) continue;                                  // unused slot (inverted box)
            ++children;
            const uint32_t t = (o.meta >> (8 * i)) & 0xFFu;
            const int32_t cref = (t & 0x80u) ? (int32_t)(cbm + t) : (int32_t)(nb - t);
            double cmn[3], cmx[3];
            below(cref, cmn, cmx);
            for (int a = 0; a < 3; ++a) {
                const double scale = std::ldexp(1.0, (int)((o.ew >> (8 * a)) & 0xFFu) - 127);
                const double blo = (double)o.org[a] + (double)((lo[a] >> (8 * i)) & 0xFFu) * scale, bhi = (double)o.org[a] + (double)((hi[a] >> (8 * i)) & 0xFFu) * scale;
                if (cmn[a] <= cmx[a] && (blo > cmn[a] || bhi < cmx[a])) { ++bad_boxes; break; }
                mn[a] = std::min(mn[a], cmn[a]); mx[a] = std::max(mx[a], cmx[a]);
            }
        }
    }
};
}  // namespace

int mi355rt_debug_wide_bvh(const float* tri_verts, uint32_t ntri, uint32_t out[8])
{
    if ((ntri && !tri_verts) || !out) return MI355RT_E_INVALID;
    std::vector<uint32_t> geom(std::max(ntri, 1u), 0u);
    mi355rt::Bvh b;
    mi355rt::build_bvh(tri_verts, geom.data(), ntri, b);
    mi355rt::build_wide(b);
    for (int k = 0; k < 8; ++k) out[k] = 0u;
    out[1] = (uint32_t)b.nodes.size(); out[3] = b.max_depth;
    if (b.nodes4.empty()) return MI355RT_OK;
    out[0] = (uint32_t)b.nodes4.size(); out[2] = b.stack_need4;
    WideWalk w{ b, std::vector<uint32_t>(ntri, 0u) };
    double mn[3], mx[3];
    w.below(0, mn, mx);
    out[4] = w.children; out[6] = w.bad_boxes;
    for (uint32_t c : w.seen) out[5] += c == 1u ? 1u : 0u;
    std::vector<uint32_t> seen2(ntri, 0u);
    std::vector<int32_t> st(1, b.root);
    while (!st.empty()) {
        const int32_t r = st.back(); st.pop_back();
        if (r < 0) { const uint32_t code = ~(uint32_t)r, first = code >> 3, cnt = (code & 7u) + 1u; for (uint32_t t = first; t < first + cnt && t < b.tris.size(); ++t) if (b.tris[t].prim < ntri) ++seen2[b.tris[t].prim]; }
        else { st.push_back(b.nodes[(size_t)r].child0); st.push_back(b.nodes[(size_t)r].child1); }
    }
    for (uint32_t c : seen2) out[7] += c == 1u ? 1u : 0u;
    return MI355RT_OK;
}

int mi355rt_debug_octree(const float* tri_verts, uint32_t ntri, uint32_t tris_per_leaf, uint32_t counts[8], float* cubes6, int32_t* first_child,
                         uint32_t* tri_first, uint32_t* tri_count, uint32_t* parent, size_t node_cap, uint32_t* leaf_tris, size_t leaf_cap)
{
    if ((ntri && !tri_verts) || !counts) return MI355RT_E_INVALID;
    const bool query = !cubes6 && !first_child && !tri_first && !tri_count && !parent && !leaf_tris;
    if (!query && (!cubes6 || !first_child || !tri_first || !tri_count || !parent || !leaf_tris)) return MI355RT_E_INVALID;
    mi355rt::Octree oct;
    mi355rt::build_octree(tri_verts, ntri, tris_per_leaf, oct);
    if (!query && (node_cap < oct.nodes.size() || leaf_cap < oct.leaf_tris.size())) return MI355RT_E_INVALID;      // nothing is written
    mi355rt::octree_counts(oct, counts);                                                                                // what Renderer puts into oct_stats_
    if (query) return MI355RT_OK;
    for (size_t i = 0; i < oct.nodes.size(); ++i) {
        const mi355rt::OctNodeFlat& f = oct.nodes[i];
        std::memcpy(&cubes6[6 * i], f.cmin, 3 * sizeof(float)); std::memcpy(&cubes6[6 * i + 3], f.cmax, 3 * sizeof(float));
        first_child[i] = f.first_child; tri_first[i] = f.tri_first; tri_count[i] = f.tri_count; parent[i] = f.parent;
    }
    if (!oct.leaf_tris.empty()) std::memcpy(leaf_tris, oct.leaf_tris.data(), oct.leaf_tris.size() * sizeof(uint32_t));
    return MI355RT_OK;
}

int mi355rt_debug_bvh_read(const mi355rt_handle* h, const float* tri_verts, const uint32_t* tri_geom, uint32_t ntri, uint32_t info[8], float* bounds6,
                           uint32_t* nodes8, size_t node_cap, uint32_t* tris12, size_t tri_cap)
{
    if (!info || (!h && ntri && !tri_verts)) return MI355RT_E_INVALID;
    const bool query = !nodes8 && !tris12;
    if (!query && (!nodes8 || !tris12)) return MI355RT_E_INVALID;
    mi355rt::Bvh built;
    if (!h) {
        std::vector<uint32_t> zeros;
        if (!tri_geom) { zeros.assign(std::max(ntri, 1u), 0u); tri_geom = zeros.data(); }
        mi355rt::build_bvh(tri_verts, tri_geom, ntri, built);
    }
    const Bvh& b = h ? h->r->bvh : built;
    if (!query && (node_cap < b.nodes.size() || tri_cap < b.tris.size())) return MI355RT_E_INVALID;                    // nothing is written
    info[0] = (uint32_t)b.nodes.size(); info[1] = (uint32_t)b.tris.size(); info[2] = (uint32_t)b.root; info[3] = b.leaves;
    info[4] = b.max_depth; info[5] = b.max_leaf; info[6] = info[7] = 0u;
    if (bounds6) { std::memcpy(bounds6, b.scene_min, 3 * sizeof(float)); std::memcpy(bounds6 + 3, b.scene_max, 3 * sizeof(float)); }
    if (query) return MI355RT_OK;
    static_assert(sizeof(BvhNode) == 8 * sizeof(uint32_t) && sizeof(BvhTri) == 12 * sizeof(uint32_t), "the read-out hands the structs out as words");
    if (!b.nodes.empty()) std::memcpy(nodes8, b.nodes.data(), b.nodes.size() * sizeof(BvhNode));
    if (!b.tris.empty()) std::memcpy(tris12, b.tris.data(), b.tris.size() * sizeof(BvhTri));
    return MI355RT_OK;
}

int mi355rt_accel_stats(const mi355rt_handle* h, uint32_t out[8])
{
    if (!h || !out) return MI355RT_E_INVALID;
    const Bvh& b = h->r->bvh;
    out[0] = (uint32_t)b.nodes.size(); out[1] = b.leaves; out[2] = b.max_depth; out[3] = b.max_leaf;
    out[4] = (uint32_t)(b.nodes.size() * sizeof(BvhNode)); out[5] = (uint32_t)(b.tris.size() * sizeof(BvhTri));
    out[6] = (uint32_t)(h->r->build_ms_[0] * 1000.0); out[7] = (uint32_t)(h->r->build_ms_[1] * 1000.0);
    return MI355RT_OK;
}
int mi355rt_bvh_build_info(const mi355rt_handle* h, uint32_t out[2])
{
    if (!h || !out) return MI355RT_E_INVALID;
    out[0] = h->r->bvh_on_device_ ? 1u : 0u; out[1] = (uint32_t)(h->r->lbvh_device_ms_ * 1000.0);
    return MI355RT_OK;
}
int mi355rt_debug_rays_read(const mi355rt_handle* h, uint64_t* out)
{
    if (!h || !out) return MI355RT_E_INVALID;
    *out = h->r->rays_read_;
    return MI355RT_OK;
}
int mi355rt_reflect_mask_info(const mi355rt_handle* h, double out[4])
{
    if (!h || !out) return MI355RT_E_INVALID;
    std::memcpy(out, h->r->reflect_mask_info_, sizeof h->r->reflect_mask_info_);
    return MI355RT_OK;
}
int mi355rt_octree_stats(const mi355rt_handle* h, uint32_t out[8])
{
    if (!h || !out) return MI355RT_E_INVALID;
    std::memcpy(out, h->r->oct_stats_, sizeof h->r->oct_stats_);
    return MI355RT_OK;
}
uint32_t mi355rt_device_count(const mi355rt_handle* h) { return h ? (uint32_t)h->g->size() : 0u; }

int mi355rt_debug_gather_rate(mi355rt_handle* h, uint32_t table_nodes, uint32_t steps, double out[3])
{
    if (!h || !out) return MI355RT_E_INVALID;
    return h->r->debug_gather_rate(table_nodes, steps, out) ? MI355RT_OK : MI355RT_E_HIP;
}

int64_t mi355rt_debug_check_guards(mi355rt_handle* h)
{
    if (!h) return -1;
    int64_t bad = 0;
    for (size_t i = 0; i < h->g->size(); ++i) { const long b = h->g->device(i)->check_guards(); if (b < 0) return -1; bad += b; }
    return bad;
}

uint64_t mi355rt_hbm_allocated_bytes(const mi355rt_handle* h)
{
    if (!h) return 0;
    uint64_t b = 0;
    for (size_t i = 0; i < h->g->size(); ++i) b += h->g->device(i)->hbm_allocated_bytes();
    return b;
}

int mi355rt_synchronize(mi355rt_handle* h)
{
    if (!h) return MI355RT_E_INVALID;
    return h->g->synchronize() ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_comm_unique_id(uint8_t* id128)
{
    if (!id128) return bad("null argument");
    std::string err;
    if (!comm_unique_id(id128, err)) { g_create_error = err; return MI355RT_E_HIP; }
    return MI355RT_OK;
}
int mi355rt_comm_available(mi355rt_handle* h)
{
    if (!h) return MI355RT_E_INVALID;
    if (h->g->size() > 1) { h->r->last_error = "a device group gathers inside the process; RCCL communicators are for one-device handles"; return MI355RT_E_INVALID; }
    return h->r->comm_available() ? MI355RT_OK : MI355RT_E_HIP;
}
int mi355rt_comm_init(mi355rt_handle* h, const uint8_t* id128)
{
    if (!h || !id128) return MI355RT_E_INVALID;
    if (h->g->size() > 1) { h->r->last_error = "a device group gathers inside the process; RCCL communicators are for one-device handles"; return MI355RT_E_INVALID; }
    return h->r->comm_init(id128) ? MI355RT_OK : MI355RT_E_HIP;
}
int mi355rt_comm_gather_frame(mi355rt_handle* h, uint32_t root, uint32_t* host_out, size_t n)
{
    if (!h) return MI355RT_E_INVALID;
    return h->r->comm_gather(root, host_out, n) ? MI355RT_OK : MI355RT_E_HIP;
}
int mi355rt_comm_destroy(mi355rt_handle* h)
{
    if (!h) return MI355RT_E_INVALID;
    h->r->comm_destroy();
    return MI355RT_OK;
}
uint32_t mi355rt_comm_ranks(mi355rt_handle* h) { return h ? h->r->comm_ranks() : 0u; }

uint32_t mi355rt_width(const mi355rt_handle* h) { return h ? h->r->cfg.width : 0u; }
uint32_t mi355rt_light_count(const mi355rt_handle* h) { return h ? h->r->nlights() : 0u; }
uint32_t mi355rt_height(const mi355rt_handle* h) { return h ? h->r->cfg.height : 0u; }
uint32_t mi355rt_triangle_count(const mi355rt_handle* h) { return h ? h->r->ntri : 0u; }
uint32_t mi355rt_current_row(const mi355rt_handle* h) { return h ? h->r->current_row : 0u; }

}  // extern "C"

// ---- probe placement (include/mi355rt.h, "PROBE PLACEMENT") --------------------------------------------------------------------------------
namespace {
const char* probe_max_distance_error(float D)
{
    return std::isfinite(D) && D > 0.0f && D <= kOctMaxDistanceTop ? nullptr : "max_distance must be finite, > 0 and <= 1e12";
}
// a survey's six arrays; device: the record arrays are read and written as float4
const char* probe_survey_error(const mi355rt_probe_survey* s, const char* name, bool device)
{
    static thread_local std::string msg;
    if (!s) { msg = std::string(name) + " is NULL"; return msg.c_str(); }
    const void* ptrs[6] = { s->n, s->back, s->front, s->near_back, s->near_front, s->far };
    const char* names[6] = { "n", "back", "front", "near_back", "near_front", "far" };
    for (int k = 0; k < 6; ++k) {
        if (!ptrs[k]) { msg = std::string(name) + "." + names[k] + " is NULL"; return msg.c_str(); }
        if (device && k >= 3 && ((uintptr_t)ptrs[k] & 15u)) { msg = std::string(name) + "." + names[k] + " must be 16-byte aligned in device memory"; return msg.c_str(); }
    }
    return nullptr;
}
// need_move: new_offsets or verdict is asked for; need_state: state is
const char* probe_place_error(const mi355rt_probe_place_config* c, bool need_move, bool need_state)
{
    if (!c) return "cfg is NULL";
    if (!(c->back_share >= 0.0f && c->back_share <= 1.0f)) return "cfg.back_share must be in [0, 1]";
    if (!(std::isfinite(c->max_offset) && c->max_offset >= 0.0f)) return "cfg.max_offset must be finite and >= 0";
    if (need_move && !(std::isfinite(c->min_front) && c->min_front > 0.0f)) return "cfg.min_front must be finite and > 0";
    if (need_state) if (const char* e = probe_max_distance_error(c->max_distance)) return e;
    return nullptr;
}
bool all_finite(const float* a, size_t n)
{
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
    return true;
}
size_t grid_probes(const mi355rt_probe_grid* g) { return (size_t)g->counts[0] * g->counts[1] * g->counts[2]; }
PlaceConfig place_config(const mi355rt_probe_place_config* c) { return PlaceConfig{ c->back_share, c->max_offset, c->min_front, c->max_distance }; }
}  // namespace

extern "C" {

void mi355rt_probes_survey_default_config(mi355rt_probe_survey_config* cfg)
{
    if (!cfg) return;
    cfg->spp = 64; cfg->first_sample = 0; cfg->accumulate = 0; cfg->flags = 0; cfg->max_distance = 0.0f;
}

void mi355rt_probes_place_default_config(mi355rt_probe_place_config* cfg)
{
    if (!cfg) return;
    cfg->back_share = 0.25f; cfg->max_offset = 0.45f; cfg->min_front = 0.0f; cfg->max_distance = 0.0f;
}

int mi355rt_probes_survey(mi355rt_handle* h, const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_survey_config* cfg, uint32_t where,
                          const mi355rt_probe_survey* out)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if (!cfg) e = "cfg is NULL";
    else if ((e = probe_survey_error(out, "out", where == MI355RT_RAYS_DEVICE)) != nullptr) {}
    else if (npoints && !points3) e = "points3 is NULL";
    else e = probe_samples_error(cfg->spp, cfg->first_sample, npoints,
                                 cfg->flags & ~MI355RT_SURVEY_FLIP ? "cfg.flags: unknown bits (MI355RT_SURVEY_FLIP)" : probe_max_distance_error(cfg->max_distance));
    if (e) { h->r->last_error = std::string("mi355rt_probes_survey: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    return h->r->probes_survey(points3, ids, npoints, *cfg, where == MI355RT_RAYS_DEVICE, *out) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_probes_place(mi355rt_handle* h, const mi355rt_probe_grid* grid, const mi355rt_probe_survey* survey, const mi355rt_probe_place_config* cfg, const float* offsets,
                         uint32_t where, float* new_offsets, uint8_t* verdict, uint8_t* state)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if ((e = probe_grid_error(grid)) != nullptr) {}
    else if ((e = probe_survey_error(survey, "survey", where == MI355RT_RAYS_DEVICE)) != nullptr) {}
    else if (!new_offsets && !verdict && !state) e = "new_offsets, verdict and state are all NULL";
    else if ((e = probe_place_error(cfg, new_offsets || verdict, state != nullptr)) != nullptr) {}
    else if (offsets && where == MI355RT_RAYS_HOST && !all_finite(offsets, grid_probes(grid) * 3)) e = "offsets holds a value that is not finite";
    if (e) { h->r->last_error = std::string("mi355rt_probes_place: ") + e; return MI355RT_E_INVALID; }
    return h->r->probes_place(*grid, *survey, *cfg, offsets, where == MI355RT_RAYS_DEVICE, new_offsets, verdict, state) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_probe_place_one(const mi355rt_probe_grid* grid, const mi355rt_probe_place_config* cfg, const uint32_t counts3[3], const float records12[12], const float offset[3],
                            float new_offset[3], uint32_t* verdict, uint32_t* state)
{
    const char* e = probe_grid_error(grid);
    if (!e) e = !counts3 ? "counts3 is NULL" : !records12 ? "records12 is NULL" : !new_offset && !verdict && !state ? "new_offset, verdict and state are all NULL" : nullptr;
    if (!e) e = probe_place_error(cfg, new_offset || verdict, state != nullptr);
    if (!e && offset && !all_finite(offset, 3)) e = "offset holds a value that is not finite";
    if (e) { g_create_error = std::string("mi355rt_probe_place_one: ") + e; return MI355RT_E_INVALID; }
    const float* r = records12;
    const SurveyState s{ counts3[0], counts3[1], counts3[2], { r[0], r[1], r[2], r[3] }, { r[4], r[5], r[6], r[7] }, { r[8], r[9], r[10], r[11] } };
    const PlaceConfig pc = place_config(cfg);
    if (state) *state = place_state(s, pc);
    if (new_offset || verdict) {
        const float zero[3] = { 0.0f, 0.0f, 0.0f };
        float out[3];
        const uint32_t v = place_one(s, offset ? offset : zero, grid->spacing, grid->counts, pc, out);
        if (new_offset) { new_offset[0] = out[0]; new_offset[1] = out[1]; new_offset[2] = out[2]; }
        if (verdict) *verdict = v;
    }
    return MI355RT_OK;
}

int mi355rt_probes_lookup_placed(mi355rt_handle* h, const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth* depth,
                                 const mi355rt_probe_vis_config* vc, const float* offsets, const float* points3, const float* dirs3, const float* normals3, size_t npoints,
                                 uint32_t mode, uint32_t where, float* rgb3, uint8_t* ok)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = probes_lookup_error(h, where, grid, n, sh, true, depth, vc, offsets, points3, dirs3, normals3, npoints, mode, rgb3);
    if (e) { h->r->last_error = std::string("mi355rt_probes_lookup_placed: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    return h->r->probes_lookup_placed(*grid, n, sh, usable, *depth, *vc, offsets, points3, dirs3, normals3, npoints, mode, where == MI355RT_RAYS_DEVICE, rgb3, ok) ? MI355RT_OK
                                                                                                                                                                  : MI355RT_E_HIP;
}

int mi355rt_probes_lookup_placed_one(const mi355rt_probe_grid* grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth* depth,
                                     const mi355rt_probe_vis_config* vc, const float* offsets, const float point[3], const float dir[3], const float normal[3], uint32_t mode,
                                     float rgb[3], uint32_t* ok)
{
    const char* e = probes_lookup_one_error(grid, n, sh, true, depth, vc, offsets, point, dir, normal, mode, rgb);
    if (e) { g_create_error = std::string("mi355rt_probes_lookup_placed_one: ") + e; return MI355RT_E_INVALID; }
    const HostVolume v(grid, n, sh, usable, depth, offsets);
    const bool used = sh9_lookup_placed(v.grid, v.n_of(), v.sh_of(), usable != nullptr, v.usable_of(), v.R, v.count_of(), v.moment_of(), offsets != nullptr, v.offset_of(), vc->flags,
                                        vc->normal_bias, point, dir, normal != nullptr, normal ? normal : kNoNormal, mode, rgb);
    if (ok) *ok = used ? 1u : 0u;
    return MI355RT_OK;
}

}  // extern "C"

// ---- probe-lit shading (include/mi355rt.h, "PROBE-LIT") ------------------------------------------------------------------------------------
namespace {
// host: the volume's arrays are host memory, and its offsets are inspected
const char* probe_volume_error(const mi355rt_probe_volume* v, bool host)
{
    if (!v) return "volume is NULL";
    if (const char* e = probe_grid_error(v->grid)) return e;
    if (!v->n) return "volume.n is NULL";
    if (!v->sh) return "volume.sh is NULL";
    if (!v->depth) {
        if (v->vc) return "volume.vc is given without volume.depth";
        if (v->offsets) return "volume.offsets is given without volume.depth";
        return nullptr;
    }
    if (const char* e = probe_depth_error(v->depth)) return e;
    if (const char* e = probe_vis_error(v->vc, true)) return e;
    if (v->offsets && host && !all_finite(v->offsets, grid_probes(v->grid) * 3)) return "volume.offsets holds a value that is not finite";
    return nullptr;
}
}  // namespace

extern "C" {

int mi355rt_probe_lit_points(mi355rt_handle* h, const mi355rt_probe_volume* volume, const float* points3, const float* normals3, size_t npoints, uint32_t flags, uint32_t where,
                             float* indirect3, uint8_t* ok)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if ((e = probe_volume_error(volume, where == MI355RT_RAYS_HOST)) != nullptr) {}
    else if (flags & ~MI355RT_PROBE_LIT_CLAMP) e = "flags: unknown bits (MI355RT_PROBE_LIT_CLAMP)";
    else if (!indirect3) e = "indirect3 is NULL";
    else if (npoints && !points3) e = "points3 is NULL";
    else if (npoints && !normals3) e = "normals3 is NULL";
    else if (npoints > 0xFFFFFFFFull) e = "npoints must fit 32 bits";
    if (e) { h->r->last_error = std::string("mi355rt_probe_lit_points: ") + e; return MI355RT_E_INVALID; }
    if (npoints == 0) return MI355RT_OK;
    return h->r->probe_lit_points(*volume, points3, normals3, npoints, flags, where == MI355RT_RAYS_DEVICE, indirect3, ok) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_probe_lit_rays(mi355rt_handle* h, const mi355rt_probe_volume* volume, const float* rays6, size_t nrays, uint32_t flags, uint32_t where,
                           const mi355rt_probe_lit_outputs* out)
{
    if (!h) return MI355RT_E_INVALID;
    const char* e = nullptr;
    if ((e = single_device_ok(h, where)) != nullptr) {}
    else if ((e = probe_volume_error(volume, where == MI355RT_RAYS_HOST)) != nullptr) {}
    else if (flags & ~MI355RT_PROBE_LIT_CLAMP) e = "flags: unknown bits (MI355RT_PROBE_LIT_CLAMP)";
    else if (!out || (!out->rgb && !out->light && !out->indirect && !out->tuv && !out->prim && !out->ok)) e = "out is NULL or every output pointer in it is NULL";
    else if (nrays && !rays6) e = "rays6 is NULL";
    else if (nrays > 0xFFFFFFFFull || (uint64_t)nrays * std::max(h->r->nlights(), 1u) >= (1ull << 32)) e = "nrays * max(nlights, 1) must be < 2^32";
    if (e) { h->r->last_error = std::string("mi355rt_probe_lit_rays: ") + e; return MI355RT_E_INVALID; }
    if (nrays == 0) return MI355RT_OK;
    return h->r->probe_lit_rays(*volume, rays6, nrays, flags, where == MI355RT_RAYS_DEVICE, *out) ? MI355RT_OK : MI355RT_E_HIP;
}

int mi355rt_probe_lit_one(const mi355rt_probe_volume* volume, const float point[3], const float normal[3], uint32_t flags, float indirect[3], uint32_t* ok)
{
    const char* e = probe_volume_error(volume, true);
    if (!e) e = flags & ~MI355RT_PROBE_LIT_CLAMP ? "flags: unknown bits (MI355RT_PROBE_LIT_CLAMP)" : !point ? "point is NULL" : !normal ? "normal is NULL" : !indirect ? "indirect is NULL" : nullptr;
    if (e) { g_create_error = std::string("mi355rt_probe_lit_one: ") + e; return MI355RT_E_INVALID; }
    const HostVolume v(volume->grid, volume->n, volume->sh, volume->usable, volume->depth, volume->offsets);
    const bool used = hemi_one(v.grid, v.n_of(), v.sh_of(), v.usable != nullptr, v.usable_of(), v.R, v.count_of(), v.moment_of(), v.offsets != nullptr, v.offset_of(),
                               volume->depth ? volume->vc->flags : 0u, volume->depth ? volume->vc->normal_bias : 0.0f, point, normal, (flags & MI355RT_PROBE_LIT_CLAMP) != 0, indirect);
    if (ok) *ok = used ? 1u : 0u;
    return MI355RT_OK;
}

}  // extern "C"
