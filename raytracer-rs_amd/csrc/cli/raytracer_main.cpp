// raytracer — headless counterpart of the reference's `raytracer` binary (raytracer/src/main.rs).
// Same flags and defaults (main.rs:13-15, 26-99: -f/--file, -m/--max_triangles, -i/--frame_iterations,
// --width, --height; unparsable numbers silently fall back to the defaults) and the same loop
// (main.rs:197-216: trace_frame_additive -> get_tonemapped_pixels -> print stats), with the window
// replaced by an optional image file.  Additions: --spp N (whole frames of N samples per pixel through
// mi355rt_render instead of the 50-row calls), --seed S, --gpus N (a device group: the N GPUs of this process share the
// rows, mi355rt_config.device_count), --out file.ppm | file.png, --fix-row-index, and adaptive sampling in place of --spp:
// --adaptive REL (mi355rt_render_adaptive with rel_error REL) with --abs-floor F, --min-spp N, --max-spp N, --batch N (defaults:
// mi355rt_adaptive_default_config), and --denoise: --out receives the denoised read-out of the film (mi355rt_get_denoised_pixels,
// mi355rt_denoise_default_config) instead of get_tonemapped_pixels; --denoise-split: the handle keeps a direct film (MI355RT_FLAG_DIRECT_FILM)
// and --out receives the split read-out (mi355rt_get_denoised_pixels_split), which filters the indirect part only.  Film files (mi355rt_film_load /
// mi355rt_film_save): --load-film PATH (repeatable) adds each file to the fresh zero film before any rendering, --save-film PATH writes the film
// after rendering and before the read-out; with --load-film and -i 0 nothing is rendered and the loaded film is read out once (a merge-only run).
// Display read-out (mi355rt_get_display_pixels, defaults: mi355rt_display_default_config): any of --exposure F, --auto-exposure, --key F,
// --curve reinhard|reinhard-white|aces|clamp, --white F, --srgb sends the written frame through it, with the source --denoise / --denoise-split select (the
// film without them), and prints the exposure used; --exposure together with --auto-exposure is an error.  Without them --out holds the bytes it always held.
// Caller-supplied rays (mi355rt_render_rays): --ortho-width W with --spp N renders the scene in parallel projection, W world units wide, through rays made
// here (ortho_rays below: the arithmetic of raytracer_rs_amd.cameras.orthographic, so both paths write the same bytes).
// Lens models (mi355rt_set_lens): --lens thin --lens-radius R --focus F (depth of field) and --lens ortho --lens-width W (parallel projection), with --spp N:
// the rays are made on the device, so --denoise, --denoise-split, the film files and the display options all apply; they exclude --adaptive, --gpus and -i.
// Tiles (mi355rt_render_tiles): --region X0,Y0,X1,Y1 with --spp N renders only the tiles the half-open pixel rectangle touches; --refine REL runs the adaptive
// loop on this side (RayTracer::refine: mi355rt_adaptive_tile_mask, then mi355rt_render_tiles) with --abs-floor, --min-spp, --max-spp and --batch as --adaptive
// takes them, and prints the line --adaptive prints.  Both work with --lens (--refine is adaptive sampling's way under a lens) and exclude --gpus, -i and --adaptive;
// --refine excludes --spp.
// Feature film (mi355rt_features_render): --features N accumulates N feature samples after the render — under --ortho-width along the rays an N-sample
// orthographic render of a cleared film takes (the render's own rays when N equals --spp), through mi355rt_features_render_rays.  --denoise-guides centre|features
// selects where --denoise / --denoise-split and the display options take their guides from (mi355rt_set_guide_source; features needs --features, and lifts the
// exclusion of --denoise under --ortho-width).  --alpha (needs --features and a .png --out) writes an RGBA PNG: the RGB bytes are what they would be without the
// option, A = (uint32_t)(alpha * 255.0f + 0.5f) of mi355rt_features_alpha; the colour is premultiplied by construction, because a miss is black.
// Light films (MI355RT_FLAG_LIGHT_FILMS): --light-films keeps a film per light; --relight W0,W1,... writes the frame with light i scaled by Wi to --out
// (mi355rt_get_relit_pixels, no tracing; the display options apply); --out-lights PREFIX writes PREFIX<i>.png, light i alone at weight 1.
// Bake (mi355rt_bake_texels, mi355rt_gather, mi355rt_bake_atlas): --bake W,H with --spp N and --out writes a lightmap instead of a frame: the auto
// atlas (mi355rt_bake_auto_atlas, gutter 1) of W x H texels, N gather samples per covered texel, radiance = albedo * direct + sum / n, --bake-dilate K (default 2)
// dilation steps, packed by mi355rt_display_image under the display options (without them: the reference's tone map).  --bake-uv-out FILE also writes the UVs,
// ntri x 6 floats, raw little-endian f32.  --auto-exposure is refused (an atlas has no film histogram), as is everything that renders or reads a frame.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <zlib.h>
#include "../raytracer_lib.hpp"

// 8-bit RGB PNG (alpha == nullptr) or RGBA PNG (one alpha byte per pixel): one IDAT chunk, filter type 0 on every scanline
static bool write_png(const std::string& path, const std::vector<uint32_t>& argb, size_t width, size_t height, const std::vector<unsigned char>* alpha = nullptr)
{
    std::vector<unsigned char> raw;
    raw.reserve((width * (alpha ? 4 : 3) + 1) * height);
    for (size_t y = 0; y < height; ++y) {
        raw.push_back(0);
        for (size_t x = 0; x < width; ++x) {
            uint32_t p = argb[y * width + x]; raw.push_back((unsigned char)(p >> 16)); raw.push_back((unsigned char)(p >> 8)); raw.push_back((unsigned char)p);
            if (alpha) raw.push_back((*alpha)[y * width + x]);
        }
    }
    uLongf clen = compressBound((uLong)raw.size());
    std::vector<unsigned char> comp(clen);
    if (compress2(comp.data(), &clen, raw.data(), (uLong)raw.size(), 6) != Z_OK) return false;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    auto be32 = [](unsigned char* b, uint32_t v) { b[0] = (unsigned char)(v >> 24); b[1] = (unsigned char)(v >> 16); b[2] = (unsigned char)(v >> 8); b[3] = (unsigned char)v; };
    auto chunk = [&](const char* type, const unsigned char* data, uint32_t len) {
        unsigned char hdr[8]; be32(hdr, len); std::memcpy(hdr + 4, type, 4);
        std::fwrite(hdr, 1, 8, f);
        if (len) std::fwrite(data, 1, len, f);
        uLong crc = crc32(0L, (const Bytef*)type, 4);
        if (len) crc = crc32(crc, data, len);
        unsigned char c[4]; be32(c, (uint32_t)crc); std::fwrite(c, 1, 4, f);
    };
    static const unsigned char sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
    std::fwrite(sig, 1, 8, f);
    unsigned char ihdr[13]; be32(ihdr, (uint32_t)width); be32(ihdr + 4, (uint32_t)height);
    ihdr[8] = 8; ihdr[9] = alpha ? 6 : 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;          // 8 bit, colour type 2 (RGB) or 6 (RGBA)
    chunk("IHDR", ihdr, 13);
    chunk("IDAT", comp.data(), (uint32_t)clen);
    chunk("IEND", nullptr, 0);
    return std::fclose(f) == 0;
}

// pcg4d (Jarzynski & Olano, JCGT 2020) and the 23-bit uniform float, as csrc/device_math.hpp runs them
static void pcg4d(uint32_t& x, uint32_t& y, uint32_t& z, uint32_t& w)
{
    x = x * 1664525u + 1013904223u; y = y * 1664525u + 1013904223u; z = z * 1664525u + 1013904223u; w = w * 1664525u + 1013904223u;
    x += y * w; y += z * x; z += x * y; w += y * z;
    x ^= x >> 16; y ^= y >> 16; z ^= z >> 16; w ^= w >> 16;
    x += y * w; y += z * x; z += x * y; w += y * z;
}
static float u01(uint32_t bits) { return (float)(bits >> 9) * (1.0f / 8388608.0f); }

// The rays of an orthographic view in mi355rt_render_rays layout: cameras.orthographic of the Python package, expression for expression (f32, unfused:
// this file is compiled with -ffp-contract=off).  rot, orient: mi355rt_camera_get; film_n: the film's sample counts before the call.
static std::vector<float> ortho_rays(const float rot[16], const float orient[16], size_t width, size_t height, size_t spp, uint32_t seed, float width_world,
                                     const std::vector<uint32_t>& film_n)
{
    const size_t npix = width * height;
    std::vector<float> rays(npix * spp * 6);
    float origin[3], axis[3];
    for (int k = 0; k < 3; ++k) {
        origin[k] = 0.0f * orient[k] + 0.0f * orient[4 + k] + 0.0f * orient[8 + k] + 1.0f * orient[12 + k];
        axis[k] = rot[8 + k] + rot[12 + k];
    }
    const float hw = width_world * 0.5f;
    const float hh = hw * ((float)height / (float)width);
    for (size_t s = 0; s < spp; ++s)
        for (size_t p = 0; p < npix; ++p) {
            uint32_t h0 = (uint32_t)p, h1 = film_n[p] + (uint32_t)s, h2 = 0u, h3 = seed;
            pcg4d(h0, h1, h2, h3);
            const float cu = (float)(uint32_t)(p % width), cv = (float)(uint32_t)(p / width);
            const float sx = -hw + (2.0f * hw) * ((cu + u01(h0)) / (float)width);
            const float sy = -hh + (2.0f * hh) * ((cv + u01(h1)) / (float)height);
            float* r = &rays[(s * npix + p) * 6];
            for (int k = 0; k < 3; ++k) { r[k] = (origin[k] + sx * rot[k]) + (-sy) * rot[4 + k]; r[3 + k] = axis[k]; }
        }
    return rays;
}

static bool parse_usize(const char* s, size_t& out)
{
    if (!s || !*s) return false;
    char* end = nullptr;
    unsigned long long v = std::strtoull(s, &end, 10);
    if (*end != '\0' || s[0] == '-') return false;
    out = (size_t)v;
    return true;
}

int main(int argc, char** argv)
{
    const size_t DEFAULT_WIDTH = 1024, DEFAULT_HEIGHT = 768;          // main.rs:13-14
    std::string file = "./data/thai2.dae";                           // main.rs:15
    size_t max_triangles = raytracer_lib::DEFAULT_TRIANGLES_PER_LEAF, width = DEFAULT_WIDTH, height = DEFAULT_HEIGHT;
    size_t frame_iterations = 0, spp = 0, seed = 1, gpus = 1;
    bool have_iterations = false, fix_row = false, share_device = false, device_lbvh = false;
    std::string out, save_film;
    std::vector<std::string> load_films;
    bool adaptive = false, denoise = false, denoise_split = false;
    mi355rt_adaptive_config acfg;
    mi355rt_adaptive_default_config(&acfg);
    bool display = false, have_exposure = false, ortho = false;
    float ortho_width = 0.0f;
    mi355rt_display_config dcfg_display;
    mi355rt_display_default_config(&dcfg_display);
    mi355rt_lens lens;
    mi355rt_lens_default(&lens);
    bool have_lens = false, have_region = false, refine = false;
    long long region[4] = { 0, 0, 0, 0 };
    size_t features = 0;
    bool guides_features = false, alpha = false;
    bool light_films = false, have_relight = false;
    std::vector<float> relight;
    std::string out_lights;
    bool have_bake = false;
    unsigned long long bake_w = 0, bake_h = 0;
    size_t bake_dilate = 2;
    std::string bake_uv_out;
    auto parse_float = [](const char* s, float& out) { if (!s || !*s) return false; char* end = nullptr; const float f = std::strtof(s, &end); if (*end != '\0' || !std::isfinite(f)) return false; out = f; return true; };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
        auto take = [&]() { ++i; return v; };
        if (a == "-f" || a == "--file") { if (v) file = take(); }
        else if (a == "-m" || a == "--max_triangles") { size_t t; if (parse_usize(take(), t)) max_triangles = t; }
        else if (a == "-i" || a == "--frame_iterations") { size_t t; if (parse_usize(take(), t)) { frame_iterations = t; have_iterations = true; } }
        else if (a == "--width") { size_t t; if (parse_usize(take(), t)) width = t; }
        else if (a == "--height") { size_t t; if (parse_usize(take(), t)) height = t; }
        else if (a == "--spp") { size_t t; if (parse_usize(take(), t)) spp = t; }
        else if (a == "--seed") { size_t t; if (parse_usize(take(), t)) seed = t; }
        else if (a == "--gpus") { size_t t; if (parse_usize(take(), t) && t >= 1) gpus = t; }
        else if (a == "--share-device") share_device = true;
        else if (a == "--out") { if (v) out = take(); }
        else if (a == "--load-film") { if (v) load_films.push_back(take()); }
        else if (a == "--save-film") { if (v) save_film = take(); }
        else if (a == "--fix-row-index") fix_row = true;
        else if (a == "--device-lbvh") device_lbvh = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-split") denoise_split = true;
        else if (a == "--exposure") { float f; if (parse_float(take(), f)) { dcfg_display.exposure = f; display = have_exposure = true; } }
        else if (a == "--auto-exposure") { dcfg_display.auto_exposure = 1u; display = true; }
        else if (a == "--key") { float f; if (parse_float(take(), f)) { dcfg_display.key = f; display = true; } }
        else if (a == "--white") { float f; if (parse_float(take(), f)) { dcfg_display.white = f; display = true; } }
        else if (a == "--srgb") { dcfg_display.transfer = MI355RT_TRANSFER_SRGB; display = true; }
        else if (a == "--curve") {
            const std::string c = v ? take() : "";
            if (c == "reinhard") dcfg_display.curve = MI355RT_CURVE_REINHARD;
            else if (c == "reinhard-white") dcfg_display.curve = MI355RT_CURVE_REINHARD_WHITE;
            else if (c == "aces") dcfg_display.curve = MI355RT_CURVE_ACES;
            else if (c == "clamp") dcfg_display.curve = MI355RT_CURVE_CLAMP;
            else { std::fprintf(stderr, "Error: --curve takes reinhard, reinhard-white, aces or clamp\n"); return 1; }
            display = true;
        }
        else if (a == "--ortho-width") { float f; if (parse_float(take(), f) && f > 0.0f) { ortho_width = f; ortho = true; } }
        else if (a == "--lens") {
            const std::string m = v ? take() : "";
            if (m == "thin") lens.model = MI355RT_LENS_THIN;
            else if (m == "ortho") lens.model = MI355RT_LENS_ORTHO;
            else if (m == "pinhole") lens.model = MI355RT_LENS_PINHOLE;
            else { std::fprintf(stderr, "Error: --lens takes pinhole, thin or ortho\n"); return 1; }
            have_lens = lens.model != MI355RT_LENS_PINHOLE;
        }
        else if (a == "--lens-radius") { float f; if (parse_float(take(), f)) lens.radius = f; }
        else if (a == "--focus") { float f; if (parse_float(take(), f)) lens.focus = f; }
        else if (a == "--lens-width") { float f; if (parse_float(take(), f)) lens.width_world = f; }
        else if (a == "--features") { size_t t; if (parse_usize(take(), t)) features = t; }
        else if (a == "--denoise-guides") {
            const std::string g = v ? take() : "";
            if (g == "features") guides_features = true;
            else if (g == "centre") guides_features = false;
            else { std::fprintf(stderr, "Error: --denoise-guides takes centre or features\n"); return 1; }
        }
        else if (a == "--alpha") alpha = true;
        else if (a == "--light-films") light_films = true;
        else if (a == "--out-lights") { if (v) out_lights = take(); }
        else if (a == "--relight") {
            const char* r = take();
            std::string tok;
            for (const char* c = r ? r : ""; ; ++c) {
                if (*c != ',' && *c != '\0') { tok += *c; continue; }
                float f;
                if (!parse_float(tok.c_str(), f)) { std::fprintf(stderr, "Error: --relight takes W0,W1,...: one finite factor per light\n"); return 1; }
                relight.push_back(f); tok.clear();
                if (*c == '\0') break;
            }
            have_relight = true;
        }
        else if (a == "--bake") {
            const char* r = take();
            char tail = 0;
            if (!r || std::sscanf(r, "%llu,%llu%c", &bake_w, &bake_h, &tail) != 2 || r[0] == '-') { std::fprintf(stderr, "Error: --bake takes W,H\n"); return 1; }
            have_bake = true;
        }
        else if (a == "--bake-dilate") { size_t t; if (parse_usize(take(), t)) bake_dilate = t; }
        else if (a == "--bake-uv-out") { if (v) bake_uv_out = take(); }
        else if (a == "--refine") { float f; if (parse_float(take(), f)) { acfg.rel_error = f; refine = true; } }
        else if (a == "--region") {
            const char* r = take();
            char tail = 0;
            if (!r || std::sscanf(r, "%lld,%lld,%lld,%lld%c", &region[0], &region[1], &region[2], &region[3], &tail) != 4) { std::fprintf(stderr, "Error: --region takes X0,Y0,X1,Y1\n"); return 1; }
            have_region = true;
        }
        else if (a == "--adaptive") { float f; if (parse_float(take(), f)) { acfg.rel_error = f; adaptive = true; } }
        else if (a == "--abs-floor") { float f; if (parse_float(take(), f)) acfg.abs_floor = f; }
        else if (a == "--min-spp") { size_t t; if (parse_usize(take(), t)) acfg.min_spp = (uint32_t)t; }
        else if (a == "--max-spp") { size_t t; if (parse_usize(take(), t)) acfg.max_spp = (uint32_t)t; }
        else if (a == "--batch") { size_t t; if (parse_usize(take(), t)) acfg.batch_spp = (uint32_t)t; }
        else if (a == "-h" || a == "--help") {
            std::printf("raytracer-rs (MI355X) 0.1.0\nusage: raytracer [-f COLLADA_FILENAME] [-m MAX_TRIS] [-i FRAME_ITERATIONS] [--width W] [--height H]\n"
                        "                 [--spp N] [--seed S] [--gpus N] [--out image.ppm|image.png] [--fix-row-index] [--device-lbvh]\n"
                        "                 [--adaptive REL [--abs-floor F] [--min-spp N] [--max-spp N] [--batch N]] [--denoise | --denoise-split]\n"
                        "                 [--load-film film.bin]... [--save-film film.bin]\n"
                        "                 [--exposure F | --auto-exposure [--key F]] [--curve reinhard|reinhard-white|aces|clamp] [--white F] [--srgb]\n"
                        "                 [--ortho-width W]   (with --spp: an orthographic view W world units wide, through mi355rt_render_rays)\n"
                        "                 [--lens thin --lens-radius R --focus F | --lens ortho --lens-width W]   (with --spp: depth of field / an orthographic\n"
                        "                                     view made on the device, mi355rt_set_lens; excludes --adaptive, --gpus and -i; adaptive sampling\n"
                        "                                     under a lens: --refine)\n"
                        "                 [--region X0,Y0,X1,Y1]   (with --spp: only the tiles the pixel rectangle touches, mi355rt_render_tiles; allowed with --lens;\n"
                        "                                     excludes --gpus, -i and --adaptive)\n"
                        "                 [--refine REL [--abs-floor F] [--min-spp N] [--max-spp N] [--batch N]]   (the adaptive loop from mi355rt_adaptive_tile_mask and\n"
                        "                                     mi355rt_render_tiles: the way to sample adaptively under --lens; excludes --spp, --gpus, -i and --adaptive)\n"
                        "                 [--features N]   (after the render: N samples per pixel into the feature film, mi355rt_features_render: the primary hits' depth,\n"
                        "                                     normal, albedo and coverage under the lens in force; under --ortho-width along the rays of an N-sample\n"
                        "                                     orthographic render; excludes --gpus)\n"
                        "                 [--denoise-guides centre|features]   (where --denoise, --denoise-split and the display options take their guides from; features\n"
                        "                                     needs --features and allows --denoise with --ortho-width)\n"
                        "                 [--alpha]   (needs --features and --out image.png: an RGBA PNG, A = coverage (hits / samples) * 255 rounded; the RGB bytes are\n"
                        "                                     unchanged and PREMULTIPLIED by construction, because a sample that misses the scene is black)\n"
                        "                 [--light-films]   (the handle keeps a film per light, MI355RT_FLAG_LIGHT_FILMS: needs --spp, --adaptive or --refine; excludes --gpus)\n"
                        "                 [--relight W0,W1,...]   (needs --light-films: --out receives the frame with light i's colour scaled by Wi, mixed from the light films\n"
                        "                                     without tracing, mi355rt_get_relit_pixels; the display options apply; excludes --denoise, --denoise-split)\n"
                        "                 [--out-lights PREFIX]   (needs --light-films: PREFIX<i>.png, light i alone at weight 1, under the same display options)\n"
                        "                 [--bake W,H [--bake-dilate K] [--bake-uv-out FILE]]   (with --spp N and --out: a lightmap of W x H texels instead of a frame: the auto\n"
                        "                                     atlas, N gather samples per covered texel, radiance = albedo * direct + indirect, K dilation steps (default 2),\n"
                        "                                     packed under the display options; FILE receives the UVs as raw little-endian f32; excludes --auto-exposure\n"
                        "                                     and every option that renders or reads a frame)\n");
            return 0;
        }
    }
    if (ortho && (!spp || adaptive || ((denoise || denoise_split) && !guides_features) || gpus > 1)) { std::fprintf(stderr, "Error: --ortho-width needs --spp and excludes --adaptive, --denoise, --denoise-split and --gpus\n"); return 1; }
    if (features && gpus > 1) { std::fprintf(stderr, "Error: --features excludes --gpus\n"); return 1; }
    if (guides_features && !features) { std::fprintf(stderr, "Error: --denoise-guides features needs --features\n"); return 1; }
    if (alpha && (!features || !(out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0))) { std::fprintf(stderr, "Error: --alpha needs --features and --out image.png\n"); return 1; }
    if ((have_relight || !out_lights.empty()) && !light_films) { std::fprintf(stderr, "Error: --relight and --out-lights need --light-films\n"); return 1; }
    if (light_films && (gpus > 1 || !(spp || adaptive || refine))) { std::fprintf(stderr, "Error: --light-films needs --spp, --adaptive or --refine and excludes --gpus\n"); return 1; }
    if (have_relight && (denoise || denoise_split)) { std::fprintf(stderr, "Error: --relight excludes --denoise and --denoise-split\n"); return 1; }
    // the option given together with --region / --refine that it excludes (null: none)
    auto excluded_by_tiles = [&](bool with_spp) -> const char* {
        if (with_spp && spp) return "--spp";
        if (gpus > 1) return "--gpus";
        if (have_iterations) return "-i";
        if (adaptive) return "--adaptive";
        if (ortho) return "--ortho-width";
        return nullptr;
    };
    if (have_region) {
        const char* x = refine ? "--refine" : excluded_by_tiles(false);
        if (x) { std::fprintf(stderr, "Error: --region excludes %s\n", x); return 1; }
        if (!spp) { std::fprintf(stderr, "Error: --region needs --spp\n"); return 1; }
    }
    if (refine) {
        if (const char* x = excluded_by_tiles(true)) { std::fprintf(stderr, "Error: --refine excludes %s\n", x); return 1; }
    }
    if (have_lens && ((!spp && !refine) || adaptive || gpus > 1 || have_iterations || ortho)) { std::fprintf(stderr, "Error: --lens thin / ortho needs --spp or --refine and excludes --adaptive, --gpus, -i and --ortho-width\n"); return 1; }
    if (have_bake) {
        if (dcfg_display.auto_exposure) { std::fprintf(stderr, "Error: --bake excludes --auto-exposure (an atlas has no film histogram; give --exposure)\n"); return 1; }
        if (!spp || out.empty()) { std::fprintf(stderr, "Error: --bake needs --spp and --out\n"); return 1; }
        if (adaptive || refine || have_region || have_lens || ortho || have_iterations || gpus > 1 || denoise || denoise_split || features || alpha || light_films || have_relight
            || !out_lights.empty() || !load_films.empty() || !save_film.empty()) {
            std::fprintf(stderr, "Error: --bake writes a lightmap, not a frame: it excludes --adaptive, --refine, --region, --lens, --ortho-width, -i, --gpus, --denoise, --denoise-split, "
                                 "--features, --alpha, --light-films, --relight, --out-lights, --load-film and --save-film\n");
            return 1;
        }
        if (bake_w < 1 || bake_h < 1 || bake_w > 16384 || bake_h > 16384 || bake_dilate > 0xFFFFFFFFull) { std::fprintf(stderr, "Error: --bake W,H: 1 .. 16384 each\n"); return 1; }
    } else if (!bake_uv_out.empty()) { std::fprintf(stderr, "Error: --bake-uv-out needs --bake\n"); return 1; }
    if (have_exposure && dcfg_display.auto_exposure) { std::fprintf(stderr, "Error: --exposure and --auto-exposure exclude each other\n"); return 1; }
    std::printf("max triangles per leaf: %zu\n", max_triangles);      // main.rs:66
    if (have_iterations) std::printf("will quit after %zu frame iterations\n", frame_iterations);   // main.rs:73
    if (!have_iterations) { frame_iterations = (spp || adaptive || refine) ? 1 : (height + 49) / 50; }   // headless: one sweep of the frame

    try {
        mi355rt_config cfg = raytracer_lib::make_config(max_triangles, width, height);
        cfg.seed = seed;
        if (fix_row) cfg.flags |= MI355RT_FLAG_FIX_ROW_INDEX;
        if (device_lbvh) cfg.flags |= MI355RT_FLAG_DEVICE_LBVH;             // BVH built on the GPU (Morton order) instead of the host's SAH build
        if (denoise_split) cfg.flags |= MI355RT_FLAG_DIRECT_FILM;
        if (light_films) cfg.flags |= MI355RT_FLAG_LIGHT_FILMS;
        cfg.device_count = (uint32_t)gpus;
        if (share_device) cfg.flags |= MI355RT_FLAG_GROUP_SHARES_DEVICE;      // testing: the whole group on one GPU
        if (gpus > 1) std::printf("rendering on %zu GPUs (rows dealt in stripes of %u)\n", gpus, cfg.stripe_rows);
        raytracer_lib::RayTracer rt = raytracer_lib::create_raytracer_from_file(file, max_triangles, width, height, &cfg);
        std::printf("number of triangles: %u\n", mi355rt_triangle_count(rt.handle()));   // colladaloader.rs:265
        if (have_bake) {
            mi355rt_handle* h = rt.handle();
            auto check = [&](int rc, bool with_handle = true) { if (rc != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(with_handle ? h : nullptr)); };
            const uint32_t ntri = mi355rt_triangle_count(h), bw = (uint32_t)bake_w, bh = (uint32_t)bake_h;
            const size_t nt = (size_t)bw * bh;
            std::vector<float> uv((size_t)ntri * 6);
            uint32_t cell = 0;
            check(mi355rt_bake_auto_atlas(ntri, bw, bh, 1u, uv.data(), &cell), false);
            if (!bake_uv_out.empty()) {
                FILE* f = std::fopen(bake_uv_out.c_str(), "wb");
                if (!f || std::fwrite(uv.data(), sizeof(float), uv.size(), f) != uv.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", bake_uv_out.c_str()); return 1; }
            }
            std::vector<uint32_t> ids(nt), cnt(nt);
            std::vector<float> points(nt * 3), normals(nt * 3), albedo(nt * 3), sum(nt * 3), direct(nt * 3), rad(nt * 3), atlas(nt * 3);
            mi355rt_bake_texel_outputs to{};
            to.ids = ids.data(); to.points = points.data(); to.normals = normals.data(); to.albedo = albedo.data();
            uint32_t n = 0;
            check(mi355rt_bake_texels(h, uv.data(), bw, bh, 0u, MI355RT_RAYS_HOST, &to, &n));
            mi355rt_gather_config gc;
            mi355rt_gather_default_config(&gc);
            gc.spp = (uint32_t)spp;
            mi355rt_gather_outputs go{};
            go.n = cnt.data(); go.sum = sum.data(); go.direct = direct.data();
            check(mi355rt_gather(h, points.data(), normals.data(), ids.data(), n, &gc, MI355RT_RAYS_HOST, &go));
            const mi355rt_ray_counts c = rt.last_counts();
            for (size_t k = 0; k < (size_t)n; ++k)
                for (int a = 0; a < 3; ++a) rad[3 * k + a] = albedo[3 * k + a] * direct[3 * k + a] + sum[3 * k + a] / (float)cnt[k];      // bake.radiance: f32, unfused
            check(mi355rt_bake_atlas(h, ids.data(), rad.data(), n, bw, bh, (uint32_t)bake_dilate, MI355RT_RAYS_HOST, atlas.data(), nullptr));
            std::vector<uint32_t> packed(nt);
            check(mi355rt_display_image(h, atlas.data(), nt, display ? &dcfg_display : nullptr, packed.data()));
            std::printf("bake: %u x %u texels in cells of %u, %u covered, %zu samples each, %u dilation steps  %.3f ms\n", bw, bh, cell, n, spp, (uint32_t)bake_dilate, c.total_ms);
            if (display) std::printf("display: exposure %.9g\n", (double)dcfg_display.exposure);
            const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0;
            if (png) {
                if (!write_png(out, packed, bw, bh, nullptr)) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
            } else {
                FILE* f = std::fopen(out.c_str(), "wb");
                if (!f) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
                std::fprintf(f, "P6\n%u %u\n255\n", bw, bh);
                for (uint32_t p : packed) { unsigned char rgb[3] = { (unsigned char)(p >> 16), (unsigned char)(p >> 8), (unsigned char)p }; std::fwrite(rgb, 1, 3, f); }
                std::fclose(f);
            }
            return 0;
        }
        if (have_lens) rt.set_lens(lens);
        for (const std::string& f : load_films) rt.film.load(f, true);     // the fresh film is zero: the first file is added to it like the others
        raytracer_lib::stats::Stats stats;
        std::vector<uint32_t> ldr;
        for (size_t it = 0; it < frame_iterations; ++it) {
            uint32_t num_primary_rays;
            if (adaptive) {
                const mi355rt_adaptive_stats st = rt.render_adaptive(acfg);
                const mi355rt_ray_counts c = rt.last_counts();
                num_primary_rays = (uint32_t)c.primary;
                std::printf("adaptive: %u rounds, %u of %u tiles active at the first verdict, %u at the last, %llu samples added (%.2f per owned pixel)  %.3f ms\n",
                            st.rounds, st.tiles_active_first, st.tiles, st.tiles_active_last, (unsigned long long)st.samples_added,
                            (double)st.samples_added / ((double)mi355rt_owned_rows(rt.handle()) * (double)width), c.total_ms);
            } else if (refine) {
                mi355rt_ray_counts c{};
                const mi355rt_adaptive_stats st = rt.refine(acfg, &c);
                num_primary_rays = (uint32_t)c.primary;
                std::printf("adaptive: %u rounds, %u of %u tiles active at the first verdict, %u at the last, %llu samples added (%.2f per owned pixel)  %.3f ms\n",
                            st.rounds, st.tiles_active_first, st.tiles, st.tiles_active_last, (unsigned long long)st.samples_added,
                            (double)st.samples_added / ((double)mi355rt_owned_rows(rt.handle()) * (double)width), c.total_ms);
            } else if (spp) {
                mi355rt_ray_counts c;
                if (have_region) c = rt.render_tiles(rt.region_mask(region[0], region[1], region[2], region[3]), (uint32_t)spp);
                else if (ortho) {
                    float rot[16], orient[16], max_xy[2];
                    mi355rt_camera_get(rt.handle(), rot, orient, max_xy);
                    std::vector<uint32_t> film_n(width * height);
                    if (mi355rt_film_get(rt.handle(), nullptr, nullptr, film_n.data()) != MI355RT_OK) throw std::runtime_error(mi355rt_last_error(rt.handle()));
                    c = rt.render_rays(ortho_rays(rot, orient, width, height, spp, (uint32_t)seed, ortho_width, film_n), (uint32_t)spp);
                } else c = rt.render((uint32_t)spp);
                num_primary_rays = (uint32_t)c.primary;
                std::printf("frame: %.3f ms  rays: %llu primary %llu bounce %llu shadow -> %.1f Mrays/s\n", c.total_ms,
                            (unsigned long long)c.primary, (unsigned long long)c.bounce, (unsigned long long)c.shadow,
                            (double)(c.primary + c.bounce + c.shadow) / c.total_ms / 1e3);
            } else {
                num_primary_rays = rt.trace_frame_additive();
            }
            ldr = rt.get_tonemapped_pixels();
            std::printf("%s\n", stats.stats(num_primary_rays).c_str());  // main.rs:213
        }
        std::printf("%s\n\n\n", stats.mean_stats().c_str());             // main.rs:216
        if (!save_film.empty()) rt.film.save(save_film);
        std::vector<unsigned char> alpha8;
        if (features) {                                                   // the feature film of the view the loop rendered
            if (ortho) {
                float rot[16], orient[16], max_xy[2];
                mi355rt_camera_get(rt.handle(), rot, orient, max_xy);
                rt.features.render_rays(ortho_rays(rot, orient, width, height, features, (uint32_t)seed, ortho_width, std::vector<uint32_t>(width * height, 0u)), (uint32_t)features);
            } else rt.features.render((uint32_t)features);
            std::printf("features: %zu samples per pixel\n", features);
            if (guides_features) rt.set_guide_source(MI355RT_GUIDES_FEATURES);
            if (alpha) for (float a : rt.features.alpha()) alpha8.push_back((unsigned char)(uint32_t)(a * 255.0f + 0.5f));
        }
        if (frame_iterations == 0 && !load_films.empty()) ldr = rt.get_tonemapped_pixels();       // a merge-only run: the loaded film, read out once
        if (light_films) {
            const size_t nl = rt.light_films.nlights();
            std::printf("light films: %zu lights\n", nl);
            if (have_relight && relight.size() != nl) throw std::runtime_error("--relight: " + std::to_string(relight.size()) + " factors given, the scene has " + std::to_string(nl) + " lights");
            dcfg_display.source = MI355RT_DISPLAY_SOURCE_FILM;
            for (size_t li = 0; !out_lights.empty() && li < nl; ++li) {    // each light alone at weight 1
                std::vector<float> w3(nl * 3, 0.0f);
                w3[li * 3] = w3[li * 3 + 1] = w3[li * 3 + 2] = 1.0f;
                const std::string path = out_lights + std::to_string(li) + ".png";
                if (!write_png(path, rt.get_relit_pixels(w3, display ? &dcfg_display : nullptr), width, height, nullptr)) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
            }
        }
        if (have_relight) {                                               // the relit frame instead of the film's read-out
            std::vector<float> w3;
            for (float f : relight) { w3.push_back(f); w3.push_back(f); w3.push_back(f); }
            float used = 1.0f;
            ldr = rt.get_relit_pixels(w3, display ? &dcfg_display : nullptr, nullptr, &used);
            if (display) std::printf("display: exposure %.9g%s\n", (double)used, dcfg_display.auto_exposure ? " (auto)" : "");
        } else if (display) {                                             // the display read-out of the film the loop left, of the source the denoise options select
            dcfg_display.source = denoise_split ? MI355RT_DISPLAY_SOURCE_DENOISED_SPLIT : denoise ? MI355RT_DISPLAY_SOURCE_DENOISED : MI355RT_DISPLAY_SOURCE_FILM;
            float used = 0.0f;
            ldr = rt.get_display_pixels(dcfg_display, nullptr, &used);
            std::printf("display: exposure %.9g%s\n", (double)used, dcfg_display.auto_exposure ? " (auto)" : "");
        } else if (denoise || denoise_split) {                            // the denoised read-out of the film the loop left (default config)
            mi355rt_denoise_config dcfg;
            mi355rt_denoise_default_config(&dcfg);
            ldr = denoise_split ? rt.get_denoised_pixels_split(dcfg) : rt.get_denoised_pixels(dcfg);
        }
        if (!out.empty()) {
            const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0;
            if (png) {
                if (!write_png(out, ldr, width, height, alpha ? &alpha8 : nullptr)) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
            } else {
                FILE* f = std::fopen(out.c_str(), "wb");
                if (!f) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
                std::fprintf(f, "P6\n%zu %zu\n255\n", width, height);
                for (uint32_t p : ldr) { unsigned char rgb[3] = { (unsigned char)(p >> 16), (unsigned char)(p >> 8), (unsigned char)p }; std::fwrite(rgb, 1, 3, f); }
                std::fclose(f);
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Error: %s\n", e.what());                   // main() -> Result<(), String>
        return 1;
    }
    return 0;
}
