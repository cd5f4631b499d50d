// renderer.cpp — see renderer.hpp.
#include "renderer.hpp"
#include "bake.hpp"
#include "display.hpp"
#include "lightmap.hpp"
#include "reflmask.hpp"
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kernels.hpp"
#include "lens.hpp"
#include "octree.hpp"
#include "probes.hpp"
#include "probes_vis.hpp"
#include "probes_place.hpp"
#include "probe_place.hpp"
#include "probe_lit.hpp"
#include "staging.hpp"

namespace mi355rt {

static_assert(sizeof(ShGrid) == sizeof(mi355rt_probe_grid), "sh9.hpp's grid is the header's");

namespace {
// counter RNG, identical to the device copy in kernels.hip (pcg4d, Jarzynski & Olano 2020)
void pcg4d(uint32_t v[4])
{
    for (int i = 0; i < 4; ++i) v[i] = v[i] * 1664525u + 1013904223u;
    v[0] += v[1] * v[3]; v[1] += v[2] * v[0]; v[2] += v[0] * v[1]; v[3] += v[1] * v[2];
    for (int i = 0; i < 4; ++i) v[i] ^= v[i] >> 16;
    v[0] += v[1] * v[3]; v[1] += v[2] * v[0]; v[2] += v[0] * v[1]; v[3] += v[1] * v[2];
}
float u01(uint32_t bits) { return (float)(bits >> 9) * (1.0f / 8388608.0f); }

// the 256-entry sRGB threshold table the display kernels search; entry 0 is never read: the search starts above it
void display_srgb_table(float t[256]) { t[0] = 0.0f; display_srgb_thresholds(t + 1); }

// DISPLAY MAPPING's arguments; dc null: the reference's tone map (the Reinhard curve, the reference's transfer)
DisplayArgs display_args(const mi355rt_display_config* dc, float exposure)
{
    DisplayArgs a{};
    a.curve = dc ? dc->curve : MI355RT_CURVE_REINHARD; a.transfer = dc ? dc->transfer : MI355RT_TRANSFER_REFERENCE; a.exposure = exposure; a.white2 = dc ? dc->white * dc->white : 16.0f;
    return a;
}
}  // namespace

bool Renderer::fail(hipError_t e, const char* what)
{
    last_error = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}
#define HIP_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return fail(e__, #expr); } while (0)

bool Renderer::bind()
{
    HIP_TRY(hipSetDevice(cfg.device));
    return true;
}

// what most entries start with: the handle's device is current and no speculative frame is out
bool Renderer::quiet() { return bind() && settle_speculation(); }

template <class T> bool Renderer::upload(DeviceBuffer<T>& buf, const void* src, size_t bytes)
{
    HIP_TRY(buf.alloc(bytes ? bytes : 16, &hbm_bytes_));
    if (bytes && src) HIP_TRY(hipMemcpy(buf.get(), src, bytes, hipMemcpyHostToDevice));
    else if (bytes) HIP_TRY(hipMemset(buf.get(), 0, bytes));
    return true;
}

template <class T> bool Renderer::upload(T*& dptr, const void* src, size_t bytes)
{
    scene_bufs_.emplace_back();
    if (!upload(scene_bufs_.back(), src, bytes)) return false;
    dptr = static_cast<T*>(scene_bufs_.back().get());
    return true;
}

std::unique_ptr<Renderer> Renderer::create(const SceneData& scene, const mi355rt_config& cfg, std::string& err, int& code)
{
    std::unique_ptr<Renderer> r(new Renderer());
    r->cfg = cfg;
    if (!r->init(scene, err, code)) return nullptr;
    return r;
}

// SampleGenerator::new, sample_generator.rs:15-24 + 36-52, seeded: 65 536 unit vectors by rejection in the unit ball
void Renderer::build_sample_table(std::vector<float>& table4)
{
    table.resize((size_t)kNumSamples * 3);
    table4.assign((size_t)kNumSamples * 4, 0.0f);
    for (uint32_t i = 0; i < kNumSamples; ++i) {
        for (uint32_t attempt = 0;; ++attempt) {
            uint32_t h[4] = { i, attempt, 0xFFFFFFFFu, (uint32_t)cfg.seed };
            pcg4d(h);
            Vec3 d(u01(h[0]) * 2.0f + -1.0f, u01(h[1]) * 2.0f + -1.0f, u01(h[2]) * 2.0f + -1.0f);   // random_range(-1.0..1.0)
            if (dot(d, d) < 1.0f) {
                Vec3 nrm = d.normalized();
                table[3 * (size_t)i] = nrm.x; table[3 * (size_t)i + 1] = nrm.y; table[3 * (size_t)i + 2] = nrm.z;
                table4[4 * (size_t)i] = nrm.x; table4[4 * (size_t)i + 1] = nrm.y; table4[4 * (size_t)i + 2] = nrm.z;
                break;
            }
        }
    }
}

// mi355rt_set_seed: the handle afterwards equals one created with this seed (per-sample hash key AND direction table)
bool Renderer::set_seed(uint64_t seed)
{
    if (!quiet()) return false;
    cfg.seed = seed;
    std::vector<float> table4;
    build_sample_table(table4);
    for (Slice& o : slices_) if (o.stream) HIP_TRY(hipStreamSynchronize(o.stream));
    HIP_TRY(hipMemcpy(const_cast<void*>(dscene_.table), table4.data(), table4.size() * sizeof(float), hipMemcpyHostToDevice));
    return true;
}

// mi355rt_set_flags: run-time flags only; a create-time flag (the intersector) cannot be changed on a live handle
bool Renderer::set_flags(uint32_t flags)
{
    constexpr uint32_t kCreateMask = MI355RT_FLAG_OCTREE_SEMANTICS | MI355RT_FLAG_TRUE_CLOSEST_HIT | MI355RT_FLAG_GROUP_SHARES_DEVICE | MI355RT_FLAG_DEVICE_LBVH | MI355RT_FLAG_DIRECT_FILM | MI355RT_FLAG_LIGHT_FILMS;
    if ((flags ^ cfg.flags) & kCreateMask) { last_error = "the intersector flags (OCTREE_SEMANTICS, TRUE_CLOSEST_HIT), GROUP_SHARES_DEVICE, DEVICE_LBVH, DIRECT_FILM and LIGHT_FILMS are create-time flags: they cannot be changed with mi355rt_set_flags"; return false; }
    if (flags != cfg.flags && !settle_speculation()) return false;
    cfg.flags = flags;
    return true;
}

bool Renderer::init(const SceneData& scene, std::string& err, int& code)
{
    code = MI355RT_E_INVALID;
    if (cfg.recursions == 0 && cfg.spread == 0) { cfg.recursions = 2; cfg.spread = 1; }   // RECURSIONS / SUB_SPREAD, mod.rs:81-82
    if (cfg.spread == 0) cfg.spread = 1;
    if (cfg.triangles_per_leaf == 0) cfg.triangles_per_leaf = MI355RT_DEFAULT_TRIANGLES_PER_LEAF;
    if (cfg.width == 0 || cfg.height == 0) { err = "width and height must be non-zero"; return false; }
    if ((uint64_t)cfg.width * cfg.height > 0x7FFFFFFFull / 4) { err = "image too large"; return false; }
    if (cfg.recursions > kMaxRecursions) { err = "recursions > 3 not supported"; return false; }
    if ((cfg.flags & MI355RT_FLAG_LIGHT_FILMS) && scene.lights.size() > MI355RT_LIGHT_FILMS_MAX_LIGHTS) { err = "MI355RT_FLAG_LIGHT_FILMS: the scene has " + std::to_string(scene.lights.size()) + " lights, more than MI355RT_LIGHT_FILMS_MAX_LIGHTS (8)"; return false; }
    if (scene.cameras.empty()) { err = "scene has no camera"; return false; }     // scene.cameras[0] panics in the reference, lib.rs:39
    if (scene.tri_geom.size() * 9 != scene.tri_verts.size()) { err = "tri_verts / tri_geom size mismatch"; return false; }
    for (uint32_t g : scene.tri_geom) if (g >= scene.materials.size()) { err = "tri_geom entry out of range"; return false; }
    for (auto& m : scene.materials) if (m.kind == 1 && m.tex_id >= scene.textures.size()) { err = "material texture id out of range"; return false; }
    if (scene.tri_geom.size() >= (1u << 26)) { err = "too many triangles"; return false; }     // 32-bit byte offsets into the 48-byte triangle array
    {   // radiance tree: level l has prod_{j<l} spread*(recursions-j) nodes
        uint64_t count = 1, first = 0;
        for (uint32_t l = 0; l <= cfg.recursions; ++l) {
            level_first[l] = (uint32_t)first; first += count; count *= (uint64_t)cfg.spread * (cfg.recursions - l);
            if (first > 0xFFFF) { err = "radiance tree too large (spread * recursions)"; return false; }
        }
        for (uint32_t l = cfg.recursions + 1; l <= kMaxLevels; ++l) level_first[l] = (uint32_t)first;
        nodes_per_sample = (uint32_t)first;
    }
    if (cfg.stripe_world <= 1) { cfg.stripe_world = 1; cfg.stripe_rank = 0; }
    if (cfg.stripe_rows == 0) cfg.stripe_rows = MI355RT_DEFAULT_STRIPE_ROWS;
    if (cfg.stripe_rank >= cfg.stripe_world) { err = "stripe_rank >= stripe_world"; return false; }

    code = MI355RT_E_NO_DEVICE;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { err = std::string("no HIP device available (") + hipGetErrorString(e) + "); this library has no CPU fallback"; return false; }
    if (cfg.device < 0 || cfg.device >= ndev) { err = "HIP device ordinal out of range"; return false; }
    auto bail = [&]() { err = last_error; return false; };
    if (!bind()) return bail();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg.device) != hipSuccess) { err = "hipGetDeviceProperties failed"; return false; }
    num_cus_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) { err = "hipStreamCreate failed"; return false; }
    if (hipEventCreate(&ev_begin_) != hipSuccess || hipEventCreate(&ev_end_) != hipSuccess) { err = "hipEventCreate failed"; return false; }

    ntri = scene.ntri();
    nlights_ = (uint32_t)scene.lights.size();
    camera = Camera::from_orientation_matrix(cfg.width, cfg.height, Matrix::from_array(scene.cameras[0].orientation), scene.cameras[0].fov_deg);

    // --- acceleration structure (host build, once) + per-triangle normals (calc_normal, mod.rs:198-205)
    const auto t_bvh = std::chrono::steady_clock::now();
    bool on_device = false;
    if (cfg.flags & MI355RT_FLAG_DEVICE_LBVH) {
        std::string why; double ms[2];
        on_device = build_bvh_device(scene.tri_verts.data(), scene.tri_geom.data(), ntri, bvh, why, ms);
        if (on_device) { lbvh_device_ms_ = ms[0]; }
        else last_error = "device LBVH not used (" + why + "): host SAH build instead";      // not an error: create goes on
    }
    if (!on_device) build_bvh(scene.tri_verts.data(), scene.tri_geom.data(), ntri, bvh);
    bvh_on_device_ = on_device;
    wide_ = false;
    if (kernels_walk_wide_nodes()) {
        build_wide(bvh);
        if (!bvh.nodes4.empty()) wide_ = true;
        else if (bvh.root >= 0) { err = "this build's kernels walk the 4-wide tree, which does not serve this scene"; code = MI355RT_E_INVALID; return false; }
    }
    build_ms_[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_bvh).count();
    collect_cull_boxes();
    if (bvh.max_depth > kBvhMaxDepth) { err = "internal: BVH deeper than the traversal stack"; code = MI355RT_E_INVALID; return false; }
    std::vector<float> normals((size_t)std::max(ntri, 1u) * 4, 0.0f);
    for (uint32_t t = 0; t < ntri; ++t) {
        const float* v = &scene.tri_verts[9 * (size_t)t];
        Vec3 v0(v[0], v[1], v[2]), v1(v[3], v[4], v[5]), v2(v[6], v[7], v[8]);
        Vec3 n = cross(v1 - v0, v2 - v0).normalized();
        normals[4 * (size_t)t] = n.x; normals[4 * (size_t)t + 1] = n.y; normals[4 * (size_t)t + 2] = n.z;
        uint32_t g = scene.tri_geom[t];
        std::memcpy(&normals[4 * (size_t)t + 3], &g, 4);
    }
    std::vector<float> table4;
    build_sample_table(table4);
    // --- uploads
    void* d_nodes = nullptr; void* d_tris = nullptr; void* d_normals = nullptr; void* d_table = nullptr;
    DMaterial* d_mats = nullptr; DLight* d_lights = nullptr; DTexture* d_tex = nullptr; float* d_texels = nullptr;
    if (wide_ ? !upload(d_nodes, bvh.nodes4.data(), bvh.nodes4.size() * sizeof(BvhNode4)) : !upload(d_nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(BvhNode))) return bail();
    if (!upload(d_tris, bvh.tris.data(), bvh.tris.size() * sizeof(BvhTri))) return bail();
    if (!upload(d_normals, normals.data(), normals.size() * sizeof(float))) return bail();
    if (!upload(d_table, table4.data(), table4.size() * sizeof(float))) return bail();
    std::vector<DMaterial> mats(std::max<size_t>(scene.materials.size(), 1));
    for (size_t i = 0; i < scene.materials.size(); ++i) {
        const MaterialData& m = scene.materials[i];
        mats[i] = DMaterial{ m.rgb[0], m.rgb[1], m.rgb[2], m.kind == 1 ? (0x80000000u | m.tex_id) : 0u };
    }
    if (!upload(d_mats, mats.data(), mats.size() * sizeof(DMaterial))) return bail();
    std::vector<DLight> lights(std::max<size_t>(scene.lights.size(), 1));
    for (size_t i = 0; i < scene.lights.size(); ++i) {
        const LightData& l = scene.lights[i];
        lights[i] = DLight{ l.pos[0], l.pos[1], l.pos[2], l.color[0], l.color[1], l.color[2], 0.0f, 0.0f };
    }
    // Depth cube maps around the lights (lightmap.hpp): shadow rays they prove free are never made.  Resolution: 512 texels per face edge, halved
    // until the build stays under ~4 M texel updates (a scene of a few huge triangles) and the maps under 64 MiB; MI355RT_LIGHT_MAP_RES (a power of two,
    // 16 .. 2048) forces it.  1024 and 2048 prove a quarter and a third of the remaining shadow rays free and were measured: they do not pay on the
    // frame (profiles/proofs_bench_ab.txt).  Padded by ten times the BVH's own padding (bvh.cpp: 2e-5 of the scene diagonal), the margin
    // the culling mask uses.
    float* d_light_maps = nullptr; uint32_t light_map_res = 0;
    if (!scene.lights.empty() && scene.lights.size() <= 8 && ntri > 0 && !getenv("MI355RT_NO_LIGHT_MAP")) {
        const auto t_lm = std::chrono::steady_clock::now();
        double diag2 = 0.0;
        { float mn[3] = { 3e38f, 3e38f, 3e38f }, mx[3] = { -3e38f, -3e38f, -3e38f };
          for (size_t i = 0; i < scene.tri_verts.size(); ++i) { const int a = (int)(i % 3); mn[a] = std::min(mn[a], scene.tri_verts[i]); mx[a] = std::max(mx[a], scene.tri_verts[i]); }
          for (int a = 0; a < 3; ++a) diag2 += ((double)mx[a] - mn[a]) * ((double)mx[a] - mn[a]); }
        const double pad = 2e-4 * std::sqrt(diag2) + 1e-7;
        uint32_t res = 512, forced = 0;
        if (const char* e = getenv("MI355RT_LIGHT_MAP_RES")) { const long v = atol(e); if (v >= 16 && v <= 2048 && (v & (v - 1)) == 0) forced = (uint32_t)v; }
        while (res > 16 && (size_t)6 * res * res * 4 * scene.lights.size() > ((size_t)64 << 20)) res /= 2;
        const uint64_t work_cap = 4ull << 20;
        for (const LightData& l : scene.lights) while (!forced && res > 16 && light_map_work(scene.tri_verts.data(), ntri, l.pos, res) > work_cap) res /= 2;
        if (forced) res = forced;
        std::vector<float> all; all.reserve((size_t)6 * res * res * scene.lights.size());
        bool finite = true;
        for (size_t i = 0; i < scene.lights.size() && finite; ++i) {
            const LightData& l = scene.lights[i];
            if (!std::isfinite(l.pos[0]) || !std::isfinite(l.pos[1]) || !std::isfinite(l.pos[2])) { finite = false; break; }
            LightMap lm; build_light_map(scene.tri_verts.data(), ntri, l.pos, pad, res, lm);
            all.insert(all.end(), lm.dist2.begin(), lm.dist2.end());
            const double tail = std::max(lm.nearest - pad, 0.0);
            lights[i].tail2 = std::isfinite(tail) ? (float)std::min(tail * tail * (1.0 - 1e-6), 3.0e38) : 3.0e38f;
            if ((double)lights[i].tail2 > tail * tail) lights[i].tail2 = std::nextafterf(lights[i].tail2, 0.0f);
        }
        if (finite) {
            if (!upload(d_light_maps, all.data(), all.size() * sizeof(float))) return bail();
            light_map_res = res;
        }
        light_map_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_lm).count();
        if (getenv("MI355RT_DEBUG_CULL")) fprintf(stderr, "[mi355rt] light maps: %zu lights, %u texels per face edge, %.1f ms\n", scene.lights.size(), light_map_res, light_map_ms_);
    }
    if (!upload(d_lights, lights.data(), lights.size() * sizeof(DLight))) return bail();
    // Direction masks of the triangles (reflmask.hpp): reflection rays they prove free are never made.  Far occluders are padded like the lights' maps are; a
    // build that would take more than MI355RT_REFLECT_MASK_WORK work units (tree nodes visited + cone tests; thai2 takes under 1 % of the default) is abandoned.
    uint32_t* d_refl_mask = nullptr; uint32_t refl_bins = 0, refl_stride = 0;
    if (ntri > 0 && cfg.recursions > 0 && !getenv("MI355RT_NO_REFLECT_MASK")) {
        double diag2 = 0.0;
        { float mn[3] = { 3e38f, 3e38f, 3e38f }, mx[3] = { -3e38f, -3e38f, -3e38f };
          for (size_t i = 0; i < scene.tri_verts.size(); ++i) { const int a = (int)(i % 3); mn[a] = std::min(mn[a], scene.tri_verts[i]); mx[a] = std::max(mx[a], scene.tri_verts[i]); }
          for (int a = 0; a < 3; ++a) diag2 += ((double)mx[a] - mn[a]) * ((double)mx[a] - mn[a]); }
        uint64_t budget = 4000000000ull;
        if (const char* e = getenv("MI355RT_REFLECT_MASK_WORK")) budget = std::strtoull(e, nullptr, 10);
        ReflMask rm;
        uint32_t bins = kReflBins;
        if (const char* e = getenv("MI355RT_REFLECT_MASK_BINS")) { const int v = atoi(e); if (v == 8 || v == 16) bins = (uint32_t)v; }     // 8: the 64-byte records of the first masks
        if (std::isfinite(diag2) && build_reflect_mask(scene.tri_verts.data(), ntri, 2e-4 * std::sqrt(diag2) + 1e-7, bins, budget, rm)) {
            if (!upload(d_refl_mask, rm.words.data(), rm.words.size() * sizeof(uint32_t))) return bail();
            refl_bins = rm.bins; refl_stride = rm.stride;
            reflect_mask_info_[2] = (double)rm.clear_bits / ((double)ntri * 6.0 * rm.bins * rm.bins);
            reflect_mask_info_[3] = (double)(rm.words.size() * sizeof(uint32_t));
        }
        reflect_mask_info_[0] = (double)refl_bins; reflect_mask_info_[1] = rm.build_ms;
        if (getenv("MI355RT_DEBUG_CULL")) fprintf(stderr, "[mi355rt] reflection masks: %u bins per face edge, %.1f ms, %llu work units, %.3f of the bits clear\n", refl_bins, rm.build_ms, (unsigned long long)rm.work, reflect_mask_info_[2]);
    }
    std::vector<DTexture> tex(std::max<size_t>(scene.textures.size(), 1));
    std::vector<float> texels;
    for (size_t i = 0; i < scene.textures.size(); ++i) {
        const TextureData& t = scene.textures[i];
        if (t.rgb.size() != (size_t)t.width * t.height * 3 || t.rgb.empty()) { err = "texture size mismatch"; code = MI355RT_E_INVALID; return false; }
        tex[i] = DTexture{ t.width, t.height, texels.size() / 3 };
        texels.insert(texels.end(), t.rgb.begin(), t.rgb.end());
    }
    if (!upload(d_tex, tex.data(), tex.size() * sizeof(DTexture))) return bail();
    if (!upload(d_texels, texels.data(), texels.size() * sizeof(float))) return bail();
    dscene_.nodes = d_nodes; dscene_.tris = d_tris; dscene_.normals = d_normals; dscene_.materials = d_mats;
    dscene_.lights = d_lights; dscene_.textures = d_tex; dscene_.texels = d_texels; dscene_.table = d_table;
    dscene_.root = bvh.root; dscene_.nlights = nlights_; dscene_.ntri = ntri;
    dscene_.light_maps = d_light_maps; dscene_.light_map_res = light_map_res;
    dscene_.refl_mask = d_refl_mask; dscene_.refl_bins = refl_bins; dscene_.refl_stride = refl_stride;
    dscene_.oct_nodes = nullptr; dscene_.oct_leaf_tris = nullptr; dscene_.prim_tris = nullptr; dscene_.oct_info = nullptr; dscene_.tri_home = nullptr; dscene_.oct_single_leaf = 0u;
    std::memset(dscene_.oct_root, 0, sizeof dscene_.oct_root);
    // Intersector semantics.  Default: the reference's default intersector (OctTreeIntersector), served by
    // the BVH + the octree confirm step.  MI355RT_FLAG_OCTREE_SEMANTICS: the octree walked directly (slow cross-check).
    // MI355RT_FLAG_TRUE_CLOSEST_HIT: BVH only (NoAccelerationIntersector semantics), no octree is built.
    mode_ = (cfg.flags & MI355RT_FLAG_OCTREE_SEMANTICS) ? kModeOctreeWalk : (cfg.flags & MI355RT_FLAG_TRUE_CLOSEST_HIT) ? kModeTrueClosest : kModeConfirm;
    if (mode_ != kModeTrueClosest) {
        // the reference's own structure (OctTreeIntersector::with_triangles_per_leaf, OCT:66-81)
        Octree oct;
        const auto t_oct = std::chrono::steady_clock::now();
        build_octree(scene.tri_verts.data(), ntri, cfg.triangles_per_leaf, oct);
        build_ms_[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_oct).count();
        octree_counts(oct, oct_stats_);
        std::vector<BvhTri> prim_tris(std::max(ntri, 1u));
        std::memset(prim_tris.data(), 0, prim_tris.size() * sizeof(BvhTri));
        for (uint32_t t = 0; t < ntri; ++t) {
            const float* v = &scene.tri_verts[9 * (size_t)t];
            for (int a = 0; a < 3; ++a) { prim_tris[t].v0[a] = v[a]; prim_tris[t].e1[a] = v[3 + a] - v[a]; prim_tris[t].e2[a] = v[6 + a] - v[a]; }
            prim_tris[t].prim = t; prim_tris[t].geom = scene.tri_geom[t];
        }
        void* d_oct = nullptr; uint32_t* d_leaf = nullptr; void* d_ptris = nullptr;
        if (!upload(d_oct, oct.nodes.data(), oct.nodes.size() * sizeof(OctNodeFlat))) return bail();
        if (!upload(d_leaf, oct.leaf_tris.data(), oct.leaf_tris.size() * 4)) return bail();
        if (!upload(d_ptris, prim_tris.data(), prim_tris.size() * sizeof(BvhTri))) return bail();
        dscene_.oct_nodes = d_oct; dscene_.oct_leaf_tris = d_leaf; dscene_.prim_tris = d_ptris;
        // compact views for the confirm walk
        std::vector<int2> info(oct.nodes.size());
        std::vector<uint32_t> home(std::max(ntri, 1u), 0xFFFFFFFEu);               // 0xFFFFFFFE: in no leaf (yet)
        for (size_t i = 0; i < oct.nodes.size(); ++i) {
            const OctNodeFlat& f = oct.nodes[i];
            if (f.first_child >= 0) { info[i].x = f.first_child; info[i].y = 0; continue; }
            info[i].x = ~(int32_t)f.tri_first; info[i].y = (int32_t)f.tri_count;
            for (uint32_t k = 0; k < f.tri_count; ++k) {
                uint32_t& h = home[oct.leaf_tris[f.tri_first + k]];
                h = h == 0xFFFFFFFEu ? (uint32_t)i : 0xFFFFFFFFu;
            }
        }
        int2* d_info = nullptr; uint32_t* d_home = nullptr;
        if (!upload(d_info, info.data(), info.size() * sizeof(int2))) return bail();
        if (!upload(d_home, home.data(), home.size() * 4)) return bail();
        dscene_.oct_info = d_info; dscene_.tri_home = d_home;
        dscene_.oct_single_leaf = (mode_ == kModeConfirm && oct.nodes.size() == 1) ? 1u : 0u;
        for (int a = 0; a < 3; ++a) { dscene_.oct_root[a] = oct.nodes[0].cmin[a]; dscene_.oct_root[3 + a] = oct.nodes[0].cmax[a]; }
    }

    // --- film (film.rs:27-35) and row lists
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!upload(d_film_sum_, nullptr, npix * 12) || !upload(d_film_sumsq_, nullptr, npix * 12) || !upload(d_film_n_, nullptr, npix * 4)) return bail();
    if ((cfg.flags & MI355RT_FLAG_DIRECT_FILM) && !upload(d_film_direct_, nullptr, npix * 12)) return bail();     // the direct film: only with the flag
    if ((cfg.flags & MI355RT_FLAG_LIGHT_FILMS) && nlights_ && !upload(d_film_lights_, nullptr, npix * 12 * nlights_)) return bail();   // the light films: only with the flag
    if (!upload(d_ldr_, nullptr, npix * 4)) return bail();
    ldr_dirty_.assign(cfg.height, (uint8_t)1);
    if (hipEventCreateWithFlags(&ev_tonemap_, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_gather_, hipEventDisableTiming) != hipSuccess) { err = "hipEventCreate failed"; return false; }
    if (hipEventCreateWithFlags(&ev_call_done_, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_spec_done_, hipEventDisableTiming) != hipSuccess
        || hipStreamCreateWithFlags(&read_stream_, hipStreamNonBlocking) != hipSuccess) { err = "hipEventCreate / hipStreamCreate failed"; return false; }
    std::vector<uint32_t> all(cfg.height);
    for (uint32_t r = 0; r < cfg.height; ++r) {
        all[r] = r;
        if ((r / cfg.stripe_rows) % cfg.stripe_world == cfg.stripe_rank) owned_rows.push_back(r);
    }
    if (!upload(d_all_rows_, all.data(), all.size() * 4)) return bail();
    if (!upload(d_owned_rows_, owned_rows.data(), owned_rows.size() * 4)) return bail();
    if (!upload(d_tmp_rows_, nullptr, 64 * 4)) return bail();
    if (!upload(d_counters_, nullptr, sizeof(DCounters) * kShards)) return bail();
    if (h_counters_.alloc(sizeof(DCounters) * kShards) != hipSuccess) { err = "pinned host allocation failed"; return false; }
    std::memset(h_counters_.get(), 0, sizeof(DCounters) * kShards);
    slices_[0].stream = stream_;
    for (uint32_t i = 0; i < kMaxSlices; ++i) {
        if (i && hipStreamCreateWithFlags(&slices_[i].stream, hipStreamNonBlocking) != hipSuccess) { err = "hipStreamCreate failed"; return false; }
        if (hipEventCreateWithFlags(&slices_[i].done, hipEventDisableTiming) != hipSuccess) { err = "hipEventCreate failed"; return false; }
        if (!upload(slices_[i].d_ctrl, nullptr, kMaxRounds * kCtrlWordsPerRound * 4)) return bail();
        if (!upload(slices_[i].d_rows, nullptr, (size_t)cfg.height * 4)) return bail();
    }
    if (const char* e = getenv("MI355RT_SLICES")) { int v = atoi(e); if (v >= 1 && v <= (int)kMaxSlices) slices = (uint32_t)v; }
    if (!upload(d_debug_color_, nullptr, 16)) return bail();

    // queue records one sample can put into one round's output queue (shadow rays of level l + rays of level l+1)
    records_per_sample_ = 1;
    for (uint32_t l = 0; l <= cfg.recursions; ++l) {
        uint32_t nl = level_first[l + 1] - level_first[l];
        uint32_t nn = l < cfg.recursions ? level_first[l + 2] - level_first[l + 1] : 0;
        records_per_sample_ = std::max(records_per_sample_, nl * std::max(nlights_, 1u) + nn);
    }
    max_level_nodes_ = 1;
    for (uint32_t l = 0; l <= cfg.recursions; ++l) max_level_nodes_ = std::max(max_level_nodes_, level_first[l + 1] - level_first[l]);
    code = MI355RT_OK;
    return true;
}

Renderer::~Renderer()
{
    if (hipSetDevice(cfg.device) != hipSuccess) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (read_stream_) (void)hipStreamSynchronize(read_stream_);          // nothing of this handle is in flight when its memory goes
    for (uint32_t i = 0; i < kMaxSlices; ++i) {
        if (i && slices_[i].stream) { (void)hipStreamSynchronize(slices_[i].stream); (void)hipStreamDestroy(slices_[i].stream); }
        if (slices_[i].done) (void)hipEventDestroy(slices_[i].done);
    }
    comm_destroy();
    if (ev_tonemap_) (void)hipEventDestroy(ev_tonemap_);
    if (read_stream_) (void)hipStreamDestroy(read_stream_);
    if (ev_call_done_) (void)hipEventDestroy(ev_call_done_);
    if (ev_spec_done_) (void)hipEventDestroy(ev_spec_done_);
    if (ev_gather_) (void)hipEventDestroy(ev_gather_);
    for (hipEvent_t e : ev_pool_) (void)hipEventDestroy(e);
    if (ev_begin_) (void)hipEventDestroy(ev_begin_);
    if (ev_end_) (void)hipEventDestroy(ev_end_);
    if (stream_) (void)hipStreamDestroy(stream_);
    // the DeviceBuffer / PinnedBuffer members free their memory after this body: behind the synchronisations above
}

// The (padded, half-precision) boxes of the top BVH subtrees, at most kCullRects of them: the boxes the
// primary-chunk frustum culling tests against.  Breadth-first refinement: always split the largest box.
void Renderer::collect_cull_boxes()
{
    cull_boxes_.clear();
    if (ntri == 0) return;
    auto half_to_float = [](uint32_t h) {
        _Float16 v; uint16_t b = (uint16_t)h; std::memcpy(&v, &b, 2); return (float)v;
    };
    struct Item { std::array<float, 6> box; int32_t node; };
    std::vector<Item> items;
    Item root; root.node = bvh.root;
    for (int a = 0; a < 3; ++a) { root.box[a] = bvh.scene_min[a]; root.box[3 + a] = bvh.scene_max[a]; }
    items.push_back(root);
    for (;;) {
        int best = -1; float best_size = -1.0f;
        for (size_t i = 0; i < items.size(); ++i) {
            if (items[i].node < 0) continue;                        // a leaf cannot be refined
            const auto& b = items[i].box;
            const float size = (b[3] - b[0]) * (b[4] - b[1]) + (b[4] - b[1]) * (b[5] - b[2]) + (b[5] - b[2]) * (b[3] - b[0]);
            if (size > best_size) { best_size = size; best = (int)i; }
        }
        if (best < 0 || items.size() + 1 > kCullRects) break;
        const BvhNode& n = bvh.nodes[items[best].node];
        Item c0, c1;
        for (int a = 0; a < 3; ++a) {
            c0.box[a] = half_to_float(n.h0[a] & 0xFFFFu); c0.box[3 + a] = half_to_float(n.h0[a] >> 16);
            c1.box[a] = half_to_float(n.h1[a] & 0xFFFFu); c1.box[3 + a] = half_to_float(n.h1[a] >> 16);
        }
        c0.node = n.child0; c1.node = n.child1;
        items[best] = c0;
        items.push_back(c1);
    }
    for (const Item& it : items) {
        bool finite = true;
        for (float v : it.box) if (!std::isfinite(v)) finite = false;
        if (!finite) { cull_boxes_.clear(); return; }               // coordinates beyond the half range: no culling
        cull_boxes_.push_back(it.box);
    }
}

// Second culling stage: the coverage mask (device_types.hpp).  Every triangle's three vertices, padded like the boxes of the first stage, are
// projected into the camera's (dir_x, dir_y) plane; the cells their bounding rectangle touches are set.  Any primary ray that hits a triangle has
// its (dir_x, dir_y) inside that triangle's rectangle, so a chunk footprint that touches no set cell holds only misses.  Rebuilt (and uploaded,
// with the renderer's streams idle) only when the camera changed; scenes of more than 2 M triangles keep the first stage only.
// The screen rectangle of every triangle (BVH order) in the camera's (dir_x, dir_y) plane, with every vertex padded by `pad` in world space: what the
// coverage mask and the tile bins are made of.  A point p maps to v = (p - origin) * inv, (dir_x, dir_y) = (v.x, -v.y) / v.z; moving p by at most pad
// per axis moves v.x by at most pad * kx (kx = the absolute column sum of inv), so dir_x by at most pad * (kx + |dir_x| kz) / (v.z - pad kz): the
// rectangle of the three projected vertices, widened by that, holds the projection of the whole padded triangle.  false: something is not in front.
// Cached per camera (both consumers are rebuilt when it changes).
bool Renderer::project_triangles(const DCamera& c, const double inv[3][3], double pad, double zmin)
{
    std::vector<float> key(c.rot, c.rot + 16);
    key.insert(key.end(), c.origin, c.origin + 3);
    if (key == rects_key_ && tri_rects_.size() == bvh.tris.size()) return rects_ok_;
    rects_key_ = key; rects_ok_ = false;
    tri_rects_.resize(bvh.tris.size());
    const double kx = std::fabs(inv[0][0]) + std::fabs(inv[1][0]) + std::fabs(inv[2][0]), ky = std::fabs(inv[0][1]) + std::fabs(inv[1][1]) + std::fabs(inv[2][1]);
    const double kz = std::fabs(inv[0][2]) + std::fabs(inv[1][2]) + std::fabs(inv[2][2]);
    for (size_t i = 0; i < bvh.tris.size(); ++i) {
        const BvhTri& t = bvh.tris[i];
        double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
        for (int v = 0; v < 3; ++v) {
            double w[3];
            for (int a = 0; a < 3; ++a) w[a] = (double)t.v0[a] + (v == 1 ? (double)t.e1[a] : v == 2 ? (double)t.e2[a] : 0.0) - c.origin[a];
            const double vx = w[0] * inv[0][0] + w[1] * inv[1][0] + w[2] * inv[2][0];
            const double vy = w[0] * inv[0][1] + w[1] * inv[1][1] + w[2] * inv[2][1];
            const double vz = w[0] * inv[0][2] + w[1] * inv[1][2] + w[2] * inv[2][2] - pad * kz;       // the nearest the padded vertex can be
            if (!(vz > zmin)) return false;
            const double dx = vx / (vz + pad * kz), dy = -vy / (vz + pad * kz);
            const double mx = pad * (kx + std::fabs(dx) * kz) / vz * 1.0001 + 4e-16 * (1.0 + std::fabs(dx)), my = pad * (ky + std::fabs(dy) * kz) / vz * 1.0001 + 4e-16 * (1.0 + std::fabs(dy));
            x0 = std::min(x0, dx - mx); x1 = std::max(x1, dx + mx); y0 = std::min(y0, dy - my); y1 = std::max(y1, dy + my);
        }
        tri_rects_[i] = TriRect{ x0, x1, y0, y1 };
    }
    rects_ok_ = true;
    return true;
}

bool Renderer::refresh_cull_mask(DCamera& c, const double inv[3][3], double pad, double zmin, bool build)
{
    c.cull_mask = nullptr; c.mask_x0 = c.mask_y0 = 0.0f; c.mask_inv_cx = c.mask_inv_cy = 0.0f;
    if (c.cull_valid == 0 || bvh.tris.empty() || bvh.tris.size() > (2u << 20) || getenv("MI355RT_NO_CULL_MASK")) return true;
    std::vector<float> key(c.rot, c.rot + 16);
    key.insert(key.end(), c.origin, c.origin + 3); key.push_back(c.max_x); key.push_back(c.max_y);
    if (key == mask_key_) {
        if (mask_valid_) { c.cull_mask = d_cull_mask_.get(); c.mask_x0 = mask_dom_[0]; c.mask_y0 = mask_dom_[1]; c.mask_inv_cx = mask_dom_[2]; c.mask_inv_cy = mask_dom_[3]; }
        return true;
    }
    // A 50-row frame of the drop-in loop (0.3 ms) is not worth a rebuild (1.5 ms) when the camera has just moved — the reference's loop moves it between
    // any two calls while a key is held, main.rs:116-169: such calls cull with the first stage alone until a whole-frame pass builds the mask
    if (!build) return true;
    mask_key_ = key; mask_valid_ = false;
    // domain: the bounding rectangle of the first stage's rectangles (everything outside is empty by the first stage)
    double X0 = 1e300, X1 = -1e300, Y0 = 1e300, Y1 = -1e300;
    for (uint32_t k = 0; k < c.cull_valid; ++k) { X0 = std::min(X0, (double)c.cull_rect[k][0]); X1 = std::max(X1, (double)c.cull_rect[k][1]); Y0 = std::min(Y0, (double)c.cull_rect[k][2]); Y1 = std::max(Y1, (double)c.cull_rect[k][3]); }
    if (!(X1 > X0) || !(Y1 > Y0)) return true;
    const double icx = kCullGrid / (X1 - X0), icy = kCullGrid / (Y1 - Y0);
    constexpr uint32_t wpr = kCullGrid / 32u;
    std::vector<uint32_t> bits((size_t)kCullGrid * wpr, 0u);
    if (!project_triangles(c, inv, pad, zmin)) return true;            // cannot happen behind a valid first stage; no mask then
    for (const TriRect& tr : tri_rects_) {
        const double x0 = tr.x0, x1 = tr.x1, y0 = tr.y0, y1 = tr.y1;
        const double mx = 1e-4 * (x1 - x0) + 1e-6, my = 1e-4 * (y1 - y0) + 1e-6;
        // 1/100 of a cell of slack: the kernel computes its cell indices in f32 (error < 1e-4 cells for |dir| of a few units)
        const long i0 = std::max(0L, (long)std::floor((x0 - mx - X0) * icx - 0.01)), i1 = std::min((long)kCullGrid - 1, (long)std::floor((x1 + mx - X0) * icx + 0.01));
        const long j0 = std::max(0L, (long)std::floor((y0 - my - Y0) * icy - 0.01)), j1 = std::min((long)kCullGrid - 1, (long)std::floor((y1 + my - Y0) * icy + 0.01));
        for (long j = j0; j <= j1; ++j) for (long i = i0; i <= i1; ++i) bits[(size_t)j * wpr + (size_t)(i >> 5)] |= 1u << (i & 31);
    }
    if (!bind()) return false;
    if (!d_cull_mask_ && d_cull_mask_.alloc(bits.size() * 4, &hbm_bytes_) != hipSuccess) return true;
    // kernels of earlier calls may still read the old mask: wait for them, then replace it (camera changes are rare and clear the film anyway, main.rs:116-169)
    (void)hipStreamSynchronize(stream_);
    for (Slice& sl : slices_) if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    if (hipMemcpy(d_cull_mask_.get(), bits.data(), bits.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return true;
    mask_dom_[0] = (float)X0; mask_dom_[1] = (float)Y0; mask_dom_[2] = (float)icx; mask_dom_[3] = (float)icy;
    mask_valid_ = true;
    c.cull_mask = d_cull_mask_.get(); c.mask_x0 = mask_dom_[0]; c.mask_y0 = mask_dom_[1]; c.mask_inv_cx = mask_dom_[2]; c.mask_inv_cy = mask_dom_[3];
    if (getenv("MI355RT_DEBUG_CULL")) { size_t n = 0; for (uint32_t w : bits) n += (size_t)__builtin_popcount(w); fprintf(stderr, "[mi355rt] cull mask: %zu of %u cells set, domain x [%g, %g] y [%g, %g]\n", n, kCullGrid * kCullGrid, X0, X1, Y0, Y1); }
    return true;
}

// Screen-space triangle bins for the primary rays (device_types.hpp, kernels.hip raster_tile).  The 64 consecutive samples a wave takes are
// 64 / sample_group pixels: tile_cols columns x row_group rows of one row group (kernels.hip, pass_column).  When every group of the pass's row list
// is row_group CONSECUTIVE image rows starting at a multiple of row_group (always, for whole images and power-of-two stripes) a tile is a fixed
// block of the image, and every triangle whose padded screen rectangle (the culling mask's) meets the tile's (dir_x, dir_y) footprint — computed
// like chunk_is_culled computes a chunk's — goes on the tile's list, nearest first.  Any primary ray that hits a triangle has its direction inside
// that triangle's rectangle, so the closest hit over the tile's list IS the closest hit over the scene.  Rebuilt with the mask when the camera
// (or the layout) changes; scenes whose lists get long (tiny triangles: > 24 per tile on average) keep the BVH walk.
bool Renderer::refresh_tile_bins(DCamera& c, const double inv[3][3], double pad, double zmin, const DPass& ps, const std::vector<uint32_t>& rows)
{
#define BINS_OUT(k) do { if (getenv("MI355RT_DEBUG_CULL")) fprintf(stderr, "[mi355rt] tile bins: not built (exit %d)\n", k); return true; } while (0)
    c.tile_ofs = nullptr; c.tile_entries = nullptr; c.tile_cols = c.tile_rg = c.tile_nblocks = 0;
    if (c.cull_valid == 0 || bvh.tris.empty() || bvh.tris.size() > (2u << 20) || getenv("MI355RT_NO_RASTER")) BINS_OUT(1);
    const uint32_t W = cfg.width, H = cfg.height, rg = ps.row_group, G = ps.sample_group;
    if (ps.use_explicit || G == 0 || 64u % G || (64u / G) % rg || ps.chunk % 64u) BINS_OUT(2);
    const uint32_t cols = 64u / G / rg;
    if (W % cols || rows.size() % rg || rows.empty() || ps.npix != rows.size() * (size_t)W) BINS_OUT(3);
    for (size_t i = 0; i < rows.size(); i += rg) {                      // every group: rg consecutive image rows from a multiple of rg
        if (rows[i] % rg) BINS_OUT(4);
        for (uint32_t k = 1; k < rg; ++k) if (rows[i + k] != rows[i] + k) BINS_OUT(5);
    }
    const bool fix_row = (ps.flags & 1u) != 0;
    std::vector<float> key(c.rot, c.rot + 16);
    key.insert(key.end(), c.origin, c.origin + 3); key.push_back(c.max_x); key.push_back(c.max_y);
    key.push_back((float)cols); key.push_back((float)rg); key.push_back(fix_row ? 1.0f : 0.0f);
    const uint32_t nblocks = W / cols, ngroups = (H + rg - 1) / rg;
    auto publish = [&]() { c.tile_ofs = d_tile_ofs_.get(); c.tile_entries = d_tile_entries_.get(); c.tile_cols = cols; c.tile_rg = rg; c.tile_nblocks = nblocks; };
    if (key == bins_key_) { if (bins_valid_) publish(); return true; }
    bins_key_ = key; bins_valid_ = false;
    const auto t_begin = std::chrono::steady_clock::now();
    const double mx = c.max_x, my = c.max_y;
    const uint64_t vmax = fix_row ? (uint64_t)H - 1 : ((uint64_t)W * H - 1) / H;
    struct Ref { uint32_t tile; float dmin; uint32_t tri; };
    std::vector<Ref> refs;
    refs.reserve(bvh.tris.size() * 6);
    const double org[3] = { c.origin[0], c.origin[1], c.origin[2] };
    if (!project_triangles(c, inv, pad, zmin)) BINS_OUT(7);
    for (size_t k = 0; k < bvh.tris.size(); ++k) {
        const BvhTri& t = bvh.tris[k];
        float v9[9];
        for (int a = 0; a < 3; ++a) { v9[a] = t.v0[a]; v9[3 + a] = t.v0[a] + t.e1[a]; v9[6 + a] = t.v0[a] + t.e2[a]; }
        const double x0 = tri_rects_[k].x0, x1 = tri_rects_[k].x1, y0 = tri_rects_[k].y0, y1 = tri_rects_[k].y1;     // the padded screen rectangle, as in the culling mask
        const double ex = 1e-4 * (x1 - x0) + 1e-6, ey = 1e-4 * (y1 - y0) + 1e-6;
        // columns cu and row indices cv (kernels.hip, primary_sample) whose jitter range [cu, cu + 1) / W, [cv, cv + 1) / H can reach the rectangle;
        // 1/100 of a column of slack covers the f32 rounding of the kernel's own expressions
        const double fx0 = (x0 - ex + mx) / (2.0 * mx) * W - 0.01, fx1 = (x1 + ex + mx) / (2.0 * mx) * W + 0.01;
        const double fy0 = (y0 - ey + my) / (2.0 * my) * H - 0.01, fy1 = (y1 + ey + my) / (2.0 * my) * H + 0.01;
        if (fx1 < 0.0 || fx0 >= (double)W || fy1 < 0.0 || fy0 > (double)vmax + 1.0) continue;
        const uint64_t c0 = (uint64_t)std::max(0.0, std::floor(fx0)), c1 = (uint64_t)std::min((double)W - 1.0, std::floor(fx1));
        const uint64_t v0 = (uint64_t)std::max(0.0, std::floor(fy0)), v1 = (uint64_t)std::min((double)vmax, std::floor(fy1));
        if (c1 < c0 || v1 < v0) continue;
        // image rows whose pixels of columns c0..c1 have cv in [v0, v1]: cv = (row * W + x) / H, or the row itself with the fixed row index
        uint64_t r0, r1;
        if (fix_row) { r0 = v0; r1 = std::min<uint64_t>(v1, H - 1); }
        else {
            const uint64_t lo = v0 * H, hi = (v1 + 1) * H - 1;                           // row * W + x in [lo, hi] for some x in [c0, c1]
            r0 = lo > c1 ? (lo - c1 + W - 1) / W : 0; r1 = hi >= c0 ? (hi - c0) / W : 0;
            if (hi < c0) continue;
            r1 = std::min<uint64_t>(r1, H - 1);
        }
        if (r1 < r0) continue;
        const double org_d = point_triangle_distance_lower(org, v9);
        const float dmin = (float)std::max((org_d - pad) * (1.0 - 1e-6), 0.0);
        const float dmin_lo = (double)dmin > std::max((org_d - pad) * (1.0 - 1e-6), 0.0) ? std::nextafterf(dmin, 0.0f) : dmin;
        for (uint64_t g = r0 / rg; g <= r1 / rg && g < ngroups; ++g) {
            const uint64_t ra = g * rg, rb = std::min<uint64_t>(ra + rg - 1, H - 1);
            for (uint64_t b = c0 / cols; b <= c1 / cols; ++b) {
                const uint64_t xa = b * cols, xb = xa + cols - 1;
                // the tile's own cv range (every pixel of it lies between its first and its last): must meet [v0, v1]
                const uint64_t ta = fix_row ? ra : (ra * W + xa) / H, tb = fix_row ? rb : (rb * W + xb) / H;
                if (tb < v0 || ta > v1) continue;
                refs.push_back(Ref{ (uint32_t)(g * nblocks + b), dmin_lo, (uint32_t)k });
            }
        }
    }
    const size_t ntiles = (size_t)nblocks * ngroups;
    std::vector<uint2> ofs(ntiles, make_uint2(0u, 0u));
    for (const Ref& r : refs) ++ofs[r.tile].y;
    size_t live = 0; uint32_t run = 0;
    for (uint2& o : ofs) { o.x = run; run += o.y; live += o.y != 0; o.y = 0; }
    if (refs.size() > ((size_t)64 << 20) || (live && refs.size() > 24 * live)) BINS_OUT(8);     // long lists: the BVH walk is the better search
    std::vector<uint2> entries(std::max<size_t>(refs.size(), 1));
    for (const Ref& r : refs) { uint2& o = ofs[r.tile]; uint32_t bits; std::memcpy(&bits, &r.dmin, 4); entries[o.x + o.y++] = make_uint2(r.tri, bits); }
    for (const uint2& o : ofs) if (o.y > 1)
        std::sort(entries.begin() + o.x, entries.begin() + o.x + o.y, [](const uint2& a, const uint2& b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });   // non-negative floats order like their bits
    if (!bind()) return false;
    // kernels of earlier calls may still read the old bins (as with the mask): wait, then replace
    (void)hipStreamSynchronize(stream_);
    for (Slice& sl : slices_) if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    if (ofs.size() * sizeof(uint2) > d_tile_ofs_.bytes() && d_tile_ofs_.alloc(ofs.size() * sizeof(uint2), &hbm_bytes_) != hipSuccess) BINS_OUT(9);
    if (entries.size() * sizeof(uint2) > d_tile_entries_.bytes() && d_tile_entries_.alloc((entries.size() + entries.size() / 4) * sizeof(uint2), &hbm_bytes_) != hipSuccess) BINS_OUT(10);    // 1/4 slack
    if (hipMemcpy(d_tile_ofs_.get(), ofs.data(), ofs.size() * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess) BINS_OUT(11);
    if (hipMemcpy(d_tile_entries_.get(), entries.data(), entries.size() * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess) BINS_OUT(12);
    bins_valid_ = true; bins_entries_ = refs.size();
    bins_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    publish();
    if (getenv("MI355RT_DEBUG_CULL")) fprintf(stderr, "[mi355rt] tile bins: %u x %u tiles of %u columns x %u rows, %zu live, %zu entries (%.1f per live tile), %.1f ms\n", nblocks, ngroups, cols, rg, live, refs.size(), live ? (double)refs.size() / live : 0.0, bins_ms_);
    return true;
}
#undef BINS_OUT

DCamera Renderer::device_camera(const DPass* layout, const std::vector<uint32_t>* rows)
{
    DCamera c;
    std::memcpy(c.rot, camera.rotation().e, sizeof c.rot);
    Vec4 pos = camera.orientation() * Vec4(0.0f, 0.0f, 0.0f, 1.0f);      // camera.rs:88
    c.origin[0] = pos.x; c.origin[1] = pos.y; c.origin[2] = pos.z;
    c.max_x = camera.max_x(); c.max_y = camera.max_y();
    c.width = cfg.width; c.height = cfg.height;
    c.lens = lens_derive(lens_.model, lens_.radius, lens_.focus, lens_.width_world, c.rot, c.max_x, c.max_y, cfg.width, cfg.height);
    // Screen-space bounds of the padded scene box for the primary-chunk frustum culling (kernels.hip,
    // chunk_is_culled).  dir = (dir_x, -dir_y, 1) * R3x3  =>  (dir_x, -dir_y, 1) ~ (p - origin) * R3x3^-1.
    // Valid only if every corner of the box is in front of the camera; computed in double, widened.
    c.cull_valid = 0;
    std::memset(c.cull_rect, 0, sizeof c.cull_rect);
    c.cull_mask = nullptr; c.mask_x0 = c.mask_y0 = 0.0f; c.mask_inv_cx = c.mask_inv_cy = 0.0f;
    c.tile_ofs = nullptr; c.tile_entries = nullptr; c.tile_cols = c.tile_rg = c.tile_nblocks = 0;
    if (!cull_boxes_.empty() && mode_ != kModeOctreeWalk && !getenv("MI355RT_NO_CULL")) {
        const float* e = c.rot;
        const double m[3][3] = { { e[0], e[1], e[2] }, { e[4], e[5], e[6] }, { e[8], e[9], e[10] } };
        const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                         + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
        if (std::fabs(det) > 1e-12) {
            double inv[3][3];
            inv[0][0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) / det; inv[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; inv[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
            inv[1][0] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) / det; inv[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; inv[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
            inv[2][0] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) / det; inv[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det; inv[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
            double diag = 0.0;
            for (int a = 0; a < 3; ++a) diag += (double)(bvh.scene_max[a] - bvh.scene_min[a]) * (bvh.scene_max[a] - bvh.scene_min[a]);
            const double pad = 1e-3 * std::sqrt(diag) + 1e-6;            // on top of the (already padded) BVH boxes
            bool front = true;
            uint32_t n = 0;
            for (const auto& bx : cull_boxes_) {
                double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
                for (int k = 0; k < 8 && front; ++k) {
                    double w[3];
                    for (int a = 0; a < 3; ++a) w[a] = ((k >> a) & 1 ? bx[3 + a] + pad : bx[a] - pad) - c.origin[a];
                    const double vx = w[0] * inv[0][0] + w[1] * inv[1][0] + w[2] * inv[2][0];
                    const double vy = w[0] * inv[0][1] + w[1] * inv[1][1] + w[2] * inv[2][1];
                    const double vz = w[0] * inv[0][2] + w[1] * inv[1][2] + w[2] * inv[2][2];
                    if (!(vz > 1e-6 * std::sqrt(diag))) { front = false; break; }
                    const double dx = vx / vz, dy = -vy / vz;
                    x0 = std::min(x0, dx); x1 = std::max(x1, dx); y0 = std::min(y0, dy); y1 = std::max(y1, dy);
                }
                if (!front) break;
                const double mx = 1e-4 * (x1 - x0) + 1e-6, my = 1e-4 * (y1 - y0) + 1e-6;
                c.cull_rect[n][0] = (float)(x0 - mx); c.cull_rect[n][1] = (float)(x1 + mx);
                c.cull_rect[n][2] = (float)(y0 - my); c.cull_rect[n][3] = (float)(y1 + my);
                ++n;
            }
            if (front) c.cull_valid = n;         // a box behind / around the camera: no culling at all
            // the mask pads every vertex by ten times what the BVH pads its boxes with (bvh.cpp: 2e-5 of the diagonal) — the same assumption about
            // the triangle test's rounding that the traversal itself rests on, with a wider margin
            if (front) (void)refresh_cull_mask(c, inv, 2e-4 * std::sqrt(diag) + 1e-7, 1e-6 * std::sqrt(diag), layout != nullptr);
            if (front && layout && rows) (void)refresh_tile_bins(c, inv, 2e-4 * std::sqrt(diag) + 1e-7, 1e-6 * std::sqrt(diag), *layout, *rows);
            if (getenv("MI355RT_DEBUG_CULL")) { fprintf(stderr, "[mi355rt] cull rects %u front %d max_x %g\n", n, (int)front, c.max_x); for (uint32_t k = 0; k < n; ++k) fprintf(stderr, "   x [%g, %g] y [%g, %g]\n", c.cull_rect[k][0], c.cull_rect[k][1], c.cull_rect[k][2], c.cull_rect[k][3]); }
        }
    }
    return c;
}

#define HIP_ALLOC(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { alloc_failed_ = e__ == hipErrorOutOfMemory; free_pass_buffers(); return fail(e__, #expr); } } while (0)

void Renderer::free_pass_buffers()
{
    for (Slice& sl : slices_) { sl.release_pass_buffers(); sl.d_block_culled.reset(); sl.cull_key.clear(); }
}

bool Renderer::ensure_pass_capacity(Slice& sl, size_t nsamples)
{
    alloc_failed_ = false;
    if (nsamples <= sl.capacity) return true;
    for (Slice& o : slices_) if (o.stream) HIP_TRY(hipStreamSynchronize(o.stream));
    sl.release_pass_buffers();          // grow: release this slice's buffers only
    const size_t nchunks = (nsamples + kChunk - 1) / kChunk;
    const size_t records = nchunks * kChunk * records_per_sample_;
    // the kernels index records, light-term floats and hit flags with 32 bits (byte offsets are 64-bit)
    if (nsamples > 0x7FFFFFFFull || records > 0x3FFFFFFFull || nchunks * kChunk * nodes_per_sample * std::max(nlights_, 1u) * 3ull > 0xFFFFFFFFull) {
        last_error = "pass too large"; alloc_failed_ = true; return false;     // the caller retries with a smaller pass
    }
    // (n_radiance, n_shadow) per chunk: the fused 50-row launch cuts the same samples into chunks as small as kMinChunk
    const size_t count_entries = nchunks * kChunk / std::min(kChunk, kMinChunk);
    // MI355RT_DEBUG_GUARD: every pass buffer gets a 256-byte tail filled with 0xA5 that check_guards() reads back
    // (tests/test_gpu_dropin.py: no launch may write past the sizes computed here)
    const size_t guard = getenv("MI355RT_DEBUG_GUARD") ? kGuardBytes : 0;
    for (int i = 0; i < 2; ++i) {
        HIP_ALLOC(sl.d_queue[i].alloc(records * kRayRecordBytes, &hbm_bytes_, guard));
        HIP_ALLOC(sl.d_chunk_counts[i].alloc(count_entries * 8, &hbm_bytes_, guard));
    }
    HIP_ALLOC(sl.d_hits.alloc(records * 16, &hbm_bytes_, guard));
    HIP_ALLOC(sl.d_hit_prim.alloc(records * 4, &hbm_bytes_, guard));
    HIP_ALLOC(sl.d_slot_L.alloc(nchunks * kChunk * nodes_per_sample * std::max(nlights_, 1u) * 12, &hbm_bytes_, guard));
    HIP_ALLOC(sl.d_sample_slot.alloc(nchunks * kChunk * 4, &hbm_bytes_, guard));
    HIP_ALLOC(sl.d_slot_ps.alloc(nchunks * kChunk * 8, &hbm_bytes_, guard));
    HIP_ALLOC(sl.d_live.alloc((nchunks + kMaxCursors) * 4, &hbm_bytes_, guard));
    sl.capacity = nsamples;
    sl.queue_records = records;
    sl.count_entries = count_entries;
    return true;
}

// Split the owned rows into `nslices` interleaved shares (blocks of stripe_rows rows, round-robin) and
// upload each slice's row list.
bool Renderer::assign_slice_rows(uint32_t nslices)
{
    if (rows_assigned_for_ == nslices) return true;
    for (Slice& o : slices_) if (o.stream) HIP_TRY(hipStreamSynchronize(o.stream));
    for (Slice& o : slices_) { o.rows.clear(); o.cull_key.clear(); }       // other rows: other pixel blocks, other verdicts
    for (size_t i = 0; i < owned_rows.size(); ++i) slices_[(i / cfg.stripe_rows) % nslices].rows.push_back(owned_rows[i]);
    for (uint32_t s = 0; s < nslices; ++s)
        if (!slices_[s].rows.empty()) HIP_TRY(hipMemcpy(slices_[s].d_rows.get(), slices_[s].rows.data(), slices_[s].rows.size() * 4, hipMemcpyHostToDevice));
    rows_assigned_for_ = nslices;
    return true;
}

// One wavefront pass: `nrows` rows starting at d_rows[row0], spp samples per pixel.
// Fill the pass descriptor shared by the wavefront kernels and the fused kernel.
void Renderer::describe_pass(DPass& ps, const Slice& sl, const PassRequest& rq, uint32_t npix, size_t nsamples, uint32_t chunk) const
{
    ps = DPass{};
    ps.rows = rq.d_rows; ps.row0 = rq.row0; ps.row_wrap = rq.row_wrap; ps.npix = npix; ps.nsamples = (uint32_t)nsamples;
    ps.spp = npix ? (uint32_t)(nsamples / npix) : 1u;
    // samples of a pixel kept together in the pass order (kernels.hip, sample_of): 2 — thai2 frame 21.1 / 20.7 / 20.7 / 20.9 / 21.5 / 21.6 ms at
    // 1 / 2 / 4 / 8 / 16 / 64, one rank's share of eight 3.27 / 3.24 / 3.30 / 3.34 / 3.40 / 3.63 ms (profiles/r03_notes.md); the largest divisor of spp <= the wish.
    // With the primary rays going through the tile bins (a wave's tile is 64 / group pixels: shorter lists for smaller tiles) and most shadow rays
    // never made: 15.5 / 15.4 / 15.1 / 15.5 ms at 2 / 4 / 8 / 16 — 8 since.
    uint32_t group = std::max(1u, std::min(8u, ps.spp));
    while (ps.spp % group) --group;
    // a power of two by preference (12 spp: 4, not 6): the tile bins and the cached culling verdicts need the group to divide a wave's 64 samples
    if (64u % group) { uint32_t p2 = 8u; while (p2 > 1u && (p2 > group || ps.spp % p2)) p2 >>= 1; group = p2; }
    ps.sample_group = group;
    // tile groups of 8 rows, or of the stripe height when rows are dealt (to ranks and to slices) in blocks of fewer rows: a group
    // that spans two blocks lying far apart in the image makes loose culling rectangles and incoherent tiles
    ps.row_group_shift = 3; while (ps.row_group_shift > 0 && (1u << ps.row_group_shift) > cfg.stripe_rows) --ps.row_group_shift;
    // ... and of a height that divides the pass's rows when there is one (1050 rows: groups of 2, not 4 with a ragged last group): whole groups everywhere is what
    // the tile bins of the primary rays need, and costs nothing
    if (!rq.explicit_sample && cfg.width) { const uint32_t prow = npix / cfg.width; while (ps.row_group_shift > 0 && prow % (1u << ps.row_group_shift)) --ps.row_group_shift; }
    ps.row_group = 1u << ps.row_group_shift;
    ps.seed = (uint32_t)cfg.seed; ps.flags = cfg.flags; ps.recursions = cfg.recursions; ps.spread = cfg.spread;
    ps.nodes_per_sample = nodes_per_sample;
    ps.nslots = (uint32_t)((nsamples + chunk - 1) / chunk) * chunk;
    std::memcpy(ps.level_first, level_first, sizeof ps.level_first);
    ps.use_explicit = rq.explicit_sample ? 1u : 0u; ps.explicit_pixel = rq.epixel; ps.explicit_sampleno = rq.esample;
    ps.chunk = chunk; ps.nchunks = (uint32_t)((nsamples + chunk - 1) / chunk); ps.region = chunk * records_per_sample_;
    ps.hit_prim = sl.d_hit_prim.get(); ps.qstride = sl.queue_records; ps.slot_ps = (uint2*)sl.d_slot_ps.get();
    ps.stack_depth = traversal_rows(); ps.list_cap = chunk * max_level_nodes_;
    // live-chunk lists (device_types.hpp): with the chunk size the buffers were sized for.
    // Not with the direct octree walk: its trace launch strides over ALL chunks, and the ray counts of the chunks the shade launches no longer visit
    // are whatever an earlier pass left there.
    ps.live = nullptr; ps.live_count = nullptr; ps.live_cap = 0;
    if (chunk == kChunk && sl.d_live && !rq.explicit_sample && mode_ != kModeOctreeWalk) {
        ps.live = sl.d_live.get(); ps.live_count = sl.d_ctrl.get(); ps.live_cap = (ps.nchunks + kMaxCursors - 1u) / kMaxCursors;
    }
}

// MI355RT_DEBUG_UTIL: load-balance diagnostics of one trace launch of a counting handle (debug only: synchronises).  Before the launch ...
bool Renderer::balance_debug_reset()
{
    DCounters init{};
    HIP_TRY(hipMemcpy(&init, d_counters_.get(), sizeof init, hipMemcpyDeviceToHost));
    init.t_first_end = ~0ull; init.t_start = ~0ull; init.t_last_end = 0; init.t_sum_end = 0; init.n_waves = 0;
    HIP_TRY(hipMemcpy(d_counters_.get(), &init, sizeof init, hipMemcpyHostToDevice));
    return true;
}
// ... and after it (and the round's confirm launch)
bool Renderer::balance_debug_report(hipStream_t st, uint32_t r)
{
    DCounters c0{};
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&c0, d_counters_.get(), sizeof c0, hipMemcpyDeviceToHost));
    {   // lane census of the launch (summed over the counter shards; cumulative over the call's launches: print differences)
        DCounters sh[kShards], t{};
        HIP_TRY(hipMemcpy(sh, d_counters_.get(), sizeof sh, hipMemcpyDeviceToHost));
        for (const DCounters& x : sh) { t.lanes_inner += x.lanes_inner; t.lanes_leaf += x.lanes_leaf; t.lanes_done += x.lanes_done; t.lane_samples += x.lane_samples;
                                        t.refills += x.refills; t.refill_passes += x.refill_passes; t.refill_rays += x.refill_rays; t.inner_execs += x.inner_execs; t.leaf_execs += x.leaf_execs; }
        static DCounters prev{};
        if (t.lane_samples < prev.lane_samples) prev = DCounters{};
        const double it = (double)(t.lane_samples - prev.lane_samples);
        if (it > 0)
            fprintf(stderr, "[mi355rt] trace round %u census: iterations %.0f, lanes at inner %.1f / at leaf %.1f / idle-or-finished %.1f per iteration; inner execs %.2f, leaf execs %.2f per iteration; refills %llu, passes %llu, rays per refill %.1f\n",
                    r, it, (t.lanes_inner - prev.lanes_inner) / it, (t.lanes_leaf - prev.lanes_leaf) / it, (t.lanes_done - prev.lanes_done) / it,
                    (t.inner_execs - prev.inner_execs) / it, (t.leaf_execs - prev.leaf_execs) / it,
                    t.refills - prev.refills, t.refill_passes - prev.refill_passes, (double)(t.refill_rays - prev.refill_rays) / std::max<double>(1.0, (double)(t.refills - prev.refills)));
        prev = t;
    }
    if (c0.n_waves)
        fprintf(stderr, "[mi355rt] trace round %u: %llu waves, mean wave busy %.1f us, first wave out of work at %.1f us, last at %.1f us\n", r, c0.n_waves,
                (double)c0.t_sum_end / c0.n_waves / 100.0, (double)(c0.t_first_end - c0.t_start) / 100.0, (double)(c0.t_last_end - c0.t_start) / 100.0);
    return true;
}

// Culling verdicts per pixel block, computed once per camera and layout (DPass::block_culled) instead of per launch and chunk
// (needs chunks that hold whole pixels — the sample group divides the chunk — and sample groups that are whole numbers of chunks: then every sample of a pixel
// lies in chunks of ONE block)
bool Renderer::cached_cull_verdicts(Slice& sl, const DCamera& cam, DPass& ps, uint32_t nrows)
{
    ps.block_culled = nullptr; ps.cull_blocks = 0;
    if (cam.cull_valid == 0 || mode_ == kModeOctreeWalk || ps.chunk % ps.sample_group != 0 || ((size_t)ps.npix * ps.sample_group) % ps.chunk != 0 || getenv("MI355RT_NO_CULL_CACHE")) return true;
    const size_t nblocks = (size_t)ps.npix * ps.sample_group / ps.chunk;
    std::vector<float> key(cam.rot, cam.rot + 16);
    key.insert(key.end(), cam.origin, cam.origin + 3); key.push_back(cam.max_x); key.push_back(cam.max_y);
    key.push_back((float)nrows); key.push_back((float)ps.chunk); key.push_back((float)ps.sample_group); key.push_back((float)ps.row_group);
    key.push_back((float)(ps.flags & 1u)); key.push_back(cam.cull_mask ? 1.0f : 0.0f); key.push_back((float)nblocks);
    if (nblocks * 4 > sl.d_block_culled.bytes()) {
        HIP_TRY(hipStreamSynchronize(sl.stream));
        if (sl.d_block_culled.alloc(nblocks * 4, &hbm_bytes_) != hipSuccess) (void)hipGetLastError();
        sl.cull_key.clear();
    }
    if (sl.d_block_culled) {
        if (key != sl.cull_key) {          // stream-ordered behind the launches that read the old verdicts
            HIP_TRY(launch_cull_blocks(sl.stream, cam, ps, (uint32_t)nblocks, sl.d_block_culled.get()));
            sl.cull_key = key;
        }
        ps.block_culled = sl.d_block_culled.get(); ps.cull_blocks = (uint32_t)nblocks;
    }
    return true;
}

// A wavefront pass: buffers, descriptor and cursors; then round by round trace (+ confirm) (+ shade); then resolve.  Every launch goes
// to the slice's stream.
bool Renderer::run_pass(Slice& sl, const PassRequest& rq)
{
    const RayFeed* feed = rq.feed;
    const bool free_rays = feed != nullptr && feed->mode == kRaysFree;       // mi355rt_trace_rays: the pass's samples are `count` rays, not pixels
    const uint32_t npix = rq.explicit_sample ? 1u : free_rays ? feed->count : rq.nrows * cfg.width;
    const size_t nsamples = (size_t)npix * rq.spp;
    if (nsamples == 0) return true;
    if (!ensure_pass_capacity(sl, nsamples)) return false;
    DPass ps;
    describe_pass(ps, sl, rq, npix, nsamples, kChunk);
    ps.tile_active = rq.tile_active; ps.tiles_x = tiles_x();
    // the tile bins of the primary rays need a pass that walks the slice's whole row list (render(); not the odd row windows of the other callers)
    // (nor a ray-fed or a lens pass: its primary rays are not the pinhole camera's, so nothing that is derived from the camera — bins, culling rectangles, cached verdicts — holds)
    const bool whole = !feed && !rq.explicit_sample && rq.d_rows == sl.d_rows.get() && rq.row0 == 0 && rq.nrows == sl.rows.size() && rq.row_wrap == kNoRowWrap;
    DCamera cam = device_camera(whole ? &ps : nullptr, whole ? &sl.rows : nullptr);
    // the feed of the primary round (device_types.hpp); a lens pass with a tile mask has instantiations of its own
    static_assert(kLensPinhole == MI355RT_LENS_PINHOLE && kLensThin == MI355RT_LENS_THIN && kLensOrtho == MI355RT_LENS_ORTHO, "lens_feed takes mi355rt_lens::model");
    const uint32_t rays = feed == nullptr ? kFeedCamera : feed->mode != kRaysOfLens ? kFeedRays : lens_feed(lens_.model, rq.tile_active != nullptr);
    if (rays != kFeedCamera) { cam.cull_valid = 0; cam.cull_mask = nullptr; cam.tile_ofs = nullptr; cam.tile_entries = nullptr; }
    if (rays == kFeedRays) {
        ps.ray_in = feed->rays; ps.ray_keys = feed->keys; ps.ray_hit = feed->hit; ps.ray_mode = feed->mode; ps.ray_base = feed->base; ps.ray_npix = cfg.width * cfg.height;
    }
    if (whole && !cached_cull_verdicts(sl, cam, ps, rq.nrows)) return false;
    // the work cursors: zeroed at creation and again by the resolve kernel of every pass that ran to its end
    hipStream_t st = sl.stream;
    if (!sl.ctrl_clean) HIP_TRY(hipMemsetAsync(sl.d_ctrl.get(), 0, kMaxRounds * kCtrlWordsPerRound * 4, st));
    sl.ctrl_clean = false;
    const bool count = (cfg.flags & MI355RT_FLAG_COUNT_STEPS) != 0;
    const bool timed = (cfg.flags & MI355RT_FLAG_TIME_KERNELS) != 0;
    // true closest hits -> the reference intersector's answers; settles the shadow rays of a round.  One-leaf octrees: done in the
    // trace kernel.  Radiance hits: confirmed by the round's SHADE kernel, which loads the ray and the hit record anyway (primary
    // round: no confirm launch at all; secondary rounds: the confirm launch handles the shadow records only).  24.3 -> 23.3 ms per frame.
    const bool confirm_here = mode_ == kModeConfirm && !dscene_.oct_single_leaf;
    // round r: trace the rays of level r (+ the shadow rays emitted by level r-1), then shade level r
    for (uint32_t r = 0; r < cfg.recursions + 2; ++r) {
        // Primary round with tile bins: the shade launch finds the closest hits itself (kernels.hip, shade_chunk<RASTER>) — no trace launch at all.
        const bool fuse_primary = r == 0 && cam.tile_ofs != nullptr && mode_ != kModeOctreeWalk;
        const void* in_q = r == 0 ? nullptr : sl.d_queue[(r - 1) & 1].get();
        const void* in_c = r == 0 ? nullptr : sl.d_chunk_counts[(r - 1) & 1].get();
        const bool balance_dbg = !fuse_primary && count && getenv("MI355RT_DEBUG_UTIL") && mode_ != kModeOctreeWalk;
        if (!fuse_primary) {
            if (timed) {
                if (ev_used_ + 2 > ev_pool_.size()) {
                    for (int k = 0; k < 2; ++k) { hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); ev_pool_.push_back(ev); }
                }
                HIP_TRY(hipEventRecord(ev_pool_[ev_used_], st));
                ev_secondary_.resize(ev_pool_.size() / 2); ev_secondary_[ev_used_ / 2] = r > 0;
            }
            if (balance_dbg && !balance_debug_reset()) return false;
            if (mode_ == kModeOctreeWalk)
                HIP_TRY(launch_trace_octree(st, num_cus_, r == 0, dscene_, cam, ps, in_q, in_c, sl.d_hits.get(), sl.d_slot_L.get(), d_film_n_.get(), r == 0 ? rays : kFeedCamera));
            else
                HIP_TRY(launch_trace(st, num_cus_, r == 0, count, mode_ == kModeConfirm, dscene_, cam, ps, in_q, in_c, sl.d_hits.get(), sl.d_ctrl.get() + r * kCtrlWordsPerRound, sl.d_slot_L.get(), d_film_n_.get(), d_counters_.get(), r == 0 ? rays : kFeedCamera));
            if (timed) { HIP_TRY(hipEventRecord(ev_pool_[ev_used_ + 1], st)); ev_used_ += 2; }
            ++launches_;
        }
        const bool shade_walks = confirm_here && r <= cfg.recursions;
        if (confirm_here && r != 0)         // (the primary round's shade kernel confirms its hits, and there are no shadow rays yet)
            HIP_TRY(launch_confirm(st, num_cus_, false, shade_walks, dscene_, cam, ps, in_q, in_c, sl.d_hits.get(), sl.d_ctrl.get() + r * kCtrlWordsPerRound + kConfirmCursorOffset, sl.d_slot_L.get(), d_film_n_.get()));
        if (balance_dbg && !balance_debug_report(st, r)) return false;
        if (r <= cfg.recursions)
            HIP_TRY(launch_shade(st, num_cus_, r == 0, shade_walks, dscene_, cam, ps, r, in_q, in_c, sl.d_hits.get(), sl.d_queue[r & 1].get(), sl.d_chunk_counts[r & 1].get(), sl.d_ctrl.get() + r * kCtrlWordsPerRound + kShadeCursorOffset, sl.d_slot_L.get(), sl.d_sample_slot.get(), d_film_n_.get(), d_counters_.get(), fuse_primary, r == 0 ? rays : kFeedCamera));
    }
    if (free_rays) HIP_TRY(launch_resolve_rays(st, ps, nlights_, sl.d_slot_L.get(), sl.d_sample_slot.get(), feed->rgb, feed->direct, feed->tuv, feed->prim, sl.d_ctrl.get()));
    else HIP_TRY(launch_resolve(st, ps, cfg.width, nlights_, sl.d_slot_L.get(), sl.d_sample_slot.get(), d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_film_direct_.get(), d_debug_color_.get(), sl.d_ctrl.get(),
                                d_film_lights_.get(), lights_stride()));
    sl.ctrl_clean = true;
    return true;
}

bool Renderer::begin_call()
{
    if (!quiet()) return false;
    call_done_valid_ = false;
    ev_used_ = 0; launches_ = 0;
    counts_pending_ = false;
    HIP_TRY(hipMemsetAsync(d_counters_.get(), 0, sizeof(DCounters) * kShards, stream_));
    HIP_TRY(hipEventRecord(ev_begin_, stream_));
    active_slices_ = 1;
    return true;
}

// Download the device counters of the call that just ended (the stream must be idle).
bool Renderer::fetch_counts(uint64_t primary, bool timed_call)
{
    DCounters c{};
    const DCounters* shard = h_counters_.get();          // pinned; filled by the asynchronous copy queue_counts_copy() put behind the call's kernels
    for (uint32_t i = 0; i < kShards; ++i) {
        const DCounters& s = shard[i];
        c.bounce += s.bounce; c.shadow += s.shadow; c.primary_hits += s.primary_hits;
        c.nodes_visited += s.nodes_visited; c.tris_tested += s.tris_tested; c.overflow |= s.overflow;
        c.inner_execs += s.inner_execs; c.leaf_execs += s.leaf_execs; c.primary_culled += s.primary_culled; c.shadow_skipped += s.shadow_skipped; c.bounce_skipped += s.bounce_skipped;
        c.t_sum_cycles += s.t_sum_cycles; c.t_sum_real += s.t_sum_real; c.refill_rays += s.refill_rays;
        for (int k = 0; k < 6; ++k) c.visits_below[k] += s.visits_below[k];
    }
    counts = mi355rt_ray_counts{};
    counts.primary = primary; counts.bounce = c.bounce + c.bounce_skipped; counts.shadow = c.shadow + c.shadow_skipped; counts.primary_hits = c.primary_hits;
    counts.shadow_skipped = c.shadow_skipped;     // shadow rays of mod.rs:226 that were never made: the light's depth map proved them free
    counts.bounce_skipped = c.bounce_skipped;     // reflection rays of mod.rs:156-158 that were never made: their triangle's direction mask proved that they hit nothing
    rays_read_ = c.refill_rays;                   // MI355RT_FLAG_COUNT_STEPS: what the trace launches took from their queues (mi355rt_debug_rays_read)
    counts.nodes_visited = c.nodes_visited; counts.tris_tested = c.tris_tested; counts.trace_launches = launches_;
    counts.inner_execs = c.inner_execs; counts.leaf_execs = c.leaf_execs; counts.primary_culled = c.primary_culled;
    if (getenv("MI355RT_DEBUG_UTIL") && c.nodes_visited)
        fprintf(stderr, "[mi355rt] inner-node visits with node index < 64 / 128 / 256 / 512 / 1024 / 2048: %.3f / %.3f / %.3f / %.3f / %.3f / %.3f of %llu\n", (double)c.visits_below[0] / c.nodes_visited, (double)c.visits_below[1] / c.nodes_visited,
                (double)c.visits_below[2] / c.nodes_visited, (double)c.visits_below[3] / c.nodes_visited, (double)c.visits_below[4] / c.nodes_visited, (double)c.visits_below[5] / c.nodes_visited, c.nodes_visited);
    if (getenv("MI355RT_DEBUG_UTIL")) fprintf(stderr, "[mi355rt] inner execs %llu (lane util %.3f) leaf execs %llu (lane util %.3f)\n", c.inner_execs, c.inner_execs ? (double)c.nodes_visited / (64.0 * c.inner_execs) : 0.0, c.leaf_execs, c.leaf_execs ? (double)c.tris_tested / (64.0 * c.leaf_execs) : 0.0);
    if (timed_call) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev_begin_, ev_end_));
        counts.total_ms = ms;
    }
    double tms = 0.0, sms = 0.0; uint64_t nsec = 0;
    for (size_t i = 0; i + 1 < ev_used_; i += 2) {           // MI355RT_FLAG_TIME_KERNELS: events around every trace / fused launch
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, ev_pool_[i], ev_pool_[i + 1]));
        tms += t;
        if (i / 2 < ev_secondary_.size() && ev_secondary_[i / 2]) { sms += t; ++nsec; }
    }
    counts.trace_ms = tms; counts.trace_secondary_ms = sms; counts.trace_secondary_launches = nsec;
    // s_memtime ticks are shader cycles, s_memrealtime ticks 10 ns: the clock the trace waves ran at (COUNT builds stamp both)
    counts.shader_clock_mhz = c.t_sum_real ? (double)c.t_sum_cycles / (double)c.t_sum_real * 100.0 : 0.0;
    if (c.overflow) { last_error = (c.overflow & 2u) ? "internal: traversal stack overflow (instrumented build: a ray held more deferred nodes than the stack has rows)" : "internal: ray queue overflow"; return false; }
    return true;
}

// the call's device counters -> the pinned host mirror, stream-ordered behind the call's kernels (one wait serves both)
bool Renderer::queue_counts_copy()
{
    HIP_TRY(hipMemcpyAsync(h_counters_.get(), d_counters_.get(), sizeof(DCounters) * kShards, hipMemcpyDeviceToHost, stream_));
    return true;
}

// wait == false (mi355rt_render_async): everything is queued — the slices joined on the main stream, the counters' copy behind them —
// and the call returns; mi355rt_last_counts / mi355rt_synchronize wait.  Consecutive frames then run back to back on the device
// instead of one host round trip apart (a few % of a 3 ms frame: one rank's share of a strong-scaled frame).
bool Renderer::join_slices()
{
    for (uint32_t i = 1; i < active_slices_; ++i) {          // join the slices on the main stream
        HIP_TRY(hipEventRecord(slices_[i].done, slices_[i].stream));
        HIP_TRY(hipStreamWaitEvent(stream_, slices_[i].done, 0));
    }
    active_slices_ = 1;
    return true;
}

bool Renderer::end_call(uint64_t primary, bool wait)
{
    if (!join_slices()) return false;
    HIP_TRY(hipEventRecord(ev_end_, stream_));
    if (!queue_counts_copy()) return false;
    if (!wait) { counts_pending_ = true; pending_primary_ = primary; pending_timed_ = true; return true; }
    HIP_TRY(hipStreamSynchronize(stream_));
    return fetch_counts(primary, true);
}

// Counters of the last call.  A 50-row frame (trace_frame_additive) returns without waiting for the device;
// its counters are fetched when somebody asks for them.
bool Renderer::last_counts(mi355rt_ray_counts& out)
{
    if (counts_pending_) {
        if (!bind()) return false;
        if (call_done_valid_) HIP_TRY(hipEventSynchronize(ev_call_done_));       // a 50-row frame: its kernel and its counters' copy, not what was queued behind them
        else HIP_TRY(hipStreamSynchronize(stream_));
        counts_pending_ = false;
        const bool timed = pending_timed_; pending_timed_ = false;
        if (!fetch_counts(pending_primary_, timed)) return false;
    }
    out = counts;
    return true;
}

// The 50-row window of one trace_frame_additive call (mod.rs:87,114) as runs of the device-resident owned-row
// list: entry i of run k is owned_rows[(first + i) % owned], and no row occurs twice inside a run (a row can
// occur more than once per call only when height < 50; each occurrence must see the previous one's film update).
struct FrameWindow { uint32_t first = 0, total = 0, next_row = 0; };
static FrameWindow frame_window(uint32_t current_row, uint32_t height, uint32_t stripe_rows, uint32_t world, uint32_t rank, const std::vector<uint32_t>& owned)
{
    FrameWindow w;
    uint32_t row = current_row;
    bool have_first = false;
    for (int k = 0; k < 50; ++k) {
        if ((row / stripe_rows) % world == rank) {
            if (!have_first) { w.first = (uint32_t)(std::lower_bound(owned.begin(), owned.end(), row) - owned.begin()); have_first = true; }
            ++w.total;
        }
        row = (row + 1) % height;
    }
    w.next_row = row;
    return w;
}

void Renderer::mark_dirty_window(uint32_t first, uint32_t total)
{
    const uint32_t nown = (uint32_t)owned_rows.size();
    for (uint32_t i = 0; i < total && i < nown; ++i) ldr_dirty_[owned_rows[(first + i) % nown]] = 1;
}

uint32_t Renderer::trace_frame_additive()
{
    if (has_light_films()) { last_error = "mi355rt_trace_frame_additive: not available on a handle created with MI355RT_FLAG_LIGHT_FILMS (the fused 50-row frame keeps no light films); mi355rt_render instead"; return 0; }
    const uint32_t nown = (uint32_t)owned_rows.size();
    const FrameWindow win = frame_window(current_row, cfg.height, cfg.stripe_rows, cfg.stripe_world, cfg.stripe_rank, owned_rows);
    // instrumented / timed / reference-exact-octree calls go through the wavefront rounds (several launches, waits for the device)
    const bool wavefront = (cfg.flags & MI355RT_FLAG_COUNT_STEPS) != 0 || mode_ == kModeOctreeWalk
                           || fused_pass_lds_rows(traversal_rows(), max_level_nodes_, records_per_sample_) > 60u || getenv("MI355RT_NO_FUSED");
    if (wavefront) {
        if (!begin_call()) return 0;
        for (uint32_t done = 0; done < win.total; done += nown) {
            PassRequest rq;
            rq.d_rows = d_owned_rows_.get(); rq.row0 = (win.first + done) % nown; rq.nrows = std::min(nown, win.total - done); rq.row_wrap = nown;
            if (!run_pass(slices_[0], rq)) return 0;
        }
        current_row = win.next_row;
        mark_dirty_window(win.first, win.total);
        if (!end_call((uint64_t)win.total * cfg.width)) return 0;
        return 50u * cfg.width;
    }
    // fast path: one launch per run, nothing uploaded, nothing waited for
    if (!bind()) return 0;
    ev_used_ = 0; launches_ = 0;
    const bool timed = (cfg.flags & MI355RT_FLAG_TIME_KERNELS) != 0;
    const DCamera cam = device_camera();
    std::vector<float> cam_key(cam.rot, cam.rot + 16);
    cam_key.insert(cam_key.end(), cam.origin, cam.origin + 3); cam_key.push_back(cam.max_x); cam_key.push_back(cam.max_y);
    // Was this frame launched already, speculatively, behind the previous one?  Then it is done or under way: take it over.
    bool adopted = false;
    if (spec_.valid) {
        if (spec_.row == current_row && spec_.first == win.first && spec_.total == win.total && spec_.seed == cfg.seed && spec_.flags == cfg.flags && spec_.cam_key == cam_key && !timed) {
            adopted = true; spec_.valid = false; ++spec_adopted_;
            std::swap(d_counters_, d_counters_spec_); std::swap(h_counters_, h_counters_spec_); std::swap(ev_call_done_, ev_spec_done_);
            launches_ = 1;
        } else if (!settle_speculation()) return 0;
    }
    if (!adopted) {
        if (hipMemsetAsync(d_counters_.get(), 0, sizeof(DCounters) * kShards, stream_) != hipSuccess) { last_error = "hipMemsetAsync failed"; return 0; }
        for (uint32_t done = 0; done < win.total; done += nown) {
            const uint32_t n = std::min(nown, win.total - done);
            if (timed) {
                while (ev_used_ + 2 > ev_pool_.size()) { hipEvent_t ev; if (hipEventCreate(&ev) != hipSuccess) { last_error = "hipEventCreate failed"; return 0; } ev_pool_.push_back(ev); }
                (void)hipEventRecord(ev_pool_[ev_used_], stream_);
                ev_secondary_.resize(ev_pool_.size() / 2); ev_secondary_[ev_used_ / 2] = false;
            }
            if (!launch_fused_window((win.first + done) % nown, n, cam, d_counters_.get())) return 0;
            if (timed) { (void)hipEventRecord(ev_pool_[ev_used_ + 1], stream_); ev_used_ += 2; }
            ++launches_;
        }
        if (!queue_counts_copy()) return 0;
        if (ev_call_done_ && hipEventRecord(ev_call_done_, stream_) != hipSuccess) { last_error = "hipEventRecord failed"; return 0; }
    }
    call_done_valid_ = ev_call_done_ != nullptr;
    current_row = win.next_row;
    mark_dirty_window(win.first, win.total);
    counts_pending_ = true; pending_primary_ = (uint64_t)win.total * cfg.width; pending_timed_ = false;
    // The next frame, speculatively (see renderer.hpp): only in the plain case — the whole image on one device (striped handles and device-group members
    // read their pixels out through paths that would give every speculation up), one launch per frame, two consecutive windows that share no row,
    // no instrumentation.
    const bool no_spec = getenv("MI355RT_NO_SPECULATE") != nullptr;
    const FrameWindow nxt = frame_window(current_row, cfg.height, cfg.stripe_rows, cfg.stripe_world, cfg.stripe_rank, owned_rows);
    if (!no_spec && !timed && cfg.stripe_world <= 1 && ev_call_done_ && read_stream_ && win.total <= nown && nxt.total != 0 && win.total + nxt.total <= nown) {
        const size_t bk = (size_t)50 * cfg.width;
        if (!d_bk_sum_) {          // all of them or none: the next call takes a non-null d_bk_sum_ for the whole set (a handle with a direct film: its backup plane too)
            DeviceBuffer<float> sum, sumsq, direct; DeviceBuffer<uint32_t> n; DeviceBuffer<DCounters> dc; PinnedBuffer<DCounters> hc;
            if (sum.alloc(bk * 12, &hbm_bytes_) != hipSuccess || sumsq.alloc(bk * 12, &hbm_bytes_) != hipSuccess || n.alloc(bk * 4, &hbm_bytes_) != hipSuccess
                || (d_film_direct_ && direct.alloc(bk * 12, &hbm_bytes_) != hipSuccess)
                || dc.alloc(sizeof(DCounters) * kShards, &hbm_bytes_) != hipSuccess || hc.alloc(sizeof(DCounters) * kShards) != hipSuccess) {
                (void)hipGetLastError(); return 50u * cfg.width;            // no room to speculate: the frame asked for is queued all the same
            }
            d_bk_sum_ = std::move(sum); d_bk_sumsq_ = std::move(sumsq); d_bk_n_ = std::move(n); d_bk_direct_ = std::move(direct); d_counters_spec_ = std::move(dc); h_counters_spec_ = std::move(hc);
        }
        const bool backed_up = launch_film_rows_copy(stream_, d_owned_rows_.get(), nxt.first, nxt.total, nown, cfg.width, d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_film_direct_.get(), d_bk_sum_.get(), d_bk_sumsq_.get(), d_bk_n_.get(), d_bk_direct_.get(), false) == hipSuccess;
        bool ok = backed_up
                  && hipMemsetAsync(d_counters_spec_.get(), 0, sizeof(DCounters) * kShards, stream_) == hipSuccess
                  && launch_fused_window(nxt.first, nxt.total, cam, d_counters_spec_.get())
                  && hipMemcpyAsync(h_counters_spec_.get(), d_counters_spec_.get(), sizeof(DCounters) * kShards, hipMemcpyDeviceToHost, stream_) == hipSuccess
                  && hipEventRecord(ev_spec_done_, stream_) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); HIP_TRY(hipStreamSynchronize(stream_));        // what was queued of it ran; put the rows back (if they were saved) and go on without
                   if (backed_up) (void)launch_film_rows_copy(stream_, d_owned_rows_.get(), nxt.first, nxt.total, nown, cfg.width, d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_film_direct_.get(), d_bk_sum_.get(), d_bk_sumsq_.get(), d_bk_n_.get(), d_bk_direct_.get(), true); }
        else { spec_.valid = true; spec_.row = current_row; spec_.first = nxt.first; spec_.total = nxt.total; spec_.next_row = nxt.next_row; spec_.cam_key = cam_key; spec_.seed = cfg.seed; spec_.flags = cfg.flags; ++spec_launched_; }
    }
    return 50u * cfg.width;
}

// one launch of the fused kernel over `total` rows of the owned-row list from entry `first` (cyclic), 1 sample per pixel
bool Renderer::launch_fused_window(uint32_t first, uint32_t total, const DCamera& cam, DCounters* dcounters)
{
    const uint32_t nown = (uint32_t)owned_rows.size();
    Slice& sl = slices_[0];
    const size_t nsamples = (size_t)total * cfg.width;
    if (!ensure_pass_capacity(sl, nsamples)) return false;
    DPass ps;
    uint32_t fchunk = 32u;                                            // samples per wave (a 4x8 pixel tile): 64 / 32 / 16 measure 0.303 / 0.266 / 0.277 ms per launch
    if (const char* e = getenv("MI355RT_FUSED_CHUNK")) { int v = atoi(e); if (v == 16 || v == 32 || v == 64) fchunk = (uint32_t)v; }   // <= 64: the LDS lists hold one row per record of a sample; >= kMinChunk: the counts arrays
    PassRequest rq;
    rq.d_rows = d_owned_rows_.get(); rq.row0 = first; rq.nrows = total; rq.row_wrap = nown;
    describe_pass(ps, sl, rq, (uint32_t)nsamples, nsamples, fchunk);
    if (ps.nchunks > sl.count_entries || (size_t)ps.nchunks * ps.region > sl.queue_records) { last_error = "internal: fused pass does not fit the pass buffers"; return false; }
    hipError_t e = launch_fused_pass(stream_, num_cus_, mode_ == kModeConfirm, dscene_, cam, ps, max_level_nodes_, records_per_sample_, sl.d_queue[0].get(), sl.d_queue[1].get(),
                                     sl.d_hits.get(), sl.d_slot_L.get(), sl.d_sample_slot.get(), d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_film_direct_.get(), dcounters);
    if (e != hipSuccess) return fail(e, "fused pass launch");
    return true;
}

// A speculative 50-row frame is out and the caller did something else: its rows go back to what they were (stream-ordered behind it).
bool Renderer::settle_speculation()
{
    if (!spec_.valid) return true;
    spec_.valid = false;
    if (!bind()) return false;
    HIP_TRY(launch_film_rows_copy(stream_, d_owned_rows_.get(), spec_.first, spec_.total, (uint32_t)owned_rows.size(), cfg.width, d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_film_direct_.get(), d_bk_sum_.get(), d_bk_sumsq_.get(), d_bk_n_.get(), d_bk_direct_.get(), true));
    return true;
}

bool Renderer::render(uint32_t spp, bool wait)
{
    if (!begin_call()) return false;
    // a lens: the same passes, their primary round fed by the lens instantiations of the kernels — no buffer, nothing to stage, so it queues like any frame
    RayFeed f{};
    f.mode = kRaysOfLens;
    if (!enqueue_frame(spp, ev_begin_, nullptr, has_lens() ? &f : nullptr)) return false;
    for (uint32_t r : owned_rows) ldr_dirty_[r] = 1;
    return end_call((uint64_t)owned_rows.size() * cfg.width * spp, wait);
}

// Samples per pass, of a frame's slice as of a ray call: 144 Mi — the whole 1080p x 64 spp frame in ONE pass (55 GB of pass buffers).  Every pass costs
// its launches' ramps and tails: 3 passes of 44 M samples 22.9 ms, 2 passes 22.2-22.6 ms, 1 pass 21.6 ms (profiles/r03_notes.md,
// with the HBM each takes: 18.9 / 27.4 / 54.5 GB); MI355RT_PASS_SAMPLES (>= 1024) or config.samples_per_pass trade the memory back.
size_t Renderer::pass_sample_budget() const
{
    if (const char* e = getenv("MI355RT_PASS_SAMPLES")) { const long v = atol(e); if (v >= 1024) return (size_t)v; }
    return (size_t)144 << 20;
}

// The passes of mi355rt_trace_rays and mi355rt_gather, `per` rays each on slice sl: halved while the device cannot hold their buffers, down to 1024
bool Renderer::fit_ray_pass(Slice& sl, size_t& per)
{
    while (!ensure_pass_capacity(sl, per)) {
        if (!alloc_failed_ || per <= 1024) return false;
        (void)hipGetLastError();
        per /= 2;
    }
    return true;
}

// The body of a frame: plan the passes of every slice (halving them while the device cannot hold their buffers) and queue them, each slice on its
// own stream, forked behind `fork` on the main stream.  render() runs one; render_adaptive() one per round, with the round's tile mask.
bool Renderer::enqueue_frame(uint32_t spp, hipEvent_t fork, const uint8_t* tile_active, const RayFeed* feed)
{
    const uint32_t nrows = (uint32_t)owned_rows.size();
    if (nrows && spp) {
        // concurrent frame slices: worth their extra launches from ~32 Mi samples per slice on (measured on one rank's share of a
        // strong-scaled 1080p x 64 frame, tools/strong_slices_probe.py: 17 / 35 / 71 / 133 M samples are fastest with 1 / 1-2 / 2 / 2-3 slices)
        uint32_t nsl = std::max(1u, std::min(slices, kMaxSlices));
        if (!slices_explicit) nsl = (uint32_t)std::min<uint64_t>(nsl, std::max<uint64_t>(1, (uint64_t)nrows * cfg.width * spp >> 25));
        nsl = std::min(nsl, (nrows + cfg.stripe_rows - 1) / cfg.stripe_rows);
        if (!assign_slice_rows(nsl)) return false;
        size_t target = pass_sample_budget();                          // per slice; config.samples_per_pass, when set, decides instead (starget below)
        // The pass buffers (two ray queues, hit records, light terms: ~410 B per sample) are sized for the
        // largest pass.  If the device cannot hold them (another tenant, a 16 GB part), halve the pass and
        // try again; results do not depend on how samples are batched into passes.
        struct PassDesc { uint32_t r0, nr, kk, s0; };          // s0: the call's sample number of the pass's first sample
        std::vector<PassDesc> plan[kMaxSlices];
        for (;;) {
            bool ok = true;
            for (uint32_t s = 0; s < nsl && ok; ++s) {
                Slice& sl = slices_[s];
                plan[s].clear();
                const uint32_t snrows = (uint32_t)sl.rows.size();
                if (!snrows) continue;
                const size_t starget = cfg.samples_per_pass ? (size_t)cfg.samples_per_pass * cfg.width * snrows : target;
                const uint32_t rows_per_pass = (uint32_t)std::min<size_t>(snrows, std::max<size_t>(1, starget / cfg.width));
                uint32_t k = (uint32_t)std::max<size_t>(1, std::min<size_t>(spp, starget / ((size_t)rows_per_pass * cfg.width)));
                if (cfg.samples_per_pass) k = std::min(spp, cfg.samples_per_pass);
                else {
                    const uint32_t np = (spp + k - 1) / k; k = (spp + np - 1) / np;      // equal passes: 48+16 -> 32+32
                    // ... of a multiple of 8 samples per pixel when there is room for it: 8 samples of a pixel sit together in the pass order (describe_pass), and the
                    // tile bins of the primary rays and the cached culling verdicts need that group to divide the 64 samples of a wave (C5: 256 spp in passes of 18 had neither)
                    if (k > 8u && k % 8u) { const uint32_t k8 = k / 8u * 8u; if ((size_t)rows_per_pass * cfg.width * (k8 + 8u) <= starget) k = k8 + 8u; else k = k8; }
                }
                ok = ensure_pass_capacity(sl, (size_t)rows_per_pass * cfg.width * std::min(k, spp));
                for (uint32_t done = 0; ok && done < spp; done += k)
                    for (uint32_t r0 = 0; r0 < snrows; r0 += rows_per_pass)
                        plan[s].push_back(PassDesc{ r0, std::min(rows_per_pass, snrows - r0), std::min(k, spp - done), done });
            }
            if (ok) break;
            if (!alloc_failed_ || cfg.samples_per_pass || target <= ((size_t)64 << 10)) return false;
            (void)hipGetLastError();
            target /= 2;
        }
        // fork: the other slices start after everything already queued on the main stream
        for (uint32_t s = 1; s < nsl; ++s) HIP_TRY(hipStreamWaitEvent(slices_[s].stream, fork, 0));
        active_slices_ = nsl;
        // Enqueue the passes round-robin so that no stream waits for the host: every slice's whole pass on its own stream.
        // Measured alternative (profiles/r02_notes.md): all trace launches on ONE stream, round by round, so that a slice's
        // confirm / shade / resolve launches (memory latency) run beside the NEXT slice's trace (VALU issue).  The schedule
        // comes out as planned, but a trace kernel with a streaming kernel beside it runs 20-25 % longer and the frame loses
        // 2 ms against the slices left to themselves (which fall into lockstep: 3 traces, then 3 shades).
        for (size_t p = 0;; ++p) {
            bool any = false;
            for (uint32_t s = 0; s < nsl; ++s) {
                if (p >= plan[s].size()) continue;
                any = true;
                const PassDesc& d = plan[s][p];
                RayFeed f{};
                if (feed) { f = *feed; f.base = d.s0; }
                PassRequest rq;
                rq.d_rows = slices_[s].d_rows.get(); rq.row0 = d.r0; rq.nrows = d.nr; rq.spp = d.kk; rq.tile_active = tile_active; rq.feed = feed ? &f : nullptr;
                if (!run_pass(slices_[s], rq)) return false;
            }
            if (!any) break;
        }
    }
    return true;
}

// ---- adaptive sampling (include/mi355rt.h) ----------------------------------------------------------------------------
// The verdict of the current film into d_tile_active_; tiles = active tiles, pixels = owned pixels in them.  The one host wait of a round: 8 bytes.
bool Renderer::adaptive_verdict(const mi355rt_adaptive_config& ac, uint32_t& tiles, uint64_t& pixels)
{
    const size_t ntiles = (size_t)tiles_x() * tiles_y();
    if (!d_tile_active_) HIP_TRY(d_tile_active_.alloc(ntiles, &hbm_bytes_));
    if (!d_tile_count_) HIP_TRY(d_tile_count_.alloc(sizeof(unsigned long long), &hbm_bytes_));
    AdaptiveArgs a{};
    a.width = cfg.width; a.height = cfg.height; a.tiles_x = tiles_x(); a.tiles_y = tiles_y();
    a.stripe_rows = cfg.stripe_rows; a.stripe_world = std::max(1u, cfg.stripe_world); a.stripe_rank = cfg.stripe_world > 1 ? cfg.stripe_rank : 0u;
    a.min_spp = ac.min_spp; a.max_spp = ac.max_spp; a.batch_spp = ac.batch_spp; a.rel_error = ac.rel_error; a.abs_floor = ac.abs_floor;
    HIP_TRY(hipMemsetAsync(d_tile_count_.get(), 0, sizeof(unsigned long long), stream_));
    HIP_TRY(launch_adaptive_tiles(stream_, a, d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_tile_active_.get(), d_tile_count_.get()));
    unsigned long long c = 0;
    HIP_TRY(hipMemcpyAsync(&c, d_tile_count_.get(), sizeof c, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    tiles = (uint32_t)(c & 0xFFFFFFFFull); pixels = c >> 32;
    return true;
}

bool Renderer::adaptive_tile_mask(const mi355rt_adaptive_config& ac, uint8_t* out, uint32_t& active)
{
    if (!quiet()) return false;
    uint64_t pixels = 0;
    if (!adaptive_verdict(ac, active, pixels)) return false;
    HIP_TRY(hipMemcpy(out, d_tile_active_.get(), (size_t)tiles_x() * tiles_y(), hipMemcpyDeviceToHost));
    return true;
}

bool Renderer::render_adaptive(const mi355rt_adaptive_config& ac, mi355rt_adaptive_stats& st)
{
    st = mi355rt_adaptive_stats{};
    std::vector<uint8_t> tile_row(tiles_y(), 0);                       // tiles with an owned pixel: whole tile rows
    for (uint32_t r : owned_rows) tile_row[r / kAdaptiveTile] = 1;
    for (uint8_t t : tile_row) st.tiles += t ? tiles_x() : 0u;
    if (!begin_call()) return false;
    uint64_t added = 0;
    for (;;) {
        uint32_t active = 0; uint64_t pixels = 0;
        if (!adaptive_verdict(ac, active, pixels)) return false;
        if (st.rounds == 0) st.tiles_active_first = active;
        st.tiles_active_last = active;
        if (active == 0 || (ac.max_rounds && st.rounds >= ac.max_rounds)) break;
        // the round's passes fork behind its verdict (slice 0 runs on the main stream; its `done` event is free here)
        HIP_TRY(hipEventRecord(slices_[0].done, stream_));
        if (!enqueue_frame(ac.batch_spp, slices_[0].done, d_tile_active_.get())) return false;
        if (!join_slices()) return false;                             // the next verdict reads what every slice wrote
        ++st.rounds;
        added += pixels * ac.batch_spp;
    }
    st.samples_added = added;
    for (uint32_t r : owned_rows) ldr_dirty_[r] = 1;
    return end_call(added, true);
}

// mi355rt_render_tiles (include/mi355rt.h): one round of the adaptive sampler with the caller's verdict — and, under a lens, with lens passes.  The passes are
// laid out over ALL owned rows as for any frame (the mask only empties chunks); the sample count comes from the mask on the host.
bool Renderer::render_tiles(const uint8_t* mask, uint32_t spp, bool device)
{
    if (!bind()) return false;
    const uint32_t tx = tiles_x(), ty = tiles_y();
    const size_t ntiles = (size_t)tx * ty;
    std::vector<uint8_t> host;
    const uint8_t* hm = mask;
    if (device) { host.resize(ntiles); HIP_TRY(hipMemcpy(host.data(), mask, ntiles, hipMemcpyDeviceToHost)); hm = host.data(); }
    // owned pixels in selected tiles, and the rows they lie in
    std::vector<uint32_t> row_pixels(ty, 0);
    for (uint32_t t = 0; t < ty; ++t)
        for (uint32_t x = 0; x < tx; ++x)
            if (hm[(size_t)t * tx + x]) row_pixels[t] += std::min(kAdaptiveTile, cfg.width - x * kAdaptiveTile);
    uint64_t pixels = 0;
    for (uint32_t r : owned_rows) pixels += row_pixels[r / kAdaptiveTile];
    const uint8_t* d_mask = mask;
    if (!device && pixels) {
        // the device copy goes ahead of begin_call's fork event on the main stream: every slice's launches are ordered behind it
        if (!d_tile_active_) HIP_TRY(d_tile_active_.alloc(ntiles, &hbm_bytes_));
        HIP_TRY(hipMemcpyAsync(d_tile_active_.get(), mask, ntiles, hipMemcpyHostToDevice, stream_));
        d_mask = d_tile_active_.get();
    }
    if (!begin_call()) return false;
    if (pixels) {
        RayFeed f{};
        f.mode = kRaysOfLens;
        if (!enqueue_frame(spp, ev_begin_, d_mask, has_lens() ? &f : nullptr)) return false;
        for (uint32_t r : owned_rows) if (row_pixels[r / kAdaptiveTile]) ldr_dirty_[r] = 1;
    }
    return end_call(pixels * spp, true);
}

// get_tonemapped_pixels, mod.rs:120-128.  The reference maps the whole film on every call although one
// trace_frame_additive changes 50 rows; here only the rows written since the last read-out are mapped again and
// copied (into a pinned host mirror of the frame), then the caller gets its own copy of the whole frame.
bool Renderer::get_tonemapped(uint32_t* out, size_t n)
{
    if (!bind()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (n < npix || !out) { last_error = "output buffer too small"; return false; }
    if (!h_ldr_) HIP_TRY(h_ldr_.alloc(npix * 4));
    // A speculative frame may be changing rows right now (trace_frame_additive).  Rows it touches that have to be read (everything is dirty after a
    // clear) would show samples the caller has not asked for yet: then the speculation is given up.  Otherwise the read-out runs beside it, on its own
    // stream, behind the frame the caller did ask for.
    if (spec_.valid) {
        bool clash = false;
        const uint32_t nown = (uint32_t)owned_rows.size();
        for (uint32_t i = 0; i < spec_.total && !clash; ++i) clash = ldr_dirty_[owned_rows[(spec_.first + i) % nown]] != 0;
        if (clash && !settle_speculation()) return false;
    }
    hipStream_t rs = stream_;
    if (spec_.valid && call_done_valid_ && read_stream_) { HIP_TRY(hipStreamWaitEvent(read_stream_, ev_call_done_, 0)); rs = read_stream_; }
    for (uint32_t r = 0; r < cfg.height;) {
        if (!ldr_dirty_[r]) { ++r; continue; }
        uint32_t e = r;
        while (e < cfg.height && ldr_dirty_[e]) ldr_dirty_[e++] = 0;
        HIP_TRY(launch_tonemap(rs, nullptr, r, e - r, cfg.width, false, d_film_sum_.get(), d_film_n_.get(), d_ldr_.get()));
        HIP_TRY(hipMemcpyAsync(h_ldr_.get() + (size_t)r * cfg.width, d_ldr_.get() + (size_t)r * cfg.width, (size_t)(e - r) * cfg.width * 4, hipMemcpyDeviceToHost, rs));
        r = e;
    }
    HIP_TRY(hipStreamSynchronize(rs));
    std::memcpy(out, h_ldr_.get(), npix * 4);
    return true;
}

// Owned rows, packed, into caller-owned DEVICE memory.  caller_stream == null: runs on the handle's stream and
// returns when done.  Otherwise the kernel is launched on the caller's stream (after everything this handle has
// queued) and the call returns at once: the write is ordered with whatever the caller does on that stream
// before and after (its collective, its buffer initialisation).
bool Renderer::tonemap_owned_rows_device(uint32_t* device_out, size_t n, hipStream_t caller_stream)
{
    if (!quiet()) return false;
    if (n < owned_rows.size() * (size_t)cfg.width || !device_out) { last_error = "output buffer too small"; return false; }
    if (caller_stream) {
        HIP_TRY(hipEventRecord(slices_[0].done, stream_));
        HIP_TRY(hipStreamWaitEvent(caller_stream, slices_[0].done, 0));
        HIP_TRY(launch_tonemap(caller_stream, d_owned_rows_.get(), 0, (uint32_t)owned_rows.size(), cfg.width, true, d_film_sum_.get(), d_film_n_.get(), device_out));
        // later work of this handle (film.clear, the next frame) must not overtake the read of the film
        HIP_TRY(hipEventRecord(ev_tonemap_, caller_stream));
        HIP_TRY(hipStreamWaitEvent(stream_, ev_tonemap_, 0));
        return true;
    }
    HIP_TRY(launch_tonemap(stream_, d_owned_rows_.get(), 0, (uint32_t)owned_rows.size(), cfg.width, true, d_film_sum_.get(), d_film_n_.get(), device_out));
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

bool Renderer::synchronize()
{
    if (!bind()) return false;
    for (Slice& o : slices_) if (o.stream) HIP_TRY(hipStreamSynchronize(o.stream));
    if (read_stream_) HIP_TRY(hipStreamSynchronize(read_stream_));
    return true;
}

// MI355RT_DEBUG_GUARD builds of the pass buffers: number of guard bytes that no longer hold the fill pattern (-1: error)
long Renderer::check_guards()
{
    if (!bind()) return -1;
    long bad = 0;
    std::vector<uint8_t> h(kGuardBytes);
    for (Slice& sl : slices_) {
        if (sl.stream && hipStreamSynchronize(sl.stream) != hipSuccess) return -1;
        sl.for_each_pass_buffer([&](const auto& buf) {
            if (bad < 0 || !buf.guard()) return;
            if (hipMemcpy(h.data(), buf.guard(), kGuardBytes, hipMemcpyDeviceToHost) != hipSuccess) bad = -1;
            else for (uint8_t b : h) bad += b != 0xA5;
        });
    }
    return bad;
}

// ---- multi-GPU gather ------------------------------------------------------------------------------------------
uint32_t Renderer::slot_rows() const
{
    const uint32_t stripes = (cfg.height + cfg.stripe_rows - 1) / cfg.stripe_rows;
    return ((stripes + cfg.stripe_world - 1) / cfg.stripe_world) * cfg.stripe_rows;
}
uint32_t Renderer::rows_of_rank(uint32_t rank) const
{
    uint32_t n = 0;
    for (uint32_t s = rank; (uint64_t)s * cfg.stripe_rows < cfg.height; s += cfg.stripe_world) n += std::min(cfg.stripe_rows, cfg.height - s * cfg.stripe_rows);
    return n;
}
bool Renderer::gather_prepare(bool root)
{
    if (!bind()) return false;
    if (d_gather_ && gather_is_root_ == root) return true;
    if (d_gather_) HIP_TRY(hipStreamSynchronize(stream_));             // kernels of earlier calls may still use the old slots
    const size_t slot = (size_t)slot_rows() * cfg.width * 4;
    HIP_TRY(d_gather_.alloc(slot * (root ? cfg.stripe_world : 1), &hbm_bytes_));
    gather_is_root_ = root;
    return true;
}
bool Renderer::tonemap_to_gather_slot()
{
    if (!quiet()) return false;
    HIP_TRY(launch_tonemap(stream_, d_owned_rows_.get(), 0, (uint32_t)owned_rows.size(), cfg.width, true, d_film_sum_.get(), d_film_n_.get(), gather_slot(cfg.stripe_rank)));
    return true;
}
bool Renderer::finish_gather(uint32_t* host_out, size_t n)
{
    if (!bind()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (host_out && n < npix) { last_error = "output buffer too small"; return false; }
    HIP_TRY(launch_place_stripes(stream_, d_gather_.get(), d_ldr_.get(), cfg.width, cfg.height, cfg.stripe_rows, cfg.stripe_world, slot_rows()));
    if (host_out) {
        if (!h_ldr_) HIP_TRY(h_ldr_.alloc(npix * 4));
        HIP_TRY(hipMemcpyAsync(h_ldr_.get(), d_ldr_.get(), npix * 4, hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        std::memcpy(host_out, h_ldr_.get(), npix * 4);
    }
    return true;
}

bool Renderer::film_get(float* sum, float* sumsq, uint32_t* n)
{
    if (!quiet()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    HIP_TRY(hipStreamSynchronize(stream_));
    if (sum) HIP_TRY(hipMemcpy(sum, d_film_sum_.get(), npix * 12, hipMemcpyDeviceToHost));
    if (sumsq) HIP_TRY(hipMemcpy(sumsq, d_film_sumsq_.get(), npix * 12, hipMemcpyDeviceToHost));
    if (n) HIP_TRY(hipMemcpy(n, d_film_n_.get(), npix * 4, hipMemcpyDeviceToHost));
    return true;
}

// mi355rt_film_get_direct: the caller has checked the flag
bool Renderer::film_get_direct(float* sum)
{
    if (!bind()) return false;
    if (!d_film_direct_) { last_error = "internal: no direct film"; return false; }
    if (!settle_speculation()) return false;
    HIP_TRY(hipStreamSynchronize(stream_));
    HIP_TRY(hipMemcpy(sum, d_film_direct_.get(), (size_t)cfg.width * cfg.height * 12, hipMemcpyDeviceToHost));
    return true;
}

bool Renderer::film_clear()
{
    if (!quiet()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    std::fill(ldr_dirty_.begin(), ldr_dirty_.end(), (uint8_t)1);     // unsampled rows read back white (NaN -> 255)
    caller_ray_film_ = false;
    if (cfg.stripe_world > 1) {
        // a striped handle only ever writes its own rows (the others stay as created: zero): one launch over them instead of three
        // whole-film memsets — 20 us of a 3.3 ms frame on one rank of eight
        HIP_TRY(launch_film_clear_rows(stream_, d_owned_rows_.get(), (uint32_t)owned_rows.size(), cfg.width, d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_film_direct_.get()));
        if (d_film_lights_) HIP_TRY(launch_light_films_clear_rows(stream_, d_owned_rows_.get(), (uint32_t)owned_rows.size(), cfg.width, nlights_, d_film_lights_.get(), lights_stride()));
        return true;
    }
    HIP_TRY(hipMemsetAsync(d_film_sum_.get(), 0, npix * 12, stream_));
    HIP_TRY(hipMemsetAsync(d_film_sumsq_.get(), 0, npix * 12, stream_));
    HIP_TRY(hipMemsetAsync(d_film_n_.get(), 0, npix * 4, stream_));
    if (d_film_direct_) HIP_TRY(hipMemsetAsync(d_film_direct_.get(), 0, npix * 12, stream_));
    if (d_film_lights_) HIP_TRY(launch_light_films_clear_rows(stream_, d_owned_rows_.get(), (uint32_t)owned_rows.size(), cfg.width, nlights_, d_film_lights_.get(), lights_stride()));
    return true;            // stream-ordered: every later call on this handle starts on the same stream
}

// mi355rt_film_set / mi355rt_film_add: the caller's planes are staged (staging.hpp; n, sum, sumsq, direct: the order of a film file), the merge kernel
// stores or adds them on the rows this handle owns, and the staging is freed again.  Everything runs on stream_: behind a
// queued frame (render_async joins its slices there) and behind the rows a speculative frame gives back, ahead of every later call.  Nothing but
// the film and the tone-map cache's dirty rows changes.
bool Renderer::film_put(const FilmPlanes& in, bool add)
{
    if (!bind()) return false;
    if (!in.sum || !in.sumsq || !in.n || (in.direct != nullptr) != (bool)d_film_direct_) { last_error = "internal: film_put planes do not match the film"; return false; }
    if (!settle_speculation()) return false;
    if (!add) caller_ray_film_ = false;                               // the film is the caller's planes now
    const size_t npix = (size_t)cfg.width * cfg.height;
    Staging st(stream_, &hbm_bytes_, false);
    const uint32_t* s_n = st.in(in.n, npix);
    const float* s_sum = st.in(in.sum, npix * 3);
    const float* s_sumsq = st.in(in.sumsq, npix * 3);
    const float* s_direct = st.in(in.direct, npix * 3);
    HIP_TRY(st.error());
    HIP_TRY(launch_film_merge(stream_, add, s_sum, s_sumsq, s_n, s_direct, (uint32_t)npix, cfg.width, cfg.stripe_rows, cfg.stripe_world, cfg.stripe_rank,
                              d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d_film_direct_.get()));
    std::fill(ldr_dirty_.begin(), ldr_dirty_.end(), (uint8_t)1);
    HIP_TRY(hipStreamSynchronize(stream_));                           // the caller's arrays and the staging are free again
    return true;
}

// ---- light films (include/mi355rt.h, "LIGHT FILMS") ----
static_assert(kMaxLightFilms == MI355RT_LIGHT_FILMS_MAX_LIGHTS, "the header's limit is the one resolve_kernel's LDS is sized for");
bool Renderer::light_films_get(float* planes)
{
    if (!quiet()) return false;
    HIP_TRY(hipStreamSynchronize(stream_));
    if (d_film_lights_) HIP_TRY(hipMemcpy(planes, d_film_lights_.get(), (size_t)nlights_ * lights_stride() * 4, hipMemcpyDeviceToHost));
    return true;
}

// mi355rt_light_films_set / _add: as film_put — the caller's planes staged in a temporary device buffer, stored or added on the owned rows, on stream_
bool Renderer::light_films_put(const float* planes, bool add)
{
    if (!quiet()) return false;
    if (!d_film_lights_) return true;                                 // no lights: no planes
    Staging st(stream_, &hbm_bytes_, false);
    const float* s_planes = st.in(planes, (size_t)nlights_ * lights_stride());
    HIP_TRY(st.error());
    HIP_TRY(launch_light_films_merge(stream_, add, s_planes, nlights_, cfg.width * cfg.height, cfg.width, cfg.stripe_rows, cfg.stripe_world, cfg.stripe_rank,
                                     d_film_lights_.get(), lights_stride()));
    HIP_TRY(hipStreamSynchronize(stream_));                           // the caller's array and the staging are free again
    return true;
}

bool Renderer::ensure_display_buffers(bool hist_and_table)
{
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!d_disp_packed_) HIP_TRY(d_disp_packed_.alloc(npix * 4, &hbm_bytes_));
    if (!hist_and_table) return true;
    if (!d_disp_hist_) HIP_TRY(d_disp_hist_.alloc(kDisplayHistWords * 4, &hbm_bytes_));
    if (!d_disp_table_) {
        float t[256];
        display_srgb_table(t);
        DeviceBuffer<float> tab;
        HIP_TRY(tab.alloc(sizeof t, &hbm_bytes_));
        HIP_TRY(hipMemcpy(tab.get(), t, sizeof t, hipMemcpyHostToDevice));
        d_disp_table_ = std::move(tab);
    }
    return true;
}

// mi355rt_get_relit_pixels: relit_kernel writes c into d_relit_rgb_, which the display kernels read as a non-film image (the film's n decides `empty`).
// dc == null: DISPLAY MAPPING with exposure 1, the Reinhard curve and the reference's transfer is get_tonemapped_pixels' map of c (c * 1.0f is c).
bool Renderer::get_relit(const float* weights3, const mi355rt_display_config* dc, float* rgb, uint32_t* packed, float& exposure_used)
{
    if (!quiet()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!d_relit_rgb_) {
        DeviceBuffer<float> img, w;
        HIP_TRY(img.alloc(npix * 12, &hbm_bytes_));
        HIP_TRY(w.alloc((size_t)MI355RT_LIGHT_FILMS_MAX_LIGHTS * 12, &hbm_bytes_));
        d_relit_rgb_ = std::move(img); d_relit_weights_ = std::move(w);
    }
    if (!ensure_display_buffers(dc != nullptr)) return false;
    if (nlights_) HIP_TRY(hipMemcpyAsync(d_relit_weights_.get(), weights3, (size_t)nlights_ * 12, hipMemcpyHostToDevice, stream_));
    HIP_TRY(launch_relit(stream_, (uint32_t)npix, nlights_, d_film_lights_.get(), lights_stride(), d_film_n_.get(), d_relit_weights_.get(), d_relit_rgb_.get()));
    float E = dc ? dc->exposure : 1.0f;
    if (dc && dc->auto_exposure) {
        mi355rt_luminance_histogram hist;
        if (!display_hist_queue(d_relit_rgb_.get(), false, hist)) return false;
        E = display_auto_exposure(hist, dc->key, dc->low, dc->high);
    }
    if (packed) {
        HIP_TRY(launch_display_pack(stream_, display_args(dc, E), (uint32_t)npix, d_relit_rgb_.get(), d_film_n_.get(), false, d_disp_table_.get(), d_disp_packed_.get()));
        HIP_TRY(hipMemcpyAsync(packed, d_disp_packed_.get(), npix * 4, hipMemcpyDeviceToHost, stream_));
    }
    if (rgb) HIP_TRY(hipMemcpyAsync(rgb, d_relit_rgb_.get(), npix * 12, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    exposure_used = E;
    return true;
}

bool Renderer::intersect(const float* rays6, size_t n, float* tuv, uint32_t* prim, uint8_t* blocked)
{
    if (!bind()) return false;
    if (n == 0) return true;
    if (n > 0x7FFFFFFFull / 24) { last_error = "too many rays in one batch"; return false; }
    const bool shadow = blocked != nullptr;               // then tuv and prim are null, and the kernel touches neither
    Staging st(stream_, &hbm_bytes_, false);
    const float* d_rays = st.in(rays6, n * 6);
    float* d_tuv = st.out(tuv, n * 3, true);              // misses stay untouched
    uint32_t* d_prim = st.out(prim, n);
    uint8_t* d_blocked = st.out(blocked, n);
    HIP_TRY(st.error());
    HIP_TRY(launch_intersect(stream_, dscene_, traversal_rows(), (int)mode_, d_rays, (uint32_t)n, shadow, d_tuv, d_prim, d_blocked));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// ---- caller-supplied rays (include/mi355rt.h) ---------------------------------------------------------------------------
// mi355rt_trace_rays: the rays as ray-fed passes of one sample each on slice 0 (the main stream), as many as the pass buffers need.  Host memory is staged
// (staging.hpp) in the caller's own layout: rays, keys, and whatever outputs are asked for; device memory is read and written in place.  A read-out like
// debug_sample: no film, no camera, no row state changes.
bool Renderer::trace_rays(const float* rays6, const uint32_t* keys2, size_t n, bool device, const mi355rt_ray_outputs& out)
{
    if (!begin_call()) return false;                                  // settles a speculative frame; a queued frame is ahead on the same stream
    if (n > 0xFFFFFFFFull) { last_error = "mi355rt_trace_rays: n does not fit 32 bits"; return false; }
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_rays = st.in(rays6, n * 6); const uint32_t* d_keys = st.in(keys2, n * 2);
    float* d_rgb = st.out(out.rgb, n * 3); float* d_direct = st.out(out.direct, n * 3);
    float* d_tuv = st.out(out.tuv, n * 3, true);                      // goes up first: a miss leaves it as it was
    uint32_t* d_prim = st.out(out.prim, n);
    HIP_TRY(st.error());
    // rays per pass: what the frame's passes hold (enqueue_frame), config.samples_per_pass images' worth when that is set; halved while the device cannot hold the buffers
    size_t per = cfg.samples_per_pass ? std::max<size_t>(1, (size_t)cfg.samples_per_pass * cfg.width * cfg.height) : pass_sample_budget();
    per = std::min(per, std::max<size_t>(n, 1));
    Slice& sl = slices_[0];
    if (n && !fit_ray_pass(sl, per)) return false;
    DeviceBuffer<float4> s_hit;
    if (n && (out.tuv || out.prim)) HIP_TRY(s_hit.alloc(per * sizeof(float4), &hbm_bytes_));
    for (size_t at = 0; at < n; at += per) {
        const size_t cnt = std::min(per, n - at);
        RayFeed f{};
        f.mode = kRaysFree; f.rays = d_rays + 6 * at; f.keys = d_keys ? d_keys + 2 * at : nullptr; f.base = (uint32_t)at; f.count = (uint32_t)cnt; f.hit = s_hit.get();
        f.rgb = d_rgb ? d_rgb + 3 * at : nullptr; f.direct = d_direct ? d_direct + 3 * at : nullptr; f.tuv = d_tuv ? d_tuv + 3 * at : nullptr; f.prim = d_prim ? d_prim + at : nullptr;
        PassRequest rq;
        rq.feed = &f;
        if (!run_pass(sl, rq)) return false;
    }
    HIP_TRY(st.download());
    return end_call(n, true);                                         // waits: the staging (and the caller's buffers) are free again
}

// The chunk loop mi355rt_gather and mi355rt_probes_gather share.  Rays per chunk: what a pass of trace_rays holds.  A chunk's rays, keys and validity bytes
// are made by gather_rays_kernel, the chunk runs as ONE ray-fed pass (RayFeed kRaysFree, exactly a pass of trace_rays) when `traced`, and `reduce` folds its
// results into the caller's outputs.  Everything is queued on one stream, the sample chunks of a point range in ascending sample order, so every point takes
// its samples in order.  Waits before it returns: the chunk buffers go out of scope here.
bool Renderer::gather_chunks(const float* d_points, const float* d_normals, const uint32_t* d_ids, size_t npoints, uint32_t spp, uint32_t first_sample, bool traced, bool want_rgb,
                             bool want_hits, const std::function<hipError_t(const GatherChunk&)>& reduce)
{
    const size_t total = npoints * spp;
    size_t per = cfg.samples_per_pass ? std::max<size_t>(1, (size_t)cfg.samples_per_pass * cfg.width * cfg.height) : pass_sample_budget();
    per = std::min(per, total);
    Slice& sl = slices_[0];
    if (traced && !fit_ray_pass(sl, per)) return false;
    const size_t cp_max = std::min(npoints, per), cs_max = std::max<size_t>(1, std::min<size_t>(spp, per / cp_max));
    const size_t cap = cp_max * cs_max;
    DeviceBuffer<float> c_rays, c_rgb, c_tuv; DeviceBuffer<uint32_t> c_keys, c_prim; DeviceBuffer<uint8_t> c_valid; DeviceBuffer<float4> c_hit;
    HIP_TRY(c_rays.alloc(cap * 24, &hbm_bytes_));
    HIP_TRY(c_keys.alloc(cap * 8, &hbm_bytes_));
    HIP_TRY(c_valid.alloc(cap, &hbm_bytes_));
    if (want_rgb) HIP_TRY(c_rgb.alloc(cap * 12, &hbm_bytes_));
    if (want_hits) { HIP_TRY(c_tuv.alloc(cap * 12, &hbm_bytes_)); HIP_TRY(c_prim.alloc(cap * 4, &hbm_bytes_)); HIP_TRY(c_hit.alloc(cap * sizeof(float4), &hbm_bytes_)); }
    for (size_t p0 = 0; p0 < npoints; p0 += cp_max) {
        const uint32_t cp = (uint32_t)std::min(cp_max, npoints - p0);
        for (uint32_t s0 = 0; s0 < spp; s0 += (uint32_t)cs_max) {
            const uint32_t cs = (uint32_t)std::min<size_t>(cs_max, spp - s0);
            HIP_TRY(launch_gather_rays(stream_, dscene_, (uint32_t)cfg.seed, d_points, d_normals, d_ids, (uint32_t)p0, cp, cs, first_sample + s0, c_rays.get(), c_keys.get(), c_valid.get()));
            if (traced) {
                RayFeed f{};
                f.mode = kRaysFree; f.rays = c_rays.get(); f.keys = c_keys.get(); f.base = 0u; f.count = cp * cs; f.hit = c_hit.get();
                f.rgb = c_rgb.get(); f.tuv = c_tuv.get(); f.prim = c_prim.get();
                PassRequest rq;
                rq.feed = &f;
                if (!run_pass(sl, rq)) return false;
            }
            HIP_TRY(reduce(GatherChunk{ (uint32_t)p0, cp, s0, cs, c_rays.get(), c_valid.get(), c_rgb.get(), c_tuv.get(), c_prim.get() }));
        }
    }
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// mi355rt_probes_gather: gather's sphere-mode samples (no normals: no walk, no void sample) through gather's chunk loop, with the projection
// of csrc/probes.hip as the reduce.  Around the call everything is gather's.
bool Renderer::probes_gather(const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_config& pc, bool device, const mi355rt_probe_outputs& out)
{
    if (!begin_call()) return false;
    const bool hitq = out.hits || out.near, traced = out.sh || hitq;  // n alone needs no ray
    const size_t total = npoints * pc.spp;
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_points = st.in(points3, npoints * 3); const uint32_t* d_ids = st.in(ids, npoints);
    const bool acc = pc.accumulate != 0;                              // then the outputs go up first: the call adds to what they hold
    mi355rt_probe_outputs d{};
    d.n = st.out(out.n, npoints, acc); d.hits = st.out(out.hits, npoints, acc); d.near = st.out(out.near, npoints, acc); d.sh = st.out(out.sh, npoints * 27, acc);
    HIP_TRY(st.error());
    if (!gather_chunks(d_points, nullptr, d_ids, npoints, pc.spp, pc.first_sample, traced, out.sh != nullptr, hitq, [&](const GatherChunk& c) {
            return launch_probes_project(stream_, c.point0, c.cp, c.cs, !acc && c.sample0 == 0, pc.near_distance, c.rays, c.rgb, c.tuv, c.prim, d.n, d.hits, d.near, d.sh);
        })) return false;
    HIP_TRY(st.download());
    return end_call(traced ? total : 0, true);                        // waits: the staging (and the caller's buffers) are free again
}

namespace {
// the volume's arrays on the device: the caller's own, or staged copies
LitVolume stage_volume(Staging& st, const mi355rt_probe_volume& vol)
{
    const mi355rt_probe_grid& grid = *vol.grid;
    const size_t nprobes = (size_t)grid.counts[0] * grid.counts[1] * grid.counts[2];
    LitVolume v{};
    std::memcpy(&v.grid, &grid, sizeof v.grid);
    v.n = st.in(vol.n, nprobes); v.sh = st.in(vol.sh, nprobes * 27); v.usable = st.in(vol.usable, nprobes);
    if (vol.depth) {
        const size_t RR = (size_t)vol.depth->res * vol.depth->res;
        v.R = vol.depth->res;
        v.count = st.in((const uint32_t*)vol.depth->count, nprobes * RR); v.moments = st.in((const float*)vol.depth->moments, nprobes * RR * 2);
        v.offsets = st.in(vol.offsets, nprobes * 3);
        v.flags = vol.vc->flags; v.normal_bias = vol.vc->normal_bias;
    }
    return v;
}
}  // namespace

// The read-outs of a probe grid (mi355rt_probes_lookup, _vis, _placed; mi355rt_probe_lit_points): arithmetic on the caller's arrays, one kernel.  Stages the
// grid's arrays, the queries (dirs3, normals3 may be null) and the outputs, queues what `launch` launches, downloads and waits.  A read-out makes no ray: a
// speculative frame is settled, a queued one is ahead on the same stream, and neither the counters nor any film is touched.
template <class Launch>
bool Renderer::volume_readout(const mi355rt_probe_volume& vol, const float* points3, const float* dirs3, const float* normals3, size_t npoints, bool device, float* rgb3, uint8_t* ok,
                              Launch launch)
{
    if (!quiet()) return false;
    Staging st(stream_, &hbm_bytes_, device);
    const LitVolume v = stage_volume(st, vol);
    const float* d_points = st.in(points3, npoints * 3); const float* d_dirs = st.in(dirs3, npoints * 3); const float* d_normals = st.in(normals3, npoints * 3);
    float* d_rgb = st.out(rgb3, npoints * 3); uint8_t* d_ok = st.out(ok, npoints);
    HIP_TRY(st.error());
    HIP_TRY(launch(v, d_points, d_dirs, d_normals, d_rgb, d_ok));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));                           // the caller's buffers are complete, on whatever stream they are used next
    return true;
}

// mi355rt_probes_lookup
bool Renderer::probes_lookup(const mi355rt_probe_grid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const float* points3, const float* dirs3, size_t npoints,
                             uint32_t mode, bool device, float* rgb3, uint8_t* ok)
{
    return volume_readout({ &grid, n, sh, usable, nullptr, nullptr, nullptr }, points3, dirs3, nullptr, npoints, device, rgb3, ok,
                          [&](const LitVolume& v, const float* p, const float* d, const float*, float* rgb, uint8_t* k) {
                              return launch_probes_lookup(stream_, v.grid, v.n, v.sh, v.usable, p, d, npoints, mode, rgb, k);
                          });
}

// mi355rt_probes_gather_depth: probes_gather with a second reduce over the same traced chunk — the depth film of csrc/probes_vis.hip.  The
// chunk temporary of its first phase (8 bytes per entry) is made when the first, largest chunk arrives and goes with the call, counted like every other.
bool Renderer::probes_gather_depth(const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_config& pc, bool device, const mi355rt_probe_outputs& out,
                                   const mi355rt_probe_depth& depth)
{
    if (!begin_call()) return false;
    const size_t total = npoints * pc.spp, RR = (size_t)depth.res * depth.res;
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_points = st.in(points3, npoints * 3); const uint32_t* d_ids = st.in(ids, npoints);
    const bool acc = pc.accumulate != 0;                              // then the outputs go up first: the call adds to what they hold
    mi355rt_probe_outputs d{};
    d.n = st.out(out.n, npoints, acc); d.hits = st.out(out.hits, npoints, acc); d.near = st.out(out.near, npoints, acc); d.sh = st.out(out.sh, npoints * 27, acc);
    uint32_t* d_count = st.out(depth.count, npoints * RR, acc); float* d_moments = st.out(depth.moments, npoints * RR * 2, acc);
    HIP_TRY(st.error());
    const bool project = d.n || d.hits || d.near || d.sh;
    DeviceBuffer<uint2> bins;
    if (!gather_chunks(d_points, nullptr, d_ids, npoints, pc.spp, pc.first_sample, true, out.sh != nullptr, true, [&](const GatherChunk& c) {
            const bool fresh = !acc && c.sample0 == 0;
            if (project) {
                const hipError_t e = launch_probes_project(stream_, c.point0, c.cp, c.cs, fresh, pc.near_distance, c.rays, c.rgb, c.tuv, c.prim, d.n, d.hits, d.near, d.sh);
                if (e != hipSuccess) return e;
            }
            const size_t need = (size_t)c.cp * c.cs * sizeof(uint2);
            if (bins.bytes() < need) {
                const hipError_t e = bins.alloc(need, &hbm_bytes_);
                if (e != hipSuccess) return e;
            }
            return launch_probes_depth(stream_, c.point0, c.cp, c.cs, fresh, depth.res, depth.max_distance, c.rays, c.tuv, c.prim, bins.get(), d_count, d_moments);
        })) return false;
    HIP_TRY(st.download());
    return end_call(total, true);                                     // waits: the staging (and the caller's buffers) are free again
}

// mi355rt_probes_lookup_vis: the depth films among the volume's arrays
bool Renderer::probes_lookup_vis(const mi355rt_probe_grid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth& depth,
                                 const mi355rt_probe_vis_config& vc, const float* points3, const float* dirs3, const float* normals3, size_t npoints, uint32_t mode, bool device,
                                 float* rgb3, uint8_t* ok)
{
    return volume_readout({ &grid, n, sh, usable, &depth, &vc, nullptr }, points3, dirs3, normals3, npoints, device, rgb3, ok,
                          [&](const LitVolume& v, const float* p, const float* d, const float* nr, float* rgb, uint8_t* k) {
                              return launch_probes_lookup_vis(stream_, v.grid, v.n, v.sh, v.usable, v.R, v.count, v.moments, v.flags, v.normal_bias, p, d, nr, npoints, mode, rgb, k);
                          });
}

// mi355rt_gather: the points as a film of their own.  Chunks of cp points x cs samples, sized by the pass capacity as trace_rays sizes its
// passes: gather_rays_kernel makes the chunk's rays, keys and validity bytes, the chunk runs as ONE ray-fed pass (RayFeed kRaysFree, exactly a pass of trace_rays),
// gather_reduce_kernel folds its results into the points' outputs.  The sample chunks of a point range go in ascending sample order, on one stream, so every
// point takes its samples in order.  `direct` is a launch_intersect in shadow mode between two kernels of its own.  Host memory is staged (the outputs go up
// first when the call accumulates); every temporary is freed on return.
bool Renderer::gather(const float* points3, const float* normals3, const uint32_t* ids, size_t npoints, const mi355rt_gather_config& gc, bool device, const mi355rt_gather_outputs& out)
{
    if (!begin_call()) return false;                                  // settles a speculative frame; a queued frame is ahead on the same stream
    const bool sums = out.sum || out.sumsq, hitq = out.hits || out.near;
    const bool sampled = sums || hitq || out.n, traced = sums || hitq;           // n alone needs the walk, not the rays' radiance
    const size_t total = sampled ? npoints * gc.spp : 0;
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_points = st.in(points3, npoints * 3); const float* d_normals = st.in(normals3, npoints * 3); const uint32_t* d_ids = st.in(ids, npoints);
    const bool acc = gc.accumulate != 0;                              // then the sampled outputs go up first: the call adds to what they hold
    mi355rt_gather_outputs d{};
    d.n = st.out(out.n, npoints, acc); d.hits = st.out(out.hits, npoints, acc); d.near = st.out(out.near, npoints, acc);
    d.sum = st.out(out.sum, npoints * 3, acc); d.sumsq = st.out(out.sumsq, npoints * 3, acc); d.direct = st.out(out.direct, npoints * 3);
    HIP_TRY(st.error());
    if (d.direct) {
        // (light, point) shadow rays in chunks of at most 4 M rays
        const size_t cpd = std::min(npoints, std::max<size_t>(1, ((size_t)4 << 20) / std::max(nlights_, 1u)));
        DeviceBuffer<float> c_rays; DeviceBuffer<uint8_t> c_blocked;
        if (nlights_) { HIP_TRY(c_rays.alloc(cpd * nlights_ * 24, &hbm_bytes_)); HIP_TRY(c_blocked.alloc(cpd * nlights_, &hbm_bytes_)); }
        for (size_t p0 = 0; p0 < npoints; p0 += cpd) {
            const uint32_t cp = (uint32_t)std::min(cpd, npoints - p0);
            HIP_TRY(launch_gather_shadow_rays(stream_, dscene_, d_points, (uint32_t)p0, cp, c_rays.get()));
            HIP_TRY(launch_intersect(stream_, dscene_, traversal_rows(), (int)mode_, c_rays.get(), cp * nlights_, true, nullptr, nullptr, c_blocked.get()));
            HIP_TRY(launch_gather_direct(stream_, dscene_, d_points, d_normals, (uint32_t)p0, cp, c_blocked.get(), d.direct));
        }
        HIP_TRY(hipStreamSynchronize(stream_));                       // the chunk buffers go out of scope here
    }
    if (total && !gather_chunks(d_points, d_normals, d_ids, npoints, gc.spp, gc.first_sample, traced, sums, hitq, [&](const GatherChunk& c) {
            return launch_gather_reduce(stream_, c.point0, c.cp, c.cs, gc.weight, !gc.accumulate && c.sample0 == 0, gc.near_distance, d_normals, c.rays, c.valid, c.rgb, c.tuv, c.prim,
                                        d.n, d.hits, d.near, d.sum, d.sumsq);
        })) return false;
    if (!total) { st.only(out.n, 0); st.only(out.hits, 0); st.only(out.near, 0); st.only(out.sum, 0); st.only(out.sumsq, 0); }     // spp == 0: nothing was sampled, nothing to copy
    HIP_TRY(st.download());
    return end_call(traced ? total : 0, true);                        // waits: the staging (and the caller's buffers) are free again
}

// mi355rt_bake_texels: csrc/bake.hip does the work on device memory; this stages host memory around it.  A read-out that makes no ray: a
// speculative frame is settled, a queued one is ahead on the same stream, and neither the counters nor any film is touched.  The points need B - A and C - A
// with the bits of the f32 subtraction: the leaf-order triangles hold exactly those (bvh.hpp), so the first call that asks for points puts them into scene
// order once (d_bake_tris_, 36 bytes per triangle, counted in hbm_allocated_bytes and kept for the handle's life).
bool Renderer::bake_texels(const float* uv, uint32_t width, uint32_t height, bool flip, bool device, const mi355rt_bake_texel_outputs& out, uint32_t* ncovered)
{
    if (!quiet()) return false;
    const size_t nt = (size_t)width * height;
    if (out.points && !d_bake_tris_ && ntri) {
        std::vector<float> t9((size_t)ntri * 9);
        for (const BvhTri& t : bvh.tris) {
            if (t.prim >= ntri) continue;
            float* q = &t9[9 * (size_t)t.prim];
            for (int a = 0; a < 3; ++a) { q[a] = t.v0[a]; q[3 + a] = t.e1[a]; q[6 + a] = t.e2[a]; }
        }
        if (!upload(d_bake_tris_, t9.data(), t9.size() * sizeof(float))) return false;
    }
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_uv = st.in(uv, (size_t)ntri * 6, true);            // ntri == 0: the callee still takes a pointer
    mi355rt_bake_texel_outputs d{};
    d.owner = st.scratch(out.owner, nt);                              // the rasteriser writes owner and bary whether or not the caller asked
    d.bary = st.scratch(out.bary, nt * 2, true);                      // uncovered texels keep what the caller had
    d.ids = st.out(out.ids, nt); d.points = st.out(out.points, nt * 3); d.normals = st.out(out.normals, nt * 3); d.albedo = st.out(out.albedo, nt * 3);
    HIP_TRY(st.error());
    uint32_t n = 0;
    HIP_TRY(bake_texels_device(stream_, dscene_, d_bake_tris_.get(), d_uv, ntri, width, height, flip, d.owner, d.bary, d.ids, d.points, d.normals, d.albedo, &n, &hbm_bytes_));
    st.only(out.ids, n); st.only(out.points, (size_t)n * 3); st.only(out.normals, (size_t)n * 3); st.only(out.albedo, (size_t)n * 3);     // the n covered entries
    HIP_TRY(st.download());
    if (!device) HIP_TRY(hipStreamSynchronize(stream_));
    if (ncovered) *ncovered = n;
    return true;
}

// mi355rt_bake_atlas: the ids are checked on the device first; verdict != 0: refused, nothing written (the caller words the error)
bool Renderer::bake_atlas(const uint32_t* ids, const float* values3, uint32_t n, uint32_t width, uint32_t height, uint32_t dilate, bool device, float* atlas, uint8_t* valid, uint32_t& verdict)
{
    if (!quiet()) return false;
    const size_t nt = (size_t)width * height;
    Staging st(stream_, &hbm_bytes_, device);
    const uint32_t* d_ids = st.in(ids, n, true); const float* d_values = st.in(values3, (size_t)n * 3, true);      // n == 0: the callee still takes pointers
    float* d_atlas = st.scratch(atlas, nt * 3); uint8_t* d_valid = st.scratch(valid, nt);                          // the fill works on both, whichever the caller asked for
    HIP_TRY(st.error());
    HIP_TRY(bake_atlas_device(stream_, d_ids, d_values, n, width, height, dilate, d_atlas, d_valid, &verdict, &hbm_bytes_));
    if (verdict) return true;                                         // refused: nothing is copied back
    HIP_TRY(st.download());
    if (!device) HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// mi355rt_render_rays: mi355rt_render whose passes read their primary rays from the caller's buffer, indexed by the CALL's sample number (enqueue_frame hands
// every pass its base).  Only the rays of owned rows are read, so a host buffer is staged whole but a striped handle never looks at the rest.
bool Renderer::render_rays(const float* rays6, uint32_t spp, bool device)
{
    if (!begin_call()) return false;
    const size_t nrays = (size_t)cfg.width * cfg.height * spp;
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_rays = st.in(rays6, nrays * 6);
    HIP_TRY(st.error());
    HIP_TRY(hipEventRecord(slices_[0].done, stream_));                // the other slices fork behind the upload (slice 0 runs on the main stream; its `done` event is free here)
    RayFeed f{};
    f.mode = kRaysOfPixels; f.rays = d_rays;
    caller_ray_film_ = true;
    if (!enqueue_frame(spp, slices_[0].done, nullptr, &f)) return false;
    for (uint32_t r : owned_rows) ldr_dirty_[r] = 1;
    return end_call((uint64_t)owned_rows.size() * cfg.width * spp, true);
}

// ---- lens models (include/mi355rt.h) ---------------------------------------------------------------------------------------
// The film, the caller-ray mark, the counters and current_row stay; a speculative 50-row frame was traced for the lens that is leaving and is given up.
bool Renderer::set_lens(const mi355rt_lens& l)
{
    if (std::memcmp(&l, &lens_, sizeof l) == 0) return true;
    if (!quiet()) return false;
    lens_ = l;
    return true;
}

// mi355rt_lens_rays: one launch on the main stream, behind whatever is queued (render_async joins its slices there).  Host memory: through a temporary
// device buffer.  Nothing of the handle changes.
bool Renderer::lens_rays(uint32_t spp, bool device, float* rays6)
{
    if (!quiet()) return false;
    const size_t nrays = (size_t)cfg.width * cfg.height * spp;
    Staging st(stream_, &hbm_bytes_, device);
    float* d = st.out(rays6, nrays * 6);
    HIP_TRY(st.error());
    HIP_TRY(launch_lens_rays(stream_, device_camera(), cfg.flags, (uint32_t)cfg.seed, spp, d_film_n_.get(), d));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));                           // the caller's buffer is complete, on whatever stream it is used next
    return true;
}

bool Renderer::debug_numerics(const float* a, const float* b, size_t n, float* q, float* r, float* p)
{
    if (!bind()) return false;
    if (n == 0) return true;
    Staging st(stream_, &hbm_bytes_, false);
    const float* d_a = st.in(a, n); const float* d_b = st.in(b, n);
    float* d_q = st.out(q, n); float* d_r = st.out(r, n); float* d_p = st.out(p, n);
    HIP_TRY(st.error());
    HIP_TRY(launch_numerics(stream_, d_a, d_b, (uint32_t)n, d_q, d_r, d_p));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// mi355rt_debug_gather_rate: the divergent-gather rate of this device's vector memory pipe (kernels.hip, gather_rate_kernel).
// out[0] = cache-line accesses per second (64 lanes x 2 loads per wave-step, each lane on its own line), out[1] = kernel ms,
// out[2] = 32-byte node fetches per second.
bool Renderer::debug_gather_rate(uint32_t table_nodes, uint32_t steps, double out[3])
{
    if (!bind()) return false;
    if (table_nodes < 1024 || steps == 0) { last_error = "bad debug_gather_rate arguments"; return false; }
    std::vector<uint32_t> host((size_t)table_nodes * 8);
    uint32_t x = 12345u;
    for (uint32_t& v : host) { x = x * 1664525u + 1013904223u; v = x >> 8; }
    DeviceBuffer<> d; DeviceBuffer<uint32_t> sink;
    HIP_TRY(d.alloc(host.size() * 4));
    HIP_TRY(sink.alloc(4));
    HIP_TRY(hipMemcpy(d.get(), host.data(), host.size() * 4, hipMemcpyHostToDevice));
    float best = 0.0f;
    for (int rep = 0; rep < 3; ++rep) {                                // first launch warms the caches and the clocks
        HIP_TRY(hipEventRecord(ev_begin_, stream_));
        HIP_TRY(launch_gather_rate(stream_, num_cus_, d.get(), table_nodes, steps, sink.get()));
        HIP_TRY(hipEventRecord(ev_end_, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev_begin_, ev_end_));
        if (rep > 0 && (best == 0.0f || ms < best)) best = ms;
    }
    if (best <= 0.0f) return false;
    const double wave_steps = (double)num_cus_ * 8.0 * 4.0 * steps;
    out[0] = wave_steps * 128.0 / (best * 1e-3); out[1] = best; out[2] = wave_steps * 64.0 / (best * 1e-3);
    return true;
}

bool Renderer::debug_slab(const float* inv_rays6, const float* cubes6, size_t n, uint8_t* hit, float* tmin)
{
    if (!bind()) return false;
    if (n == 0) return true;
    if (n > (1u << 24)) { last_error = "too many slab tests in one batch"; return false; }
    Staging st(stream_, &hbm_bytes_, false);
    const float* d_rays = st.in(inv_rays6, n * 6); const float* d_cubes = st.in(cubes6, n * 6);
    uint8_t* d_hit = st.out(hit, n); float* d_tmin = st.out(tmin, n);
    HIP_TRY(st.error());
    HIP_TRY(launch_slab(stream_, d_rays, d_cubes, (uint32_t)n, d_hit, d_tmin));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// Film::get_pixels / get_estimated_variances computed on the device, downloaded as width*height*3 floats
bool Renderer::film_stat(bool variances, float* rgb)
{
    if (!quiet()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    Staging st(stream_, &hbm_bytes_, false);
    float* d = st.out(rgb, npix * 3);
    HIP_TRY(st.error());
    HIP_TRY(launch_film_stat(stream_, variances, npix, d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), d));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// ---- denoised read-out (include/mi355rt.h) ------------------------------------------------------------------------
// What a pixel's camera ray depends on: the camera, the FIX_ROW_INDEX bit and the lens.  The key of the guides cache and the camera stamp of the feature film.
std::vector<float> Renderer::view_key()
{
    const DCamera cam = device_camera();
    std::vector<float> key(cam.rot, cam.rot + 16);
    key.insert(key.end(), cam.origin, cam.origin + 3); key.push_back(cam.max_x); key.push_back(cam.max_y);
    key.push_back((cfg.flags & MI355RT_FLAG_FIX_ROW_INDEX) ? 1.0f : 0.0f);
    key.push_back((float)lens_.model);                                // the lens: its model and the fields that model reads (validated: finite)
    key.push_back(lens_.model == MI355RT_LENS_THIN ? lens_.radius : 0.0f); key.push_back(lens_.model == MI355RT_LENS_THIN ? lens_.focus : 0.0f);
    key.push_back(lens_.model == MI355RT_LENS_ORTHO ? lens_.width_world : 0.0f);
    return key;
}

// ---- feature film (include/mi355rt.h "FEATURE FILM") -------------------------------------------------------------------
// Everything runs on stream_: behind a queued frame (render_async joins its slices there) and behind the rows a speculative frame gives back.  Nothing but
// the feature film, its stamp and its version changes: no film, counter, row or dirty-row state.
bool Renderer::ensure_features()
{
    if (d_features_) return true;
    const size_t npix = (size_t)cfg.width * cfg.height;
    DeviceBuffer<uint8_t> b;
    HIP_TRY(b.alloc(npix * 36, &hbm_bytes_));
    HIP_TRY(hipMemsetAsync(b.get(), 0, npix * 36, stream_));
    d_features_ = std::move(b);
    feat_.n = reinterpret_cast<uint32_t*>(d_features_.get());
    feat_.hits = feat_.n + npix;
    feat_.depth = reinterpret_cast<float*>(feat_.hits + npix);
    feat_.normal = feat_.depth + npix;
    feat_.albedo = feat_.normal + 3 * npix;
    return true;
}

bool Renderer::feature_view_current() { return feat_stamp_ == kFeatCamera && feat_key_ == view_key(); }

bool Renderer::features_render(const float* rays6, uint32_t spp, bool device)
{
    if (!quiet()) return false;
    if (!ensure_features()) return false;
    const size_t nrays = (size_t)cfg.width * cfg.height * spp;
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_rays = st.in(rays6, nrays * 6);                    // null: the handle's own rays
    HIP_TRY(st.error());
    const DCamera cam = device_camera();
    HIP_TRY(launch_features(stream_, dscene_, cam, cfg.flags & MI355RT_FLAG_FIX_ROW_INDEX, (uint32_t)cfg.seed, traversal_rows(),
                            (int)mode_, d_owned_rows_.get(), (uint32_t)owned_rows.size(), spp, d_rays, feat_));
    if (feat_stamp_ == kFeatEmpty) {
        feat_stamp_ = rays6 ? kFeatRays : kFeatCamera;
        if (!rays6) feat_key_ = view_key();
    }
    ++feat_version_;
    HIP_TRY(hipStreamSynchronize(stream_));                           // the caller's rays and the staging are free again
    return true;
}

bool Renderer::features_clear()
{
    if (!quiet()) return false;
    feat_stamp_ = kFeatEmpty; feat_key_.clear();
    ++feat_version_;
    if (!d_features_) return true;
    HIP_TRY(launch_features_clear(stream_, d_owned_rows_.get(), (uint32_t)owned_rows.size(), cfg.width, feat_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// A feature film that was never allocated reads as the zeros it would hold
bool Renderer::features_get(uint32_t* n, uint32_t* hits, float* depth, float* normal3, float* albedo3)
{
    if (!quiet()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!d_features_) {
        if (n) std::memset(n, 0, npix * 4);
        if (hits) std::memset(hits, 0, npix * 4);
        if (depth) std::memset(depth, 0, npix * 4);
        if (normal3) std::memset(normal3, 0, npix * 12);
        if (albedo3) std::memset(albedo3, 0, npix * 12);
        return true;
    }
    if (n) HIP_TRY(hipMemcpyAsync(n, feat_.n, npix * 4, hipMemcpyDeviceToHost, stream_));
    if (hits) HIP_TRY(hipMemcpyAsync(hits, feat_.hits, npix * 4, hipMemcpyDeviceToHost, stream_));
    if (depth) HIP_TRY(hipMemcpyAsync(depth, feat_.depth, npix * 4, hipMemcpyDeviceToHost, stream_));
    if (normal3) HIP_TRY(hipMemcpyAsync(normal3, feat_.normal, npix * 12, hipMemcpyDeviceToHost, stream_));
    if (albedo3) HIP_TRY(hipMemcpyAsync(albedo3, feat_.albedo, npix * 12, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

bool Renderer::features_alpha(float* alpha)
{
    if (!quiet()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!d_features_) { std::memset(alpha, 0, npix * 4); return true; }
    Staging st(stream_, &hbm_bytes_, false);
    float* d = st.out(alpha, npix);
    HIP_TRY(st.error());
    HIP_TRY(launch_features_alpha(stream_, (uint32_t)npix, feat_, d));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// MI355RT_GUIDES_FEATURES: the guides converted from the feature film, rebuilt (stream-ordered) only when it has changed; the caller has checked that it holds samples
bool Renderer::refresh_feature_guides()
{
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!d_features_) { last_error = "internal: no feature film"; return false; }
    if (!d_fguide0_) {
        DeviceBuffer<float4> g0, g1;          // both or neither
        HIP_TRY(g0.alloc(npix * sizeof(float4), &hbm_bytes_));
        HIP_TRY(g1.alloc(npix * sizeof(float4), &hbm_bytes_));
        d_fguide0_ = std::move(g0); d_fguide1_ = std::move(g1);
        fguides_version_ = feat_version_ - 1;
    }
    if (fguides_version_ == feat_version_) return true;
    HIP_TRY(launch_features_guides(stream_, (uint32_t)npix, feat_, d_fguide0_.get(), d_fguide1_.get()));
    fguides_version_ = feat_version_;
    return true;
}

// The guides on the device for the current camera, FIX_ROW_INDEX bit and lens: rebuilt (stream-ordered, on the main stream) only when that key changes.
// Under MI355RT_GUIDES_FEATURES: the feature film's (guide0() / guide1() name the buffers of the source in force).
bool Renderer::refresh_guides()
{
    if (guide_source_ == MI355RT_GUIDES_FEATURES) return refresh_feature_guides();
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!d_guide0_) {
        DeviceBuffer<float4> g0, g1;          // both or neither
        HIP_TRY(g0.alloc(npix * sizeof(float4), &hbm_bytes_));
        HIP_TRY(g1.alloc(npix * sizeof(float4), &hbm_bytes_));
        d_guide0_ = std::move(g0); d_guide1_ = std::move(g1);
        guides_key_.clear();
    }
    const DCamera cam = device_camera();
    const std::vector<float> key = view_key();
    if (key == guides_key_) return true;
    guides_key_.clear();
    HIP_TRY(launch_guides(stream_, dscene_, cam, cfg.flags & MI355RT_FLAG_FIX_ROW_INDEX, traversal_rows(), (int)mode_,
                          d_guide0_.get(), d_guide1_.get()));
    guides_key_ = key;
    return true;
}

bool Renderer::get_guides(float* depth, float* normal3, float* albedo3, uint32_t* prim)
{
    if (!quiet()) return false;
    if (!refresh_guides()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    std::vector<float4> g0(npix), g1(npix);
    HIP_TRY(hipMemcpyAsync(g0.data(), guide0(), npix * sizeof(float4), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(g1.data(), guide1(), npix * sizeof(float4), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    for (size_t p = 0; p < npix; ++p) {
        if (depth) depth[p] = g0[p].w;
        if (normal3) { normal3[3 * p] = g0[p].x; normal3[3 * p + 1] = g0[p].y; normal3[3 * p + 2] = g0[p].z; }
        if (albedo3) { albedo3[3 * p] = g1[p].x; albedo3[3 * p + 1] = g1[p].y; albedo3[3 * p + 2] = g1[p].z; }
        if (prim) std::memcpy(&prim[p], &g1[p].w, 4);
    }
    return true;
}

// The filter of one read-out, queued on the main stream: afterwards d_dn_rgb_ (rgb) and / or d_dn_packed_ (packed) hold its result
bool Renderer::run_denoise(const mi355rt_denoise_config& dc, bool rgb, bool packed, bool split)
{
    if (split && !d_film_direct_) { last_error = "internal: no direct film"; return false; }
    if (!settle_speculation()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (!d_dn_ping_) {                        // all five or none
        DeviceBuffer<float4> ping, pong; DeviceBuffer<uint32_t> flags, pk; DeviceBuffer<float> out;
        HIP_TRY(ping.alloc(npix * sizeof(float4), &hbm_bytes_));
        HIP_TRY(pong.alloc(npix * sizeof(float4), &hbm_bytes_));
        HIP_TRY(flags.alloc(npix * 4, &hbm_bytes_));
        HIP_TRY(out.alloc(npix * 12, &hbm_bytes_));
        HIP_TRY(pk.alloc(npix * 4, &hbm_bytes_));
        d_dn_ping_ = std::move(ping); d_dn_pong_ = std::move(pong); d_dn_flags_ = std::move(flags); d_dn_rgb_ = std::move(out); d_dn_packed_ = std::move(pk);
    }
    if (!refresh_guides()) return false;
    DenoiseArgs a{};
    a.width = cfg.width; a.height = cfg.height; a.step = 1u; a.normal_power_log2 = dc.normal_power_log2;
    a.sigma_luminance = dc.sigma_luminance; a.sigma_depth = dc.sigma_depth; a.sigma_albedo = dc.sigma_albedo;
    HIP_TRY(launch_denoise(stream_, a, dc.iterations, d_film_sum_.get(), d_film_sumsq_.get(), d_film_n_.get(), split ? d_film_direct_.get() : nullptr,
                           guide0(), guide1(), d_dn_flags_.get(),
                           d_dn_ping_.get(), d_dn_pong_.get(), rgb ? d_dn_rgb_.get() : nullptr, packed ? d_dn_packed_.get() : nullptr));
    return true;
}

bool Renderer::get_denoised(const mi355rt_denoise_config& dc, float* rgb, uint32_t* packed, bool split)
{
    if (!bind()) return false;
    if (!run_denoise(dc, rgb != nullptr, packed != nullptr, split)) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    if (rgb) HIP_TRY(hipMemcpyAsync(rgb, d_dn_rgb_.get(), npix * 12, hipMemcpyDeviceToHost, stream_));
    if (packed) HIP_TRY(hipMemcpyAsync(packed, d_dn_packed_.get(), npix * 4, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

// ---- display read-out (include/mi355rt.h) -----------------------------------------------------------------------------
// The source image on the device, stream-ordered: the film's sums, or the rgb read-out of the denoiser, run here (once per call)
bool Renderer::display_source(uint32_t source, const mi355rt_denoise_config& dn, const float*& img, bool& film)
{
    film = source == MI355RT_DISPLAY_SOURCE_FILM;
    if (film) {
        if (!settle_speculation()) return false;
        img = d_film_sum_.get();
        return true;
    }
    if (!run_denoise(dn, true, false, source == MI355RT_DISPLAY_SOURCE_DENOISED_SPLIT)) return false;
    img = d_dn_rgb_.get();
    return true;
}

bool Renderer::display_hist_queue(const float* img, bool film, mi355rt_luminance_histogram& out)
{
    static_assert(sizeof(mi355rt_luminance_histogram) == kDisplayHistWords * 4, "the kernel's words are the struct");
    if (!d_disp_hist_) HIP_TRY(d_disp_hist_.alloc(kDisplayHistWords * 4, &hbm_bytes_));
    HIP_TRY(hipMemsetAsync(d_disp_hist_.get(), 0, kDisplayHistWords * 4, stream_));
    HIP_TRY(launch_display_hist(stream_, num_cus_, cfg.width * cfg.height, img, d_film_n_.get(), film, d_disp_hist_.get()));
    HIP_TRY(hipMemcpyAsync(&out, d_disp_hist_.get(), kDisplayHistWords * 4, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

bool Renderer::display_histogram(uint32_t source, const mi355rt_denoise_config& dn, mi355rt_luminance_histogram& out)
{
    if (!bind()) return false;
    const float* img = nullptr; bool film = true;
    if (!display_source(source, dn, img, film)) return false;
    return display_hist_queue(img, film, out);
}

bool Renderer::get_display(const mi355rt_display_config& dc, const mi355rt_denoise_config& dn, uint32_t* packed, float& exposure_used)
{
    if (!bind()) return false;
    const size_t npix = (size_t)cfg.width * cfg.height;
    const float* img = nullptr; bool film = true;
    if (!display_source(dc.source, dn, img, film)) return false;
    if (!ensure_display_buffers(true)) return false;      // with the first call, whatever it asks for: the handle's memory does not depend on the configs that follow
    float E = dc.exposure;
    if (dc.auto_exposure) {
        mi355rt_luminance_histogram hist;
        if (!display_hist_queue(img, film, hist)) return false;
        E = display_auto_exposure(hist, dc.key, dc.low, dc.high);
    }
    HIP_TRY(launch_display_pack(stream_, display_args(&dc, E), (uint32_t)npix, img, d_film_n_.get(), film, d_disp_table_.get(), d_disp_packed_.get()));
    HIP_TRY(hipMemcpyAsync(packed, d_disp_packed_.get(), npix * 4, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    exposure_used = E;
    return true;
}

// mi355rt_display_image: display_pack_kernel on an image that is no film (as mi355rt_get_relit_pixels feeds it), all buffers of the call's own — the
// handle's display buffers are sized for its frame and allocated on first use, and this call must not move hbm_allocated_bytes.  The kernel reads a sample
// count per pixel that only a film uses: a zeroed plane stands in for it.
bool Renderer::display_image(const float* rgb3, size_t npix, const mi355rt_display_config* dc, uint32_t* packed)
{
    if (!bind()) return false;
    float t[256];
    display_srgb_table(t);
    Staging st(stream_, &hbm_bytes_, false);
    const float* tab = st.in(t, 256); const float* img = st.in(rgb3, npix * 3);
    uint32_t* cnt = st.scratch<uint32_t>(nullptr, npix);
    uint32_t* out = st.out(packed, npix);
    HIP_TRY(st.error());
    HIP_TRY(hipMemsetAsync(cnt, 0, npix * 4, stream_));
    HIP_TRY(launch_display_pack(stream_, display_args(dc, dc ? dc->exposure : 1.0f), (uint32_t)npix, img, cnt, false, tab, out));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));
    return true;
}

bool Renderer::debug_sample(uint32_t pixel, uint32_t sampleno, float* color3, float* node_L, size_t nodes)
{
    if (!bind()) return false;
    if (nodes < nodes_per_sample || pixel >= cfg.width * cfg.height) { last_error = "bad debug_sample arguments"; return false; }
    if (!settle_speculation()) return false;
    call_done_valid_ = false;
    HIP_TRY(hipMemsetAsync(d_counters_.get(), 0, sizeof(DCounters) * kShards, stream_));
    ev_used_ = 0; counts_pending_ = false;
    PassRequest rq;
    rq.nrows = 1; rq.explicit_sample = true; rq.epixel = pixel; rq.esample = sampleno;
    if (!run_pass(slices_[0], rq)) return false;
    HIP_TRY(hipStreamSynchronize(stream_));
    const uint32_t nl = std::max(nlights_, 1u);
    std::vector<float> raw((size_t)nodes_per_sample * nl * 3);
    uint32_t sl = 0xFFFFFFFFu;
    HIP_TRY(hipMemcpy(&sl, slices_[0].d_sample_slot.get(), 4, hipMemcpyDeviceToHost));
    std::fill(raw.begin(), raw.end(), 0.0f);
    if (sl != 0xFFFFFFFFu)         // slot_L is node-major: plane q = node * nlights + light, kChunk slots in this one-sample pass
        for (size_t q = 0; q < (size_t)nodes_per_sample * nl; ++q)
            HIP_TRY(hipMemcpy(raw.data() + 3 * q, slices_[0].d_slot_L.get() + 3 * (q * kChunk + sl), 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(color3, d_debug_color_.get(), 12, hipMemcpyDeviceToHost));
    for (uint32_t nd = 0; nd < nodes_per_sample; ++nd) {
        float acc[3] = { 0.0f, 0.0f, 0.0f };
        for (uint32_t li = 0; li < nlights_; ++li)
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + raw[3 * ((size_t)nd * nl + li) + c];
        node_L[3 * nd] = acc[0]; node_L[3 * nd + 1] = acc[1]; node_L[3 * nd + 2] = acc[2];
    }
    return true;
}

// ---- probe placement (include/mi355rt.h, "PROBE PLACEMENT") -----------------------------------------------------------------------------
// mi355rt_probes_survey: probes_gather's samples through gather's chunk loop, but not through a pass: a ray-fed pass cannot stop after its primary round, and
// the survey wants closest hits and no radiance.  The loop makes the chunk's rays and traces nothing (traced = false); the reduce traces them with the
// closest-hit launch of mi355rt_intersect_rays into two chunk temporaries (tuv, prim: 16 bytes per entry, made when the first, largest chunk arrives) and
// folds them with the survey kernel.  The counters see no bounce and no shadow ray; the call reports npoints * spp primary rays.
bool Renderer::probes_survey(const float* points3, const uint32_t* ids, size_t npoints, const mi355rt_probe_survey_config& sc, bool device, const mi355rt_probe_survey& out)
{
    if (!begin_call()) return false;
    const size_t total = npoints * sc.spp;
    Staging st(stream_, &hbm_bytes_, device);
    const float* d_points = st.in(points3, npoints * 3); const uint32_t* d_ids = st.in(ids, npoints);
    const bool acc = sc.accumulate != 0;                              // then the outputs go up first: the call continues what they hold
    uint32_t* d_n = st.out(out.n, npoints, acc); uint32_t* d_back = st.out(out.back, npoints, acc); uint32_t* d_front = st.out(out.front, npoints, acc);
    float* d_nb = st.out(out.near_back, npoints * 4, acc); float* d_nf = st.out(out.near_front, npoints * 4, acc); float* d_far = st.out(out.far, npoints * 4, acc);
    HIP_TRY(st.error());
    DeviceBuffer<float> c_tuv; DeviceBuffer<uint32_t> c_prim;
    if (!gather_chunks(d_points, nullptr, d_ids, npoints, sc.spp, sc.first_sample, false, false, false, [&](const GatherChunk& c) {
            const size_t entries = (size_t)c.cp * c.cs;
            if (c_prim.bytes() < entries * 4) {
                hipError_t e = c_tuv.alloc(entries * 12, &hbm_bytes_);
                if (e == hipSuccess) e = c_prim.alloc(entries * 4, &hbm_bytes_);
                if (e != hipSuccess) return e;
            }
            const hipError_t e = launch_intersect(stream_, dscene_, traversal_rows(), (int)mode_, c.rays, (uint32_t)entries, false, c_tuv.get(), c_prim.get(), nullptr);
            if (e != hipSuccess) return e;
            return launch_probes_survey(stream_, c.point0, c.cp, c.cs, !acc && c.sample0 == 0, (sc.flags & MI355RT_SURVEY_FLIP) != 0, sc.max_distance, dscene_.ntri, c.rays,
                                        c_tuv.get(), c_prim.get(), dscene_.normals, d_n, d_back, d_front, d_nb, d_nf, d_far);
        })) return false;
    HIP_TRY(st.download());
    return end_call(total, true);                                     // waits: the staging (and the caller's buffers) are free again
}

// mi355rt_probes_place: arithmetic on the caller's arrays, one kernel, and probes_lookup's rules around it.
bool Renderer::probes_place(const mi355rt_probe_grid& grid, const mi355rt_probe_survey& survey, const mi355rt_probe_place_config& pc, const float* offsets, bool device,
                            float* new_offsets, uint8_t* verdict, uint8_t* state)
{
    if (!quiet()) return false;
    const size_t nprobes = (size_t)grid.counts[0] * grid.counts[1] * grid.counts[2];
    ShGrid g;
    std::memcpy(&g, &grid, sizeof g);
    Staging st(stream_, &hbm_bytes_, device);
    const uint32_t* d_n = st.in((const uint32_t*)survey.n, nprobes); const uint32_t* d_back = st.in((const uint32_t*)survey.back, nprobes);
    const uint32_t* d_front = st.in((const uint32_t*)survey.front, nprobes);
    const float* d_nb = st.in((const float*)survey.near_back, nprobes * 4); const float* d_nf = st.in((const float*)survey.near_front, nprobes * 4);
    const float* d_far = st.in((const float*)survey.far, nprobes * 4);
    const float* d_off = st.in(offsets, nprobes * 3);
    float* d_new = st.out(new_offsets, nprobes * 3); uint8_t* d_verdict = st.out(verdict, nprobes); uint8_t* d_state = st.out(state, nprobes);
    HIP_TRY(st.error());
    HIP_TRY(launch_probes_place(stream_, g, PlaceConfig{ pc.back_share, pc.max_offset, pc.min_front, pc.max_distance }, (uint32_t)nprobes, d_n, d_back, d_front, d_nb, d_nf, d_far,
                                d_off, d_new, d_verdict, d_state));
    HIP_TRY(st.download());
    HIP_TRY(hipStreamSynchronize(stream_));                           // the caller's buffers are complete, on whatever stream they are used next
    return true;
}

// mi355rt_probes_lookup_placed: the probes' offsets among the volume's arrays too; null offsets still launch this kernel
bool Renderer::probes_lookup_placed(const mi355rt_probe_grid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const mi355rt_probe_depth& depth,
                                    const mi355rt_probe_vis_config& vc, const float* offsets, const float* points3, const float* dirs3, const float* normals3, size_t npoints,
                                    uint32_t mode, bool device, float* rgb3, uint8_t* ok)
{
    return volume_readout({ &grid, n, sh, usable, &depth, &vc, offsets }, points3, dirs3, normals3, npoints, device, rgb3, ok,
                          [&](const LitVolume& v, const float* p, const float* d, const float* nr, float* rgb, uint8_t* k) {
                              return launch_probes_lookup_placed(stream_, v.grid, v.n, v.sh, v.usable, v.R, v.count, v.moments, v.offsets, v.flags, v.normal_bias, p, d, nr, npoints, mode,
                                                                 rgb, k);
                          });
}

// ---- probe-lit shading (include/mi355rt.h, "PROBE-LIT") ----------------------------------------------------------------------------------
// mi355rt_probe_lit_points: the hemisphere mean as one more read-out of the volume
bool Renderer::probe_lit_points(const mi355rt_probe_volume& vol, const float* points3, const float* normals3, size_t npoints, uint32_t flags, bool device, float* indirect3, uint8_t* ok)
{
    return volume_readout(vol, points3, nullptr, normals3, npoints, device, indirect3, ok, [&](const LitVolume& v, const float* p, const float*, const float* nr, float* ind, uint8_t* k) {
        return launch_probe_lit_points(stream_, v, (flags & MI355RT_PROBE_LIT_CLAMP) != 0, p, nr, npoints, ind, k);
    });
}

// mi355rt_probe_lit_rays: the rays in chunks; per chunk the closest-hit launch of mi355rt_intersect_rays into two chunk temporaries (as probes_survey takes
// its hits), the surface kernel's shadow rays through launch_intersect in shadow mode (as gather takes `direct`), then the shade kernel.  The temporaries are
// made at the first, largest chunk and go with the call.  The counters see no bounce and no shadow ray; the call reports nrays primary rays.
bool Renderer::probe_lit_rays(const mi355rt_probe_volume& vol, const float* rays6, size_t nrays, uint32_t flags, bool device, const mi355rt_probe_lit_outputs& out)
{
    if (!begin_call()) return false;
    Staging st(stream_, &hbm_bytes_, device);
    const LitVolume v = stage_volume(st, vol);
    const float* d_rays = st.in(rays6, nrays * 6);
    LitOutputs d{};
    d.rgb = st.out(out.rgb, nrays * 3); d.light = st.out(out.light, nrays * 3); d.indirect = st.out(out.indirect, nrays * 3);
    d.tuv = st.out(out.tuv, nrays * 3, true);                         // goes up first: a miss leaves it as it was
    d.prim = st.out(out.prim, nrays); d.ok = st.out(out.ok, nrays);
    HIP_TRY(st.error());
    const size_t nl = std::max(nlights_, 1u);
    const size_t per = std::min(nrays, std::max<size_t>(1, std::min(pass_sample_budget(), ((size_t)4 << 20) / nl)));
    DeviceBuffer<float> c_tuv, c_shadow; DeviceBuffer<uint32_t> c_prim; DeviceBuffer<uint8_t> c_blocked;
    for (size_t at = 0; at < nrays; at += per) {
        const uint32_t cn = (uint32_t)std::min(per, nrays - at);
        if (!c_prim) {
            HIP_TRY(c_tuv.alloc(per * 12, &hbm_bytes_)); HIP_TRY(c_prim.alloc(per * 4, &hbm_bytes_));
            if (nlights_) { HIP_TRY(c_shadow.alloc(per * nlights_ * 24, &hbm_bytes_)); HIP_TRY(c_blocked.alloc(per * nlights_, &hbm_bytes_)); }
        }
        const float* r = d_rays + 6 * at;
        HIP_TRY(launch_intersect(stream_, dscene_, traversal_rows(), (int)mode_, r, cn, false, c_tuv.get(), c_prim.get(), nullptr));
        if (nlights_) {
            HIP_TRY(launch_probe_lit_surface(stream_, dscene_, r, c_tuv.get(), c_prim.get(), cn, c_shadow.get()));
            HIP_TRY(launch_intersect(stream_, dscene_, traversal_rows(), (int)mode_, c_shadow.get(), cn * nlights_, true, nullptr, nullptr, c_blocked.get()));
        }
        const LitOutputs o{ d.rgb ? d.rgb + 3 * at : nullptr, d.light ? d.light + 3 * at : nullptr, d.indirect ? d.indirect + 3 * at : nullptr, d.tuv ? d.tuv + 3 * at : nullptr,
                            d.prim ? d.prim + at : nullptr, d.ok ? d.ok + at : nullptr };
        HIP_TRY(launch_probe_lit_shade(stream_, dscene_, v, (flags & MI355RT_PROBE_LIT_CLAMP) != 0, r, c_tuv.get(), c_prim.get(), c_blocked.get(), cn, o));
    }
    HIP_TRY(st.download());
    return end_call(nrays, true);                                     // waits: the staging, the chunk temporaries (and the caller's buffers) are free again
}

}  // namespace mi355rt
