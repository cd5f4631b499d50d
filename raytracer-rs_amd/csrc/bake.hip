// bake.hip — the device side of a bake (include/mi355rt.h, "BAKE"): the texture-space rasteriser that turns UV charts into texels and
// surface points (mi355rt_bake_texels), and the atlas scatter and dilation (mi355rt_bake_atlas).  The per-texel arithmetic is csrc/bake_raster.hpp, the
// statement raytracer-rs_amd/bake.py.  Shaped like the frame's screen-space rasteriser (kernels.hip, raster_tile): the UV triangles are binned into tiles
// of 8 x 8 texels (count, scan, fill), one wave takes one tile with one lane per texel, and all 64 lanes test the SAME triangle, its six UV floats coming
// through the scalar cache.  Every lane keeps the lowest covering index, so no atomic decides a result and the order inside a bin does not matter.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <algorithm>
#include <cstdint>
#include "bake.hpp"
#include "bake_raster.hpp"
#include "device_buffer.hpp"

namespace mi355rt {
namespace {

constexpr int kBakeBlock = 256;
constexpr uint32_t kBakeSmallRect = 16u;      // a triangle whose box touches more tiles is binned by a whole block, not by one lane
constexpr uint32_t kBakeWideGrid = 1024u;     // blocks that share the wide triangles

typedef uint32_t bu32x2_t __attribute__((ext_vector_type(2)));
typedef const bu32x2_t __attribute__((address_space(4))) * bake_u2_ptr;     // constant address space: a wave-uniform address loads through the scalar cache
typedef const uint32_t __attribute__((address_space(4))) * bake_u1_ptr;
typedef const unsigned long long __attribute__((address_space(4))) * bake_u64_ptr;

// the tiles a triangle's box touches (bake_box >> 3); false: none
__device__ __forceinline__ bool tile_rect(const float* __restrict__ uv6, uint32_t width, uint32_t height, uint32_t& tx0, uint32_t& tx1, uint32_t& ty0, uint32_t& ty1)
{
    float u[6];
    for (int k = 0; k < 6; ++k) u[k] = uv6[k];
    const BakeTri t = bake_tri(u, width, height);
    int32_t x0, x1, y0, y1;
    if (!bake_box(t, width, height, x0, x1, y0, y1)) return false;
    tx0 = (uint32_t)x0 / kBakeTile; tx1 = (uint32_t)x1 / kBakeTile; ty0 = (uint32_t)y0 / kBakeTile; ty1 = (uint32_t)y1 / kBakeTile;
    return true;
}

// count (FILL false): counts[tile] += 1;  fill: entries[ofs[tile] + cursor[tile]++] = tri.  `counts` is the count array or the cursor array.
template <bool FILL>
__device__ __forceinline__ void bin_one(uint32_t tile, uint32_t tri, uint32_t* __restrict__ counts, const unsigned long long* __restrict__ ofs, uint32_t* __restrict__ entries)
{
    const uint32_t pos = atomicAdd(&counts[tile], 1u);
    if (FILL) entries[ofs[tile] + pos] = tri;
}

}  // namespace

// one lane per triangle: the small ones are binned here, the wide ones listed for bake_bin_wide_kernel (count launch) or left to it (fill launch)
template <bool FILL>
__global__ __launch_bounds__(kBakeBlock) void bake_bin_kernel(const float* __restrict__ uv, uint32_t ntri, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                             uint32_t* __restrict__ counts, const unsigned long long* __restrict__ ofs, uint32_t* __restrict__ entries,
                                                             uint32_t* __restrict__ wide, uint32_t* __restrict__ nwide)
{
    const uint32_t tri = blockIdx.x * kBakeBlock + threadIdx.x;
    if (tri >= ntri) return;
    uint32_t tx0, tx1, ty0, ty1;
    if (!tile_rect(uv + 6ull * tri, width, height, tx0, tx1, ty0, ty1)) return;
    const uint32_t nx = tx1 - tx0 + 1u, n = nx * (ty1 - ty0 + 1u);
    if (n > kBakeSmallRect) {
        if (!FILL) wide[atomicAdd(nwide, 1u)] = tri;          // at most ntri entries: every triangle is listed once
        return;
    }
    for (uint32_t i = 0; i < n; ++i) bin_one<FILL>((ty0 + i / nx) * tiles_x + tx0 + i % nx, tri, counts, ofs, entries);
}

// the wide triangles: the blocks share the list, a block's lanes share a triangle's tiles, so a chart over the whole atlas costs every lane a few tiles
template <bool FILL>
__global__ __launch_bounds__(kBakeBlock) void bake_bin_wide_kernel(const float* __restrict__ uv, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                  uint32_t* __restrict__ counts, const unsigned long long* __restrict__ ofs, uint32_t* __restrict__ entries,
                                                                  const uint32_t* __restrict__ wide, const uint32_t* __restrict__ nwide)
{
    const uint32_t nw = *nwide;
    for (uint32_t w = blockIdx.x; w < nw; w += gridDim.x) {
        const uint32_t tri = wide[w];
        uint32_t tx0, tx1, ty0, ty1;
        if (!tile_rect(uv + 6ull * tri, width, height, tx0, tx1, ty0, ty1)) continue;
        const uint32_t nx = tx1 - tx0 + 1u, n = nx * (ty1 - ty0 + 1u);
        for (uint32_t i = threadIdx.x; i < n; i += kBakeBlock) bin_one<FILL>((ty0 + i / nx) * tiles_x + tx0 + i % nx, tri, counts, ofs, entries);
    }
}

// One wave per tile, one lane per texel: the lowest index of the tile's list that covers the lane's centre, then (u, v) of that triangle.
__global__ __launch_bounds__(kBakeBlock) void bake_raster_kernel(const float* __restrict__ uv, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t ntiles,
                                                                const unsigned long long* __restrict__ ofs_g, const uint32_t* __restrict__ entries_g,
                                                                uint32_t* __restrict__ owner_out, float* __restrict__ bary)
{
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBakeBlock / 64) + threadIdx.x / 64u));
    if (tile >= ntiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = (tile % tiles_x) * kBakeTile + (lane & 7u), y = (tile / tiles_x) * kBakeTile + (lane >> 3);
    const bake_u64_ptr ofs = (bake_u64_ptr)(uintptr_t)ofs_g;
    const bake_u1_ptr entries = (bake_u1_ptr)(uintptr_t)entries_g;
    const bake_u2_ptr uv2 = (bake_u2_ptr)(uintptr_t)uv;
    const unsigned long long first = ofs[tile], last = ofs[tile + 1u];
    uint32_t owner = kBakeMiss;
    for (unsigned long long e = first; e < last; ++e) {
        const uint32_t tri = entries[e];
        const bu32x2_t a = uv2[3ull * tri], b = uv2[3ull * tri + 1u], c = uv2[3ull * tri + 2u];
        const float u6[6] = { __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(c.x), __uint_as_float(c.y) };
        const BakeTri t = bake_tri(u6, width, height);
        const bool hit = bake_in_box(t, width, height, x, y) && bake_covered(bake_edges(t, x, y));
        owner = (hit & (tri < owner)) ? tri : owner;
    }
    if (x >= width || y >= height) return;
    const size_t texel = (size_t)y * width + x;
    owner_out[texel] = owner;
    if (owner == kBakeMiss) return;
    float u6[6];
    for (int k = 0; k < 6; ++k) u6[k] = uv[6ull * owner + k];
    const BakeEdges e = bake_edges(bake_tri(u6, width, height), x, y);
    bary[2 * texel] = e.e1 / e.s;
    bary[2 * texel + 1] = e.e2 / e.s;
}

struct BakeIsCovered { __host__ __device__ uint32_t operator()(uint32_t o) const { return o != kBakeMiss ? 1u : 0u; } };

// the covered texels' indices, ascending: entry incl[t] - 1 of a covered texel t
__global__ __launch_bounds__(kBakeBlock) void bake_ids_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ incl, uint32_t ntexels, uint32_t* __restrict__ ids)
{
    const uint32_t t = blockIdx.x * kBakeBlock + threadIdx.x;
    if (t >= ntexels || owner[t] == kBakeMiss) return;
    ids[incl[t] - 1u] = t;
}

// the lists, consecutive lanes on consecutive entries: point, normal and diffuse colour of entry k (texel ids[k]); any list may be null
__global__ __launch_bounds__(kBakeBlock) void bake_lists_kernel(DScene sc, const float* __restrict__ tri9, const uint32_t* __restrict__ ids, uint32_t n, uint32_t flip,
                                                               const uint32_t* __restrict__ owner, const float* __restrict__ bary,
                                                               float* __restrict__ points, float* __restrict__ normals, float* __restrict__ albedo)
{
    const uint32_t k = blockIdx.x * kBakeBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t t = ids[k], tri = owner[t];
    const float u = bary[2ull * t], v = bary[2ull * t + 1];
    const float4 nq = reinterpret_cast<const float4*>(sc.normals)[tri];
    if (points) {
        const float* q = tri9 + 9ull * tri;
        for (int a = 0; a < 3; ++a) points[3ull * k + a] = bake_point(q[a], q[3 + a], q[6 + a], u, v);
    }
    if (normals) {
        normals[3ull * k] = flip ? -nq.x : nq.x; normals[3ull * k + 1] = flip ? -nq.y : nq.y; normals[3ull * k + 2] = flip ? -nq.z : nq.z;
    }
    if (albedo) {
        const DMaterial m = sc.materials[__float_as_uint(nq.w)];
        float r = m.r, g = m.g, b = m.b;
        if (m.kind_tex & 0x80000000u) {
            const DTexture tx = sc.textures[m.kind_tex & 0x7FFFFFFFu];
            const float* p = sc.texels + 3ull * (tx.offset + bake_texel_index(tx.width, tx.height, u, v));
            r = p[0]; g = p[1]; b = p[2];
        }
        albedo[3ull * k] = r; albedo[3ull * k + 1] = g; albedo[3ull * k + 2] = b;
    }
}

// ---- atlas -------------------------------------------------------------------------------------------------------------------------------------
// seen[id] counts the entries that name texel id; verdict |= 1: an id >= ntexels, |= 2: an id named twice
__global__ __launch_bounds__(kBakeBlock) void bake_check_ids_kernel(const uint32_t* __restrict__ ids, uint32_t n, uint32_t ntexels, uint32_t* __restrict__ seen, uint32_t* __restrict__ verdict)
{
    const uint32_t k = blockIdx.x * kBakeBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t id = ids[k];
    if (id >= ntexels) { atomicOr(verdict, 1u); return; }
    if (atomicAdd(&seen[id], 1u) != 0u) atomicOr(verdict, 2u);
}

// ids were checked: in range, no repeats
__global__ __launch_bounds__(kBakeBlock) void bake_scatter_kernel(const uint32_t* __restrict__ ids, const float* __restrict__ values, uint32_t n, float* __restrict__ atlas, uint8_t* __restrict__ valid)
{
    const uint32_t k = blockIdx.x * kBakeBlock + threadIdx.x;
    if (k >= n) return;
    const size_t id = ids[k];
    atlas[3 * id] = values[3ull * k]; atlas[3 * id + 1] = values[3ull * k + 1]; atlas[3 * id + 2] = values[3ull * k + 2];
    valid[id] = 1u;
}

// one iteration, previous image -> next image (every texel is written); mark: 1 + iteration, saturated
__global__ __launch_bounds__(kBakeBlock) void bake_dilate_kernel(uint32_t width, uint32_t height, uint32_t mark, const float* __restrict__ src, const uint8_t* __restrict__ src_valid,
                                                                float* __restrict__ dst, uint8_t* __restrict__ dst_valid)
{
    const uint32_t t = blockIdx.x * kBakeBlock + threadIdx.x;
    if (t >= width * height) return;
    float rgb[3] = { src[3ull * t], src[3ull * t + 1], src[3ull * t + 2] };
    uint8_t v = src_valid[t];
    if (!v) {
        const uint32_t count = bake_dilate_texel([src_valid](size_t i) { return src_valid[i] != 0; }, [src](size_t i, int c) { return src[3 * i + c]; },
                                                 width, height, t % width, t / width, rgb);
        if (count) v = (uint8_t)mark;
    }
    dst[3ull * t] = rgb[0]; dst[3ull * t + 1] = rgb[1]; dst[3ull * t + 2] = rgb[2];
    dst_valid[t] = v;
}

namespace {

inline uint32_t blocks_for(size_t n) { return (uint32_t)((n + kBakeBlock - 1) / kBakeBlock); }

#define BAKE_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

}  // namespace

hipError_t bake_texels_device(hipStream_t stream, const DScene& sc, const float* tri9, const float* uv, uint32_t ntri, uint32_t width, uint32_t height, bool flip,
                              uint32_t* owner, float* bary, uint32_t* ids, float* points, float* normals, float* albedo, uint32_t* ncovered, size_t* hbm)
{
    const uint32_t tiles_x = (width + kBakeTile - 1) / kBakeTile, tiles_y = (height + kBakeTile - 1) / kBakeTile, ntiles = tiles_x * tiles_y;
    const uint32_t ntexels = width * height;
    DeviceBuffer<uint32_t> d_counts, d_wide, d_nwide, d_entries, d_incl, d_ids;
    DeviceBuffer<unsigned long long> d_ofs;
    DeviceBuffer<> d_tmp;
    BAKE_TRY(d_counts.alloc(((size_t)ntiles + 1) * 4, hbm));
    BAKE_TRY(d_ofs.alloc(((size_t)ntiles + 1) * 8, hbm));
    BAKE_TRY(d_wide.alloc((size_t)std::max(ntri, 1u) * 4, hbm));
    BAKE_TRY(d_nwide.alloc(4, hbm));
    BAKE_TRY(d_incl.alloc((size_t)ntexels * 4, hbm));
    size_t scan_a = 0, scan_b = 0;
    auto covered = rocprim::make_transform_iterator(owner, BakeIsCovered());
    BAKE_TRY(rocprim::exclusive_scan(nullptr, scan_a, d_counts.get(), d_ofs.get(), 0ull, (size_t)ntiles + 1, rocprim::plus<unsigned long long>(), stream));
    BAKE_TRY(rocprim::inclusive_scan(nullptr, scan_b, covered, d_incl.get(), (size_t)ntexels, rocprim::plus<uint32_t>(), stream));
    BAKE_TRY(d_tmp.alloc(std::max<size_t>({ scan_a, scan_b, 16 }), hbm));
    // 1. bins: count, scan, fill
    BAKE_TRY(hipMemsetAsync(d_counts.get(), 0, ((size_t)ntiles + 1) * 4, stream));
    BAKE_TRY(hipMemsetAsync(d_nwide.get(), 0, 4, stream));
    if (ntri) {
        hipLaunchKernelGGL(bake_bin_kernel<false>, dim3(blocks_for(ntri)), dim3(kBakeBlock), 0, stream, uv, ntri, width, height, tiles_x, d_counts.get(), (const unsigned long long*)nullptr, (uint32_t*)nullptr, d_wide.get(), d_nwide.get());
        hipLaunchKernelGGL(bake_bin_wide_kernel<false>, dim3(std::min(kBakeWideGrid, ntri)), dim3(kBakeBlock), 0, stream, uv, width, height, tiles_x, d_counts.get(), (const unsigned long long*)nullptr, (uint32_t*)nullptr, d_wide.get(), d_nwide.get());
    }
    BAKE_TRY(rocprim::exclusive_scan(d_tmp.get(), scan_a, d_counts.get(), d_ofs.get(), 0ull, (size_t)ntiles + 1, rocprim::plus<unsigned long long>(), stream));
    unsigned long long total = 0;
    BAKE_TRY(hipMemcpyAsync(&total, d_ofs.get() + ntiles, 8, hipMemcpyDeviceToHost, stream));
    BAKE_TRY(hipStreamSynchronize(stream));
    BAKE_TRY(d_entries.alloc((size_t)std::max<unsigned long long>(total, 1ull) * 4, hbm));
    if (total) {
        BAKE_TRY(hipMemsetAsync(d_counts.get(), 0, ((size_t)ntiles + 1) * 4, stream));     // the counts become the fill cursors
        hipLaunchKernelGGL(bake_bin_kernel<true>, dim3(blocks_for(ntri)), dim3(kBakeBlock), 0, stream, uv, ntri, width, height, tiles_x, d_counts.get(), (const unsigned long long*)d_ofs.get(), d_entries.get(), d_wide.get(), d_nwide.get());
        hipLaunchKernelGGL(bake_bin_wide_kernel<true>, dim3(std::min(kBakeWideGrid, ntri)), dim3(kBakeBlock), 0, stream, uv, width, height, tiles_x, d_counts.get(), (const unsigned long long*)d_ofs.get(), d_entries.get(), d_wide.get(), d_nwide.get());
    }
    // 2. owner and (u, v)
    hipLaunchKernelGGL(bake_raster_kernel, dim3((ntiles + kBakeBlock / 64 - 1) / (kBakeBlock / 64)), dim3(kBakeBlock), 0, stream, uv, width, height, tiles_x, ntiles,
                       (const unsigned long long*)d_ofs.get(), (const uint32_t*)d_entries.get(), owner, bary);
    // 3. the covered texels in ascending order
    BAKE_TRY(rocprim::inclusive_scan(d_tmp.get(), scan_b, covered, d_incl.get(), (size_t)ntexels, rocprim::plus<uint32_t>(), stream));
    uint32_t n = 0;
    BAKE_TRY(hipMemcpyAsync(&n, d_incl.get() + (ntexels - 1), 4, hipMemcpyDeviceToHost, stream));
    BAKE_TRY(hipStreamSynchronize(stream));
    if (ncovered) *ncovered = n;
    if (n && (ids || points || normals || albedo)) {
        if (!ids) { BAKE_TRY(d_ids.alloc((size_t)n * 4, hbm)); ids = d_ids.get(); }
        hipLaunchKernelGGL(bake_ids_kernel, dim3(blocks_for(ntexels)), dim3(kBakeBlock), 0, stream, (const uint32_t*)owner, (const uint32_t*)d_incl.get(), ntexels, ids);
        if (points || normals || albedo)
            hipLaunchKernelGGL(bake_lists_kernel, dim3(blocks_for(n)), dim3(kBakeBlock), 0, stream, sc, tri9, (const uint32_t*)ids, n, flip ? 1u : 0u, (const uint32_t*)owner, (const float*)bary, points, normals, albedo);
    }
    BAKE_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);          // the temporaries go out of scope here
}

hipError_t bake_atlas_device(hipStream_t stream, const uint32_t* ids, const float* values, uint32_t n, uint32_t width, uint32_t height, uint32_t dilate,
                             float* atlas, uint8_t* valid, uint32_t* verdict, size_t* hbm)
{
    const uint32_t ntexels = width * height;
    *verdict = 0;
    if (n) {
        DeviceBuffer<uint32_t> d_seen;
        BAKE_TRY(d_seen.alloc(((size_t)ntexels + 1) * 4, hbm));      // the last word is the verdict
        BAKE_TRY(hipMemsetAsync(d_seen.get(), 0, ((size_t)ntexels + 1) * 4, stream));
        hipLaunchKernelGGL(bake_check_ids_kernel, dim3(blocks_for(n)), dim3(kBakeBlock), 0, stream, ids, n, ntexels, d_seen.get(), d_seen.get() + ntexels);
        BAKE_TRY(hipMemcpyAsync(verdict, d_seen.get() + ntexels, 4, hipMemcpyDeviceToHost, stream));
        BAKE_TRY(hipStreamSynchronize(stream));
        if (*verdict) return hipSuccess;                              // refused: nothing is written
    }
    // an empty texel that can be filled at all lies within max(width, height) - 1 texels (Chebyshev) of a given one and is filled by that iteration:
    // further ones change nothing and are not run
    const uint32_t iters = std::min(dilate, std::max(width, height) - 1u);
    DeviceBuffer<float> d_pong; DeviceBuffer<uint8_t> d_pong_valid;
    if (iters) { BAKE_TRY(d_pong.alloc((size_t)ntexels * 12, hbm)); BAKE_TRY(d_pong_valid.alloc(ntexels, hbm)); }
    // the last iteration writes the caller's buffers: start on the side that makes it so
    float* img[2] = { atlas, d_pong.get() }; uint8_t* val[2] = { valid, d_pong_valid.get() };
    uint32_t cur = iters & 1u;
    BAKE_TRY(hipMemsetAsync(img[cur], 0, (size_t)ntexels * 12, stream));
    BAKE_TRY(hipMemsetAsync(val[cur], 0, ntexels, stream));
    if (n) hipLaunchKernelGGL(bake_scatter_kernel, dim3(blocks_for(n)), dim3(kBakeBlock), 0, stream, ids, values, n, img[cur], val[cur]);
    for (uint32_t k = 1; k <= iters; ++k) {
        hipLaunchKernelGGL(bake_dilate_kernel, dim3(blocks_for(ntexels)), dim3(kBakeBlock), 0, stream, width, height, std::min(1u + k, 255u), (const float*)img[cur], (const uint8_t*)val[cur], img[cur ^ 1u], val[cur ^ 1u]);
        cur ^= 1u;
    }
    BAKE_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

}  // namespace mi355rt
