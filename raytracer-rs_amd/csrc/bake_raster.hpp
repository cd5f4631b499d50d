// bake_raster.hpp — the per-texel arithmetic of a bake (include/mi355rt.h, "BAKE").  ONE statement, compiled for the host
// (mi355rt_bake_texel, mi355rt_bake_auto_atlas) and for the device (csrc/bake.hip): f32, unfused (every file that includes this is built with
// -ffp-contract=off), expression for expression what raytracer-rs_amd/bake.py writes in numpy.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace mi355rt {

constexpr uint32_t kBakeMiss = 0xFFFFFFFFu;
constexpr uint32_t kBakeTile = 8u;            // texels per tile edge: one wave rasterises one tile, one lane per texel

// The UV triangle in texel units: px_k = u_k * (float)width, py_k = v_k * (float)height
struct BakeTri { float px[3], py[3]; };
__host__ __device__ __forceinline__ BakeTri bake_tri(const float* uv6, uint32_t width, uint32_t height)
{
    BakeTri t;
    const float w = (float)width, h = (float)height;
    t.px[0] = uv6[0] * w; t.py[0] = uv6[1] * h;
    t.px[1] = uv6[2] * w; t.py[1] = uv6[3] * h;
    t.px[2] = uv6[4] * w; t.py[2] = uv6[5] * h;
    return t;
}

// The texels a triangle is tested against: x in [floor(min px) - 1, floor(max px) + 1], y alike, cut to the atlas.  An exactly covered centre has
// min px <= x + 0.5 <= max px and lies well inside; the box only takes from a sliver the far centres that nothing but the rounding of its edge functions
// gives it.  The bounds are clamped to the atlas as floats before they become integers.  A NaN or infinite coordinate gives an empty box: such a chart
// covers nothing (its edge functions would be infinite or NaN, and so would the points made from them).
// Returns false: no texel.  x0 .. x1, y0 .. y1 inclusive.
__host__ __device__ __forceinline__ bool bake_box(const BakeTri& t, uint32_t width, uint32_t height, int32_t& x0, int32_t& x1, int32_t& y0, int32_t& y1)
{
    const float lox = floorf(fminf(fminf(t.px[0], t.px[1]), t.px[2])) - 1.0f, hix = floorf(fmaxf(fmaxf(t.px[0], t.px[1]), t.px[2])) + 1.0f;
    const float loy = floorf(fminf(fminf(t.py[0], t.py[1]), t.py[2])) - 1.0f, hiy = floorf(fmaxf(fmaxf(t.py[0], t.py[1]), t.py[2])) + 1.0f;
    // x - x == 0 fails for NaN and for +-inf alike (fminf / fmaxf would drop a NaN operand: the coordinates themselves are asked)
    const bool finite = t.px[0] - t.px[0] == 0.0f && t.px[1] - t.px[1] == 0.0f && t.px[2] - t.px[2] == 0.0f && t.py[0] - t.py[0] == 0.0f && t.py[1] - t.py[1] == 0.0f && t.py[2] - t.py[2] == 0.0f;
    if (!finite) return false;
    const float w = (float)width, h = (float)height;
    if (!(lox < w) || !(hix >= 0.0f) || !(loy < h) || !(hiy >= 0.0f)) return false;
    x0 = (int32_t)(lox > 0.0f ? lox : 0.0f); x1 = (int32_t)(hix < w - 1.0f ? hix : w - 1.0f);
    y0 = (int32_t)(loy > 0.0f ? loy : 0.0f); y1 = (int32_t)(hiy < h - 1.0f ? hiy : h - 1.0f);
    return true;
}

// edge(p, q) relative to the texel centre: (px_p - cx) * (py_q - cy) - (py_p - cy) * (px_q - cx); edge(p, q) == -edge(q, p) exactly
struct BakeEdges { float e0, e1, e2, s; };
__host__ __device__ __forceinline__ BakeEdges bake_edges(const BakeTri& t, uint32_t x, uint32_t y)
{
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const float ax = t.px[0] - cx, ay = t.py[0] - cy, bx = t.px[1] - cx, by = t.py[1] - cy, qx = t.px[2] - cx, qy = t.py[2] - cy;
    BakeEdges e;
    e.e0 = bx * qy - by * qx;      // edge(b, c)
    e.e1 = qx * ay - qy * ax;      // edge(c, a)
    e.e2 = ax * by - ay * bx;      // edge(a, b)
    e.s = (e.e0 + e.e1) + e.e2;
    return e;
}
__host__ __device__ __forceinline__ bool bake_covered(const BakeEdges& e)
{
    return (((e.e0 >= 0.0f) & (e.e1 >= 0.0f) & (e.e2 >= 0.0f)) | ((e.e0 <= 0.0f) & (e.e1 <= 0.0f) & (e.e2 <= 0.0f))) & (e.s != 0.0f);
}
// the box test for one texel (the device walks bins built from the same box)
__host__ __device__ __forceinline__ bool bake_in_box(const BakeTri& t, uint32_t width, uint32_t height, uint32_t x, uint32_t y)
{
    int32_t x0, x1, y0, y1;
    if (!bake_box(t, width, height, x0, x1, y0, y1)) return false;
    return (int32_t)x >= x0 && (int32_t)x <= x1 && (int32_t)y >= y0 && (int32_t)y <= y1;
}

// P = (A + u * (B - A)) + v * (C - A) per component; e1 = B - A and e2 = C - A as the scene's triangles hold them
__host__ __device__ __forceinline__ float bake_point(float a, float e1, float e2, float u, float v) { return (a + u * e1) + v * e2; }

// the texel of a texture at (u, v), texture.rs:21-27 as kernels.hip's fetch_texel restates it: `as usize` truncation (NaN and negatives -> 0), the index
// clamped to the last texel
__host__ __device__ __forceinline__ unsigned long long bake_texel_index(uint32_t tw, uint32_t th, float u, float v)
{
    const float fx = u * (float)tw, fy = v * (float)th;
    unsigned long long x = fx > 0.0f ? (fx >= 1.8446744e19f ? ~0ull : (unsigned long long)fx) : 0ull;
    unsigned long long y = fy > 0.0f ? (fy >= 1.8446744e19f ? ~0ull : (unsigned long long)fy) : 0ull;
    const unsigned long long n = (unsigned long long)tw * th;
    unsigned long long i = (y > n ? n : y) * tw + (x > n ? n : x);
    if (i >= n) i = n - 1;
    return i;
}

// One step of the atlas dilation for an EMPTY texel (x, y): the mean of the non-empty 8-neighbours of the previous image in the order N, W, E, S, NW, NE, SW,
// SE, (((v0 + v1) + v2) + ...) / (float)count.  valid(i) / value(i, c) read texel index i.  Returns the count (0: the texel stays empty, rgb untouched).
template <class Valid, class Value>
__host__ __device__ __forceinline__ uint32_t bake_dilate_texel(Valid valid, Value value, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float rgb[3])
{
    const int dx[8] = { 0, -1, 1, 0, -1, 1, -1, 1 }, dy[8] = { -1, 0, 0, 1, -1, -1, 1, 1 };
    uint32_t count = 0;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int k = 0; k < 8; ++k) {
        const long long nx = (long long)x + dx[k], ny = (long long)y + dy[k];
        if (nx < 0 || ny < 0 || nx >= (long long)width || ny >= (long long)height) continue;
        const size_t i = (size_t)ny * width + (size_t)nx;
        if (!valid(i)) continue;
        if (count == 0) { s0 = value(i, 0); s1 = value(i, 1); s2 = value(i, 2); }
        else { s0 = s0 + value(i, 0); s1 = s1 + value(i, 1); s2 = s2 + value(i, 2); }
        ++count;
    }
    if (count) { const float c = (float)count; rgb[0] = s0 / c; rgb[1] = s1 / c; rgb[2] = s2 / c; }
    return count;
}

// mi355rt_bake_auto_atlas: a chart for a mesh that has none.  Two triangles per square cell of `cell` texels, cells row by row from the top left:
// triangle i sits in cell i / 2 at (ox, oy) = ((i / 2) % cols * cell, (i / 2) / cols * cell), cols = width / cell.  With g = gutter, L = cell - 2 g and
// d = max(g - 0.5, 0.5), leg = L - d:
//     even i:  A = (ox + g, oy + g)                  B = (ox + g + leg, oy + g)                C = (ox + g, oy + g + leg)
//     odd i:   A = (ox + cell - g, oy + cell - g)    B = (ox + cell - g - leg, oy + cell - g)  C = (ox + cell - g, oy + cell - g - leg)
// in texels; uv = (x / (float)width, y / (float)height), one f32 division each.  The legs lie on texel borders and the two hypotenuses on x + y = integer
// + 0.5, so no centre is within 0.35 texels of an edge and the rounding of uv * size cannot move one across.  The texels a cell's halves own differ by
// at least 2 d in x + y, so they are max(g, 1) texels apart (Chebyshev), and owned texels of neighbouring cells are 2 g + 1 apart.
// cell is the largest with (width / cell) * (height / cell) >= ceil(ntri / 2); each half owns a texel iff L >= 1 + d.  Returns null, or why it is refused.
inline const char* bake_auto_atlas(uint32_t ntri, uint32_t width, uint32_t height, uint32_t gutter, float* uv, uint32_t* cell_out)
{
    if (ntri == 0) return "ntri is 0";
    if (width == 0 || height == 0) return "width and height must be >= 1";
    if (width > 16384u || height > 16384u) return "width and height must be <= 16384";
    if (gutter > 16384u) return "gutter must be <= 16384";
    const unsigned long long cells = ((unsigned long long)ntri + 1ull) / 2ull;
    uint32_t cell = width < height ? width : height;
    while (cell && (unsigned long long)(width / cell) * (height / cell) < cells) --cell;
    const float g = (float)gutter, d = gutter ? g - 0.5f : 0.5f;
    if (cell == 0 || (float)cell - 2.0f * g < 1.0f + d) return "the atlas is too small: a cell cannot give both of its triangles a texel (larger atlas, or smaller gutter)";
    const uint32_t cols = width / cell;
    const float c = (float)cell, leg = (c - 2.0f * g) - d, w = (float)width, h = (float)height;
    for (uint32_t i = 0; i < ntri; ++i) {
        const float ox = (float)((i / 2u) % cols * cell), oy = (float)((i / 2u) / cols * cell);
        float* o = uv + 6ull * i;
        if ((i & 1u) == 0u) {
            const float ax = ox + g, ay = oy + g;
            o[0] = ax / w; o[1] = ay / h; o[2] = (ax + leg) / w; o[3] = ay / h; o[4] = ax / w; o[5] = (ay + leg) / h;
        } else {
            const float ax = (ox + c) - g, ay = (oy + c) - g;
            o[0] = ax / w; o[1] = ay / h; o[2] = (ax - leg) / w; o[3] = ay / h; o[4] = ax / w; o[5] = (ay - leg) / h;
        }
    }
    if (cell_out) *cell_out = cell;
    return nullptr;
}

}  // namespace mi355rt
