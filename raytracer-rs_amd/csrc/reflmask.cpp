// reflmask.cpp — per-triangle direction masks for the reflection rays (see reflmask.hpp).
#include "reflmask.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>

namespace mi355rt {
namespace {

struct V3 { double x, y, z; };
inline V3 sub(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline V3 add(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline V3 mul(V3 a, double s) { return { a.x * s, a.y * s, a.z * s }; }
inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
inline double len(V3 a) { return std::sqrt(dot(a, a)); }
inline bool unit(V3& a) { const double l = len(a); if (!(l > 0.0) || !std::isfinite(l)) return false; a = mul(a, 1.0 / l); return true; }

// face f = 2 * major axis + (direction component negative); the two other axes (a, b) in ascending order (lightmap.cpp, light_proves_unoccluded)
const int kAxisA[3] = { 1, 0, 0 }, kAxisB[3] = { 2, 2, 1 };

struct Bin {
    V3 corner[4];        // unit vectors, in order around the bin
    V3 face[4];          // unit normals of the four planes through the origin that bound the bin's pyramid, pointing inwards
    V3 centre;
    double cos_rho, sin_rho;   // rho: the largest angle between the centre and a corner
};

void make_bins(uint32_t B, std::vector<Bin>& bins)
{
    bins.resize((size_t)6 * B * B);
    for (uint32_t f = 0; f < 6; ++f) {
        const int m = (int)(f >> 1), a = kAxisA[m], b = kAxisB[m];
        const double sg = (f & 1u) ? -1.0 : 1.0;
        auto dir = [&](double u, double v) { double w[3]; w[m] = sg; w[a] = u; w[b] = v; V3 d = { w[0], w[1], w[2] }; unit(d); return d; };
        for (uint32_t i = 0; i < B; ++i) for (uint32_t j = 0; j < B; ++j) {
            Bin& bn = bins[((size_t)f * B + i) * B + j];
            const double u0 = 2.0 * i / B - 1.0, u1 = 2.0 * (i + 1) / B - 1.0, v0 = 2.0 * j / B - 1.0, v1 = 2.0 * (j + 1) / B - 1.0;
            bn.corner[0] = dir(u0, v0); bn.corner[1] = dir(u1, v0); bn.corner[2] = dir(u1, v1); bn.corner[3] = dir(u0, v1);
            bn.centre = dir(0.5 * (u0 + u1), 0.5 * (v0 + v1));
            double cmin = 1.0;
            for (int k = 0; k < 4; ++k) {
                cmin = std::min(cmin, dot(bn.centre, bn.corner[k]));
                V3 w = cross(bn.corner[k], bn.corner[(k + 1) & 3]); unit(w);
                if (dot(w, bn.centre) < 0.0) w = mul(w, -1.0);
                bn.face[k] = w;
            }
            cmin = std::max(cmin - 1e-12, -1.0);
            bn.cos_rho = cmin; bn.sin_rho = std::sqrt(std::max(0.0, 1.0 - cmin * cmin));
        }
    }
}

// a plain tree over the triangles' boxes (median split), walked per triangle
struct Node { V3 c, h; double r; int32_t left, right; uint32_t first, count; };

struct Tree {
    std::vector<Node> nodes;
    std::vector<uint32_t> order;
    const float* verts;
    int32_t build(uint32_t lo, uint32_t hi)
    {
        V3 mn = { 1e300, 1e300, 1e300 }, mx = { -1e300, -1e300, -1e300 }, cmn = mn, cmx = mx;
        for (uint32_t k = lo; k < hi; ++k) {
            const float* v = verts + 9 * (size_t)order[k];
            V3 c = { 0, 0, 0 };
            for (int q = 0; q < 3; ++q) {
                const V3 p = { v[3 * q], v[3 * q + 1], v[3 * q + 2] };
                mn = { std::min(mn.x, p.x), std::min(mn.y, p.y), std::min(mn.z, p.z) }; mx = { std::max(mx.x, p.x), std::max(mx.y, p.y), std::max(mx.z, p.z) };
                c = add(c, mul(p, 1.0 / 3.0));
            }
            cmn = { std::min(cmn.x, c.x), std::min(cmn.y, c.y), std::min(cmn.z, c.z) }; cmx = { std::max(cmx.x, c.x), std::max(cmx.y, c.y), std::max(cmx.z, c.z) };
        }
        const int32_t id = (int32_t)nodes.size();
        nodes.push_back(Node{});
        Node nd; nd.c = mul(add(mn, mx), 0.5); nd.h = mul(sub(mx, mn), 0.5); nd.r = len(nd.h) * (1.0 + 1e-12); nd.left = nd.right = -1; nd.first = lo; nd.count = hi - lo;
        if (hi - lo > 4u) {
            const V3 e = sub(cmx, cmn);
            const int ax = e.x >= e.y && e.x >= e.z ? 0 : e.y >= e.z ? 1 : 2;
            const uint32_t mid = lo + (hi - lo) / 2u;
            const float* vv = verts;
            std::nth_element(order.begin() + lo, order.begin() + mid, order.begin() + hi, [vv, ax](uint32_t p, uint32_t q) {
                const float* a = vv + 9 * (size_t)p; const float* b = vv + 9 * (size_t)q;
                return (double)a[ax] + a[3 + ax] + a[6 + ax] < (double)b[ax] + b[3 + ax] + b[6 + ax]; });
            nd.left = build(lo, mid); nd.right = build(mid, hi);
        }
        nodes[(size_t)id] = nd;
        return id;
    }
};

struct Walker {
    const std::vector<Bin>& bins;
    const std::vector<Bin>& groups;     // the quadrants of the faces (make_bins(2)): a cap is tested against a quadrant before it is tested against its bins
    uint32_t B;
    const Tree& tree;
    const float* verts;
    double pad, min_cos, pad_angle, sin_pad;
    uint32_t nbits;
    struct Cap { V3 centre; double cos_rho, sin_rho; };
    std::vector<Cap> bcap, gcap;        // the bounding caps of the bins and of the quadrants, packed for cap_touch
    std::vector<uint16_t> clear[24];   // the bins of the current triangle that are still clear, per quadrant
    uint32_t nclear = 0;
    V3 normal = { 0, 0, 1 };            // of the current triangle
    double up_sin;
    std::vector<uint16_t> touched, cand;
    uint64_t work = 0, exacts = 0;

    Walker(const std::vector<Bin>& b, const std::vector<Bin>& g, uint32_t B_, const Tree& t, const float* v, double p, double mc, double pa)
        : bins(b), groups(g), B(B_), tree(t), verts(v), pad(p), min_cos(mc), pad_angle(pa), sin_pad(std::sin(pa)), nbits((uint32_t)b.size()), up_sin(std::sqrt(1.0 - mc * mc))
    {
        for (const Bin& x : b) bcap.push_back(Cap{ x.centre, x.cos_rho, x.sin_rho });
        for (const Bin& x : g) gcap.push_back(Cap{ x.centre, x.cos_rho, x.sin_rho });
    }
    uint32_t group_of(uint32_t b) const { const uint32_t j = b % B, i = (b / B) % B, f = b / (B * B); return f * 4u + (i >= B / 2u ? 2u : 0u) + (j >= B / 2u ? 1u : 0u); }

    static V3 vert(const float* v, int q) { return { v[3 * q], v[3 * q + 1], v[3 * q + 2] }; }

    // Which clear bins does the cap of half-angle `half` (cos, sin given) around the unit vector d touch?  Conservative: a bin counts as its bounding cap.
    void cap_touch(V3 d, double cos_half, double sin_half)
    {
        touched.clear();
        {   // every clear bin lies in the cap of the directions that rise by the minimum cosine around the normal
            const double c = cos_half * min_cos - sin_half * up_sin, s = sin_half * min_cos + cos_half * up_sin;
            if (s > 0.0 && dot(normal, d) < c) return;
        }
        // touched unless angle(centre, d) > half + rho, i.e. unless cos(angle) < cos(half + rho) with half + rho < pi
        auto touches = [&](const Cap& bn) {
            const double c = cos_half * bn.cos_rho - sin_half * bn.sin_rho, s = sin_half * bn.cos_rho + cos_half * bn.sin_rho;   // cos / sin of half + rho
            return s <= 0.0 || dot(bn.centre, d) >= c;
        };
        for (uint32_t g = 0; g < 24u; ++g) {
            if (clear[g].empty() || !touches(gcap[g])) continue;
            for (uint16_t b : clear[g]) if (touches(bcap[b])) touched.push_back(b);
        }
    }
    void all_clear() { touched.clear(); for (uint32_t g = 0; g < 24u; ++g) touched.insert(touched.end(), clear[g].begin(), clear[g].end()); }
    void set_bins(const std::vector<uint16_t>& which, uint32_t* row)
    {
        for (uint16_t b : which) {
            row[b >> 5] |= 1u << (b & 31u);
            std::vector<uint16_t>& cl = clear[group_of(b)];
            auto it = std::find(cl.begin(), cl.end(), b);
            if (it != cl.end()) { *it = cl.back(); cl.pop_back(); --nclear; }
        }
    }

    // The exact cone of triangle U seen from the shrunken triangle tp: the conic hull of the nine vertex differences.  A clear bin stays clear only when a plane
    // through the origin separates it from the cone by the angular pad: one of the bin's own four planes, or a supporting plane of the cone.
    void exact(const V3 tp[3], V3 n, const float* u9, uint32_t* row)
    {
        ++work;
        {   // U lies wholly at or below T's plane (a half space is convex: so does the conic hull of the nine differences), while every direction of a clear bin
            // rises: U is not met.  (Generators that rise only a little do NOT bound the hull's rise: a wide triangle passing low over T has nine flat
            // generators and a hull that points straight up.)
            bool below = true;
            for (int i = 0; i < 3 && below; ++i) for (int j = 0; j < 3; ++j) {
                const V3 d = sub(vert(u9, j), tp[i]);
                const double nd = dot(n, d);
                if (!(nd <= 0.0) && !(nd * nd <= 1e-18 * dot(d, d))) { below = false; break; }
            }
            if (below) return;
        }
        ++exacts;
        V3 a[9];
        bool ok = true;
        for (int i = 0; i < 3 && ok; ++i) for (int j = 0; j < 3; ++j) {
            V3 d = sub(vert(u9, j), tp[i]);
            if (!unit(d)) { ok = false; break; }
            a[3 * i + j] = d;
        }
        {   // the candidates: the clear bins touched by a cap that holds the nine generators (a cap of less than a right angle is convex: it holds their conic hull)
            V3 mean = { 0, 0, 0 };
            for (int k = 0; k < 9 && ok; ++k) mean = add(mean, a[k]);
            double cmin = 1.0;
            if (ok && unit(mean)) for (int k = 0; k < 9; ++k) cmin = std::min(cmin, dot(mean, a[k])); else cmin = 0.0;
            if (cmin > 0.1) {
                cmin -= 1e-12;
                const double smax = std::sqrt(std::max(0.0, 1.0 - cmin * cmin)), cp = std::cos(pad_angle);
                cap_touch(mean, cmin * cp - smax * sin_pad, smax * cp + cmin * sin_pad);
                if (touched.empty()) return;
            } else all_clear();
        }
        cand.assign(touched.begin(), touched.end());
        // first the bins' own planes; the cone's supporting planes are worked out only when some bin is left
        touched.clear();
        for (uint16_t b : cand) {
            const Bin& bn = bins[b];
            bool separated = false;
            for (int f = 0; f < 4 && ok && !separated; ++f) {
                bool out = true;
                for (int k = 0; k < 9; ++k) if (!(dot(bn.face[f], a[k]) < -sin_pad - 1e-9)) { out = false; break; }
                separated = out;
            }
            if (!separated) touched.push_back(b);
        }
        if (touched.empty()) return;
        if (ok) {
            V3 sup[40]; int nsup = 0;
            for (int p = 0; p < 9 && nsup < 38; ++p) for (int q = p + 1; q < 9 && nsup < 38; ++q) {
                V3 w = cross(a[p], a[q]);
                if (!(len(w) > 1e-9) || !unit(w)) continue;
                double lo = 0.0, hi = 0.0;
                for (int k = 0; k < 9 && (hi <= 1e-9 || lo >= -1e-9); ++k) { const double s = dot(w, a[k]); lo = std::min(lo, s); hi = std::max(hi, s); }
                if (hi <= 1e-9) sup[nsup++] = w;                      // the whole cone in w . x <= 0
                else if (lo >= -1e-9) sup[nsup++] = mul(w, -1.0);
            }
            cand.assign(touched.begin(), touched.end());
            touched.clear();
            for (uint16_t b : cand) {
                const Bin& bn = bins[b];
                bool separated = false;
                for (int s = 0; s < nsup && !separated; ++s) {
                    bool in = true;
                    for (int k = 0; k < 4; ++k) if (!(dot(sup[s], bn.corner[k]) > sin_pad + 1e-9)) { in = false; break; }
                    separated = in;
                }
                if (!separated) touched.push_back(b);
            }
        }
        cand.assign(touched.begin(), touched.end());
        set_bins(cand, row);
    }

    void triangle(uint32_t t, uint32_t* row, uint32_t stride)
    {
        const uint32_t mask_words = stride - kReflGuardWords;
        for (uint32_t k = 0; k < mask_words; ++k) row[k] = 0xFFFFFFFFu;
        const float* v = verts + 9 * (size_t)t;
        std::memcpy(&row[mask_words], v, 12);
        float hmin = std::numeric_limits<float>::infinity();
        std::memcpy(&row[mask_words + 3], &hmin, 4);
        for (int k = 0; k < 9; ++k) if (!std::isfinite(v[k])) return;
        const V3 p0 = vert(v, 0), p1 = vert(v, 1), p2 = vert(v, 2);
        V3 n = cross(sub(p1, p0), sub(p2, p0));              // calc_normal's side (mod.rs:198-205): the hemisphere the reflection rays are drawn from
        const double area2 = len(n);
        const double emax = std::max(len(sub(p1, p0)), std::max(len(sub(p2, p0)), len(sub(p2, p1))));
        if (!(emax > 0.0) || !unit(n)) return;
        const double hgt = area2 / emax;                     // the triangle's smallest height
        if (!(hgt > 1e-3 * emax)) return;                    // degenerate or a sliver: everything is traced
        // the reference's hit point is a rounded f32 point: it may sit off the plane by a few ulps of its coordinates, and the line of a ray that rises at
        // min_cos crosses the plane that much / min_cos away from it.  Half of the guard's barycentric margin must cover that.
        double amax = 0.0;
        for (int k = 0; k < 9; ++k) amax = std::max(amax, std::fabs((double)v[k]));
        const double slop = 4.0 * std::ldexp(amax, -23) / min_cos;
        const double bm = 0.5 * (double)kReflBary;
        if (!(slop < 0.5 * bm * hgt)) return;
        const V3 tp[3] = { add(mul(p0, 1.0 - 2.0 * bm), mul(add(p1, p2), bm)), add(mul(p1, 1.0 - 2.0 * bm), mul(add(p0, p2), bm)), add(mul(p2, 1.0 - 2.0 * bm), mul(add(p0, p1), bm)) };
        const V3 ct = mul(add(p0, add(p1, p2)), 1.0 / 3.0);
        const double rt = std::max(len(sub(tp[0], ct)), std::max(len(sub(tp[1], ct)), len(sub(tp[2], ct))));
        // bins whose every direction rises by the minimum cosine (a bin is the conic hull of its corners: the minimum over it is at a corner)
        for (uint32_t g = 0; g < 24u; ++g) clear[g].clear();
        nclear = 0; normal = n;
        for (uint32_t b = 0; b < nbits; ++b) {
            bool up = true;
            for (int k = 0; k < 4; ++k) if (!(dot(n, bins[b].corner[k]) >= min_cos + 2.0 * pad_angle)) { up = false; break; }
            if (up) { clear[group_of(b)].push_back((uint16_t)b); ++nclear; row[b >> 5] &= ~(1u << (b & 31u)); }
        }
        // the triangle's own test puts the ray's crossing of the plane at t = -height / rise, with an error of a few ulps of |bo - v0| <= emax, divided by the
        // rise and by the sine of the angle between the edges (>= hgt / emax): the crossing stays behind the origin while the height exceeds that
        hmin = (float)(kReflHeightUlps * std::ldexp(emax, -24) * (emax / hgt));
        if (!(hmin > 0.0f)) return;                          // (all bits are cleared above only for bins in `clear`; with no margin the guard never holds)
        std::memcpy(&row[mask_words + 3], &hmin, 4);
        int32_t stack[128]; int sp = 0;
        stack[sp++] = 0;
        while (sp > 0 && nclear != 0u) {
            const Node& nd = tree.nodes[(size_t)stack[--sp]];
            ++work;
            // the whole box at or below T's plane: nothing in it is met by a rising ray
            const V3 rel = sub(nd.c, p0);
            if (dot(n, rel) + std::fabs(n.x) * nd.h.x + std::fabs(n.y) * nd.h.y + std::fabs(n.z) * nd.h.z <= 0.0) continue;
            V3 d = sub(nd.c, ct);
            const double dist = len(d), R = nd.r + rt + pad;
            bool far = false;
            if (dist > R * 1.0000001 && unit(d)) {
                // every direction from a point of T to a point of the (padded) box lies in the cap of half-angle asin(R / dist) around d, widened by the pad
                const double s0 = R / dist, c0 = std::sqrt(std::max(0.0, 1.0 - s0 * s0));
                const double cp = std::cos(pad_angle), sp_ = sin_pad;
                const double ch = c0 * cp - s0 * sp_, sh = s0 * cp + c0 * sp_;
                cap_touch(d, ch, sh);
                if (touched.empty()) continue;
                far = s0 < 0.12;
            }
            if (far) {
                cand.assign(touched.begin(), touched.end());
                set_bins(cand, row);
            } else if (nd.left < 0) {
                for (uint32_t k = 0; k < nd.count && nclear != 0u; ++k) {
                    const uint32_t u = tree.order[nd.first + k];
                    if (u != t) exact(tp, n, verts + 9 * (size_t)u, row);
                }
            } else if (sp + 2 <= 128) {
                // the nearer child last: it is walked first, and a triangle in a pit is finished early
                const Node& l = tree.nodes[(size_t)nd.left]; const Node& r = tree.nodes[(size_t)nd.right];
                const bool l_near = len(sub(l.c, ct)) <= len(sub(r.c, ct));
                stack[sp++] = l_near ? nd.right : nd.left; stack[sp++] = l_near ? nd.left : nd.right;
            } else {
                all_clear();
                cand.assign(touched.begin(), touched.end());
                set_bins(cand, row);
            }
        }
    }
};

}  // namespace

bool build_reflect_mask(const float* tri_verts, uint32_t ntri, double pad, uint32_t B, uint64_t work_budget, ReflMask& out, double min_cos, double pad_angle)
{
    out = ReflMask{};
    if (ntri == 0 || B < 4 || B > 16 || (6u * B * B) % 128u != 0u || !(pad >= 0.0) || !(min_cos > 0.0 && min_cos < 1.0) || !(pad_angle >= 0.0 && pad_angle < 0.1)) return false;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t stride = refl_mask_stride(B);
    std::vector<Bin> bins, groups; make_bins(B, bins); make_bins(2, groups);
    Tree tree; tree.verts = tri_verts; tree.order.resize(ntri);
    for (uint32_t i = 0; i < ntri; ++i) tree.order[i] = i;
    tree.nodes.reserve((size_t)ntri);
    tree.build(0, ntri);
    std::vector<uint32_t> words((size_t)ntri * stride);
    std::atomic<uint32_t> next{ 0 };
    std::atomic<uint64_t> work{ 0 }, exacts{ 0 };
    std::atomic<bool> over{ false };
    auto worker = [&]() {
        Walker w(bins, groups, B, tree, tri_verts, pad, min_cos, pad_angle);
        for (;;) {
            const uint32_t first = next.fetch_add(64u);
            if (first >= ntri || over.load()) break;
            for (uint32_t t = first; t < std::min(first + 64u, ntri); ++t) w.triangle(t, &words[(size_t)t * stride], stride);
            if (work.fetch_add(w.work) + w.work > work_budget) over.store(true);
            w.work = 0;
            exacts.fetch_add(w.exacts); w.exacts = 0;
        }
    };
    const uint32_t nthreads = std::max(1u, std::min({ 16u, std::thread::hardware_concurrency(), (ntri + 255u) / 256u }));
    std::vector<std::thread> pool;
    for (uint32_t i = 1; i < nthreads; ++i) pool.emplace_back(worker);
    worker();
    for (std::thread& th : pool) th.join();
    out.work = work.load(); out.exact_tests = exacts.load();
    out.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (over.load()) return false;
    uint64_t clear_bits = 0;
    for (uint32_t t = 0; t < ntri; ++t) for (uint32_t k = 0; k < stride - kReflGuardWords; ++k) clear_bits += 32u - (uint32_t)__builtin_popcount(words[(size_t)t * stride + k]);
    out.bins = B; out.stride = stride; out.words.swap(words); out.clear_bits = clear_bits;
    return true;
}

}  // namespace mi355rt
