// variants_check — csrc/variants.hpp and the feed vocabulary of csrc/device_types.hpp with a recorder in place of the launch, for a build with
// -fsanitize=address,undefined: every run-time combination the launchers accept (and some they refuse) is walked, and the tag each reaches is held to
// the table of the variant sets — 16 trace_kernel, 7 trace_octree_kernel, 16 shade_kernel, 24 resolve_kernel, 4 fused_pass_kernel, 4 film_merge_kernel,
// 2 light_films_merge_kernel — and to the refusals.  Host code only: nothing here touches a device, and no HIP library is linked.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/variants_check.cpp -o variants_check
#include <array>
#include <cstdio>
#include <set>
#include "../raytracer-rs_amd/csrc/variants.hpp"

using namespace mi355rt;
using Tag = std::array<uint32_t, 4>;
static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } } while (0)

static_assert(kFeedCamera == 0u && kFeedRays == 1u && kFeedLensThin == 2u && kFeedLensOrtho == 3u && kFeedLensThinMasked == 4u && kFeedLensOrthoMasked == 5u, "the kernels' mangled names hold these numbers");
static_assert(kRaysOfPixels == 1u && kRaysFree == 2u && kRaysOfLens == 3u, "DPass travels to the device by value");
static_assert(lens_feed(kLensPinhole, false) == kFeedCamera && lens_feed(kLensPinhole, true) == kFeedCamera, "the pinhole camera honours a mask itself");
static_assert(lens_feed(kLensThin, false) == kFeedLensThin && lens_feed(kLensThin, true) == kFeedLensThinMasked, "thin lens");
static_assert(lens_feed(kLensOrtho, false) == kFeedLensOrtho && lens_feed(kLensOrtho, true) == kFeedLensOrthoMasked, "orthographic lens");
static_assert(kFeedLens<kFeedLensThin> && kFeedLens<kFeedLensOrthoMasked> && !kFeedLens<kFeedRays> && !kFeedLens<kFeedCamera>, "kFeedLens");
static_assert(kFeedThin<kFeedLensThin> && kFeedThin<kFeedLensThinMasked> && !kFeedThin<kFeedLensOrtho> && !kFeedThin<kFeedLensOrthoMasked>, "kFeedThin");
static_assert(kFeedMasked<kFeedCamera> && kFeedMasked<kFeedLensThinMasked> && kFeedMasked<kFeedLensOrthoMasked> && !kFeedMasked<kFeedRays> && !kFeedMasked<kFeedLensThin> && !kFeedMasked<kFeedLensOrtho>, "kFeedMasked");

int main()
{
    const uint32_t kFeeds = kFeedLensOrthoMasked + 1u;
    {   // trace_kernel<PRIMARY, COUNT, CONFIRM, RAYS>
        std::set<Tag> seen;
        for (int primary = 0; primary < 2; ++primary) for (int count = 0; count < 2; ++count) for (int confirm = 0; confirm < 2; ++confirm) for (uint32_t rays = 0; rays < kFeeds + 3u; ++rays) {
            int calls = 0; Tag got{};
            const hipError_t e = select_trace(primary, count, confirm, rays, [&](auto P, auto C, auto F, auto R) { ++calls; got = Tag{ P(), C(), F(), R() }; return hipSuccess; });
            if ((rays && !primary) || rays >= kFeeds) { CHECK(e == hipErrorInvalidValue && calls == 0); continue; }
            CHECK(e == hipSuccess && calls == 1);
            CHECK(got == (primary ? Tag{ 1u, (uint32_t)count, 1u, rays } : Tag{ 0u, (uint32_t)count, (uint32_t)confirm, kFeedCamera }));
            seen.insert(got);
        }
        CHECK(seen.size() == 16);
    }
    {   // trace_octree_kernel<PRIMARY, RAYS>
        std::set<Tag> seen;
        for (int primary = 0; primary < 2; ++primary) for (uint32_t rays = 0; rays < kFeeds + 3u; ++rays) {
            int calls = 0; Tag got{};
            const hipError_t e = select_trace_octree(primary, rays, [&](auto P, auto R) { ++calls; got = Tag{ P(), R(), 0u, 0u }; return hipSuccess; });
            if ((rays && !primary) || rays >= kFeeds) { CHECK(e == hipErrorInvalidValue && calls == 0); continue; }
            CHECK(e == hipSuccess && calls == 1 && got == (Tag{ (uint32_t)primary, rays, 0u, 0u }));
            seen.insert(got);
        }
        CHECK(seen.size() == 7);
    }
    {   // shade_kernel<PRIMARY, WALK, RASTER, RAYS>
        std::set<Tag> seen;
        for (int primary = 0; primary < 2; ++primary) for (int walk = 0; walk < 2; ++walk) for (int raster = 0; raster < 2; ++raster) for (uint32_t rays = 0; rays < kFeeds + 3u; ++rays) {
            int calls = 0; Tag got{};
            const hipError_t e = select_shade(primary, walk, raster, rays, [&](auto P, auto W, auto T, auto R) { ++calls; got = Tag{ P(), W(), T(), R() }; return hipSuccess; });
            if ((rays && (!primary || raster)) || rays >= kFeeds) { CHECK(e == hipErrorInvalidValue && calls == 0); continue; }
            CHECK(e == hipSuccess && calls == 1);
            CHECK(got == (primary ? Tag{ 1u, (uint32_t)walk, (uint32_t)raster, rays } : Tag{ 0u, (uint32_t)walk, 0u, kFeedCamera }));     // the later rounds have no tile bins: raster is not looked at
            seen.insert(got);
        }
        CHECK(seen.size() == 16);
    }
    {   // resolve_kernel<LANES, ., DIRECT, FLAT, LIGHTS>
        std::set<Tag> seen;
        for (uint32_t lanes = 0; lanes < 10u; ++lanes) for (int direct = 0; direct < 2; ++direct) for (int flat = 0; flat < 2; ++flat) for (uint32_t films = 0; films < kMaxLightFilms + 3u; ++films) {
            int calls = 0; Tag got{};
            const hipError_t e = select_resolve(lanes, direct, flat, films, [&](auto N, auto D, auto FL, auto L) { ++calls; got = Tag{ N(), D(), FL(), L() }; return hipSuccess; });
            if (films > kMaxLightFilms || (lanes != 2u && lanes != 4u && lanes != 8u)) { CHECK(e == hipErrorInvalidValue && calls == 0); continue; }
            CHECK(e == hipSuccess && calls == 1 && got == (Tag{ lanes, (uint32_t)direct, (uint32_t)flat, films ? 1u : 0u }));
            seen.insert(got);
        }
        CHECK(seen.size() == 24);
    }
    {   // fused_pass_kernel<CONFIRM, DIRECT> and film_merge_kernel<ADD, DIRECT> (two with_bool, as their launchers nest them), light_films_merge_kernel<ADD> (one)
        std::set<Tag> two, one;
        for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) {
            Tag got{ 9u, 9u, 0u, 0u };
            CHECK(with_bool(a, [&](auto A) { return with_bool(b, [&](auto B) { got = Tag{ A(), B(), 0u, 0u }; return hipSuccess; }); }) == hipSuccess);
            CHECK(got == (Tag{ (uint32_t)a, (uint32_t)b, 0u, 0u }));
            two.insert(got);
        }
        for (int a = 0; a < 2; ++a) CHECK(with_bool(a, [&](auto A) { one.insert(Tag{ A(), 0u, 0u, 0u }); return A() == (bool)a ? hipSuccess : hipErrorUnknown; }) == hipSuccess);
        CHECK(two.size() == 4 && one.size() == 2);
        CHECK(with_bool(true, [](auto) { return hipErrorOutOfMemory; }) == hipErrorOutOfMemory);       // the launch's error is the launcher's
    }
    std::printf(g_failed ? "variants_check: %d checks failed\n" : "variants_check: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
