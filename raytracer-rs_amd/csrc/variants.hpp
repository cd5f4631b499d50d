// variants.hpp — which instantiation of a kernel a launch takes: run-time values -> compile-time tags, and per wavefront kernel THE SET of its variants.
// Plain host C++ (kernels.hip's launchers call it with the launch as `f`; tools/variants_check.cpp with a recorder, under a sanitizer).  A tag is a
// std::integral_constant handed to a generic lambda: `[&](auto P, auto R) { launch<P(), R()>(...); }`.  The sets are no cross products — what a select_*
// does not reach is not compiled; a new feed is one constant (device_types.hpp), one arm of with_feed and the kernels' `if constexpr`.
#pragma once
#include <type_traits>
#include "kernels.hpp"

namespace mi355rt {

template <bool B> using BoolTag = std::integral_constant<bool, B>;
template <uint32_t V> using U32Tag = std::integral_constant<uint32_t, V>;
using CameraFeedTag = U32Tag<kFeedCamera>;

template <class F> hipError_t with_bool(bool b, F&& f) { return b ? f(BoolTag<true>{}) : f(BoolTag<false>{}); }
template <class F> hipError_t with_feed(uint32_t feed, F&& f)
{
    switch (feed) {
    case kFeedCamera: return f(U32Tag<kFeedCamera>{});
    case kFeedRays: return f(U32Tag<kFeedRays>{});
    case kFeedLensThin: return f(U32Tag<kFeedLensThin>{});
    case kFeedLensOrtho: return f(U32Tag<kFeedLensOrtho>{});
    case kFeedLensThinMasked: return f(U32Tag<kFeedLensThinMasked>{});
    case kFeedLensOrthoMasked: return f(U32Tag<kFeedLensOrthoMasked>{});
    default: return hipErrorInvalidValue;
    }
}
template <class F> hipError_t with_resolve_lanes(uint32_t lanes, F&& f)      // lanes per pixel: resolve_kernel's header
{
    switch (lanes) {
    case 2: return f(U32Tag<2>{});
    case 4: return f(U32Tag<4>{});
    case 8: return f(U32Tag<8>{});
    default: return hipErrorInvalidValue;
    }
}

// trace_kernel<PRIMARY, COUNT, CONFIRM, RAYS>, 16: the primary round takes the six feeds x COUNT, always as CONFIRM (primary rays are radiance rays either
// way); the later rounds CONFIRM x COUNT on the camera feed.  Only the primary round of a pass is fed.
template <class F> hipError_t select_trace(bool primary, bool count, bool confirm, uint32_t rays, F&& f)
{
    if (rays && !primary) return hipErrorInvalidValue;
    return with_bool(count, [&](auto C) {
        if (primary) return with_feed(rays, [&](auto R) { return f(BoolTag<true>{}, C, BoolTag<true>{}, R); });
        return with_bool(confirm, [&](auto X) { return f(BoolTag<false>{}, C, X, CameraFeedTag{}); });
    });
}
// trace_octree_kernel<PRIMARY, RAYS>, 7: the six feeds of the primary round, and the later rounds
template <class F> hipError_t select_trace_octree(bool primary, uint32_t rays, F&& f)
{
    if (rays && !primary) return hipErrorInvalidValue;
    if (!primary) return f(BoolTag<false>{}, CameraFeedTag{});
    return with_feed(rays, [&](auto R) { return f(BoolTag<true>{}, R); });
}
// shade_kernel<PRIMARY, WALK, RASTER, RAYS>, 16: WALK x (the six feeds of a primary round that walks the tree; the pinhole camera's primary round through
// the tile bins; the later rounds).  A ray-fed or lens primary round walks the tree: no pinhole camera, no tile bins.
template <class F> hipError_t select_shade(bool primary, bool walk, bool raster, uint32_t rays, F&& f)
{
    if (rays && (!primary || raster)) return hipErrorInvalidValue;
    return with_bool(walk, [&](auto W) {
        if (!primary) return f(BoolTag<false>{}, W, BoolTag<false>{}, CameraFeedTag{});
        if (raster) return f(BoolTag<true>{}, W, BoolTag<true>{}, CameraFeedTag{});
        return with_feed(rays, [&](auto R) { return f(BoolTag<true>{}, W, BoolTag<false>{}, R); });
    });
}
// resolve_kernel<LANES, ., DIRECT, FLAT, LIGHTS>, 24: the full 3 x 2 x 2 x 2.  light_films: the planes the pass adds to (0: none: the kernels without them)
template <class F> hipError_t select_resolve(uint32_t lanes, bool direct, bool flat, uint32_t light_films, F&& f)
{
    if (light_films > kMaxLightFilms) return hipErrorInvalidValue;       // Renderer::init refuses such a scene with the flag
    return with_resolve_lanes(lanes, [&](auto N) { return with_bool(direct, [&](auto D) { return with_bool(flat, [&](auto FL) { return with_bool(light_films != 0u, [&](auto L) {
        return f(N, D, FL, L); }); }); }); });
}

}  // namespace mi355rt
