// staging_check — csrc/staging.hpp against a HIP shim in host memory, for a build with -fsanitize=address,undefined: every "device" allocation is a malloc
// of exactly the bytes asked for, so a copy that overruns a temporary or the caller's array, a temporary that is never freed and one that is used after the
// Staging object is gone are all findings of the sanitizer.  Host code only: nothing here touches a device, and no HIP library is linked.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/staging_check.cpp -o staging_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../raytracer-rs_amd/csrc/staging.hpp"

// ---- the shim: the six runtime calls DeviceBuffer and Staging make
static int g_fail_allocs = 0;            // the next allocations fail with hipErrorOutOfMemory
static int g_uploads = 0, g_downloads = 0;
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes)
{
    if (g_fail_allocs > 0) { --g_fail_allocs; *p = nullptr; return hipErrorOutOfMemory; }
    *p = bytes ? std::malloc(bytes) : nullptr;
    if (*p) std::memset(*p, 0xCD, bytes);
    return hipSuccess;
}
hipError_t hipFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
hipError_t hipHostFree(void* p) { return hipFree(p); }
hipError_t hipMemset(void* p, int v, size_t bytes) { std::memset(p, v, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    ++(kind == hipMemcpyHostToDevice ? g_uploads : g_downloads);
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
}

using mi355rt::Staging;
static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } } while (0)

int main()
{
    const size_t n = 70;
    std::vector<float> rays(6 * n, 1.5f), tuv(3 * n, -7.0f), rgb(3 * n, 0.0f);
    std::vector<uint32_t> prim(n, 9u), ids(n, 0u);
    size_t counter = 0;

    {   // host memory: inputs go up, outputs come back, the preloaded one keeps what the "kernel" leaves alone
        Staging st(nullptr, &counter, false);
        const float* d_rays = st.in(rays.data(), 6 * n);
        const uint32_t* d_keys = st.in((const uint32_t*)nullptr, 2 * n);
        const float* d_none = st.in(rays.data(), 0);
        const float* d_dummy = st.in(rays.data(), 0, true);
        const float* d_dummy_null = st.in((const float*)nullptr, 6 * n, true);
        float* d_rgb = st.out(rgb.data(), 3 * n);
        float* d_tuv = st.out(tuv.data(), 3 * n, true);
        uint32_t* d_prim = st.out(prim.data(), n);
        float* d_absent = st.out((float*)nullptr, 3 * n);
        float* d_empty = st.out(rgb.data(), 0);
        CHECK(st.error() == hipSuccess);
        CHECK(d_rays && d_rays != rays.data() && d_rays[6 * n - 1] == 1.5f);
        CHECK(!d_keys && !d_none && !d_absent && !d_empty);
        CHECK(d_dummy && d_dummy_null);
        CHECK(d_tuv && d_tuv[0] == -7.0f && d_tuv[3 * n - 1] == -7.0f);
        CHECK(g_uploads == 2);                                          // the rays and the preloaded tuv: a dummy uploads nothing
        CHECK(counter == 6 * n * 4 + 4 + 4 + 3 * n * 4 + 3 * n * 4 + n * 4);
        for (size_t i = 0; i < 3 * n; ++i) d_rgb[i] = (float)i;
        for (size_t i = 0; i < n; ++i) d_prim[i] = (uint32_t)i;
        d_tuv[3] = 2.0f;                                                // one "hit"
        CHECK(rgb[5] == 0.0f);                                          // nothing reaches the caller before download()
        CHECK(st.download() == hipSuccess);
        CHECK(g_downloads == 3);
        CHECK(rgb[5] == 5.0f && rgb[3 * n - 1] == (float)(3 * n - 1) && prim[n - 1] == n - 1);
        CHECK(tuv[3] == 2.0f && tuv[0] == -7.0f && tuv[3 * n - 1] == -7.0f);
        CHECK(counter != 0);                                            // the temporaries live until the object goes: behind the call's wait
    }
    CHECK(counter == 0);

    {   // scratch on host memory, and a prefix download
        g_uploads = g_downloads = 0;
        std::vector<uint32_t> owner(n, 1u);
        std::vector<float> bary(2 * n, -3.0f), points(3 * n, -1.0f);
        Staging st(nullptr, &counter, false);
        uint32_t* d_owner = st.scratch(owner.data(), n);
        uint32_t* d_private = st.scratch((uint32_t*)nullptr, n);
        float* d_bary = st.scratch(bary.data(), 2 * n, true);
        uint32_t* d_ids = st.out(ids.data(), n);
        float* d_points = st.out(points.data(), 3 * n);
        CHECK(st.error() == hipSuccess && d_owner && d_private && d_bary && d_ids && d_points);
        CHECK(g_uploads == 1 && d_bary[2 * n - 1] == -3.0f);
        for (size_t i = 0; i < n; ++i) { d_owner[i] = 5u; d_private[i] = 6u; d_ids[i] = 7u; }
        for (size_t i = 0; i < 3 * n; ++i) d_points[i] = 8.0f;
        st.only(ids.data(), 3); st.only(points.data(), 9);
        st.only((float*)nullptr, 0); st.only(rays.data(), 0);           // absent and never staged: nothing to do
        CHECK(st.download() == hipSuccess);
        CHECK(g_downloads == 4);                                        // owner, bary, ids, points: not the private scratch
        CHECK(owner[n - 1] == 5u && ids[2] == 7u && ids[3] == 0u && points[8] == 8.0f && points[9] == -1.0f);
        st.only(ids.data(), 0);
        CHECK(st.download() == hipSuccess && g_downloads == 4);         // a second download has nothing left
    }
    CHECK(counter == 0);

    {   // an output trimmed to nothing is not copied
        g_downloads = 0;
        Staging st(nullptr, &counter, false);
        float* d = st.out(rgb.data(), 3 * n);
        d[0] = 123.0f;
        st.only(rgb.data(), 0);
        CHECK(st.download() == hipSuccess && g_downloads == 0 && rgb[0] == 0.0f);
    }

    {   // device memory: the caller's pointers as they are, a temporary only for the scratch the caller left out
        g_uploads = g_downloads = 0;
        Staging st(nullptr, &counter, true);
        CHECK(st.in(rays.data(), 6 * n) == rays.data());
        CHECK(st.in((const float*)nullptr, 0, true) == nullptr);
        CHECK(st.out(rgb.data(), 3 * n) == rgb.data() && st.out(tuv.data(), 3 * n, true) == tuv.data());
        CHECK(st.out((float*)nullptr, 3 * n) == nullptr);
        CHECK(st.scratch(prim.data(), n) == prim.data());
        CHECK(counter == 0);
        uint32_t* d_private = st.scratch((uint32_t*)nullptr, n);
        CHECK(d_private && counter == n * 4);
        d_private[n - 1] = 1u;
        st.only(rgb.data(), 1);
        CHECK(st.download() == hipSuccess && st.error() == hipSuccess);
        CHECK(g_uploads == 0 && g_downloads == 0);
    }
    CHECK(counter == 0);

    {   // the first error sticks: nothing is queued behind it, and what was allocated before it is still given back
        g_uploads = g_downloads = 0;
        Staging st(nullptr, &counter, false);
        const float* ok = st.in(rays.data(), 6 * n);
        g_fail_allocs = 1;
        float* bad = st.out(rgb.data(), 3 * n, true);
        float* after = st.out(tuv.data(), 3 * n, true);
        const float* after_in = st.in(rays.data(), 6 * n, true);
        CHECK(ok && !bad && !after && !after_in);
        CHECK(st.error() == hipErrorOutOfMemory && st.download() == hipErrorOutOfMemory);
        CHECK(g_uploads == 1 && g_downloads == 0 && counter == 6 * n * 4);
    }
    CHECK(counter == 0);

    std::printf(g_failed ? "staging_check: %d checks failed\n" : "staging_check: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
