// probes_place.hip — the device side of probe placement (include/mi355rt.h, "PROBE PLACEMENT"): the survey of a gather chunk's closest hits
// (mi355rt_probes_survey), the move and the state of every surveyed probe (mi355rt_probes_place), and the visibility-weighted lookup of a grid whose probes
// have moved (mi355rt_probes_lookup_placed).  The arithmetic is csrc/probe_place.hpp, the statement raytracer-rs_amd/probes.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "probes_place.hpp"
#include "probe_place.hpp"

namespace mi355rt {
namespace {
constexpr int kPlaceBlock = 256;
constexpr uint32_t kPlaceMiss = 0xFFFFFFFFu;    // prim of a ray that hit nothing, as intersect_kernel writes it

__device__ __forceinline__ SurveyRecord load_record(const float* a, size_t o) { const float4 v = reinterpret_cast<const float4*>(a)[o]; return SurveyRecord{ v.x, v.y, v.z, v.w }; }
__device__ __forceinline__ void store_record(float* a, size_t o, const SurveyRecord& r) { reinterpret_cast<float4*>(a)[o] = make_float4(r.dist, r.x, r.y, r.z); }
}  // namespace

// One lane per probe walks the chunk's samples of its point in sample order, the state in registers (15 words), loaded and stored once per chunk: the order of
// the statement is the order of the loop, and a tie keeps the earlier sample without a word about it.  Entry s * cp + i: the lanes of a wave read consecutive
// 24-byte ray rows, 12-byte tuv rows and prim words, so every cache line fetched is used whole; the normal of the hit triangle is the one scattered read.
// None of the loads depends on the state, so the compiler is free to issue the next samples' while this one is compared (unroll 4).
__global__ __launch_bounds__(kPlaceBlock) void probes_survey_kernel(uint32_t point0, uint32_t cp, uint32_t cs, int fresh, int flip, float max_distance, uint32_t ntri,
                                                                   const float* __restrict__ rays6, const float* __restrict__ tuv, const uint32_t* __restrict__ prim,
                                                                   const float4* __restrict__ normals, uint32_t* out_n, uint32_t* out_back, uint32_t* out_front,
                                                                   float* out_near_back, float* out_near_front, float* out_far)
{
    const uint32_t i = blockIdx.x * kPlaceBlock + threadIdx.x;
    if (i >= cp) return;
    const size_t o = (size_t)point0 + i;
    SurveyState st = survey_empty();
    if (!fresh) {
        st.n = out_n[o]; st.back = out_back[o]; st.front = out_front[o];
        st.near_back = load_record(out_near_back, o); st.near_front = load_record(out_near_front, o); st.far = load_record(out_far, o);
    }
#pragma unroll 4
    for (uint32_t s = 0; s < cs; ++s) {
        const size_t e = (size_t)s * cp + i;
        const uint32_t p = prim[e];
        const bool found = p != kPlaceMiss && p < ntri;               // an index the scene does not have is never used as one
        const float t = found ? tuv[3 * e] : 0.0f;
        survey_sample(st, found, t, rays6[6 * e + 3], rays6[6 * e + 4], rays6[6 * e + 5],
                      [&](float& nx, float& ny, float& nz) { const float4 nq = normals[p]; nx = nq.x; ny = nq.y; nz = nq.z; }, flip != 0, max_distance);
    }
    out_n[o] = st.n; out_back[o] = st.back; out_front[o] = st.front;
    store_record(out_near_back, o, st.near_back); store_record(out_near_front, o, st.near_front); store_record(out_far, o, st.far);
}

// One lane per probe: place_one and place_state on the probe's survey.  new_offsets may be offsets itself: a lane reads its own three floats before it writes them.
__global__ __launch_bounds__(kPlaceBlock) void probes_place_kernel(ShGrid grid, PlaceConfig cfg, uint32_t nprobes, const uint32_t* __restrict__ n, const uint32_t* __restrict__ back,
                                                                  const uint32_t* __restrict__ front, const float* __restrict__ near_back, const float* __restrict__ near_front,
                                                                  const float* __restrict__ far, const float* offsets, float* new_offsets, uint8_t* __restrict__ verdict,
                                                                  uint8_t* __restrict__ state)
{
    const uint32_t i = blockIdx.x * kPlaceBlock + threadIdx.x;
    if (i >= nprobes) return;
    SurveyState st;
    st.n = n[i]; st.back = back[i]; st.front = front[i];
    st.near_back = load_record(near_back, i); st.near_front = load_record(near_front, i); st.far = load_record(far, i);
    if (state != nullptr) state[i] = (uint8_t)place_state(st, cfg);
    if (new_offsets == nullptr && verdict == nullptr) return;
    float off[3] = { 0.0f, 0.0f, 0.0f }, out[3];
    if (offsets != nullptr) { off[0] = offsets[3ull * i]; off[1] = offsets[3ull * i + 1]; off[2] = offsets[3ull * i + 2]; }
    const uint32_t v = place_one(st, off, grid.spacing, grid.counts, cfg, out);
    if (new_offsets != nullptr) { new_offsets[3ull * i] = out[0]; new_offsets[3ull * i + 1] = out[1]; new_offsets[3ull * i + 2] = out[2]; }
    if (verdict != nullptr) verdict[i] = (uint8_t)v;
}

// One lane per query, as probes_lookup_vis_kernel: sh9_lookup_placed with the corner loop outside and the 27 running values in registers.  Per corner that
// computes a weight it adds three 4-byte reads of the probe's offset and three additions.
__global__ __launch_bounds__(kPlaceBlock) void probes_lookup_placed_kernel(ShGrid grid, const uint32_t* __restrict__ n, const float* __restrict__ sh, const uint8_t* __restrict__ usable,
                                                                          uint32_t R, const uint32_t* __restrict__ count, const float* __restrict__ moments,
                                                                          const float* __restrict__ offsets, uint32_t flags, float normal_bias, const float* __restrict__ points3,
                                                                          const float* __restrict__ dirs3, const float* __restrict__ normals3, uint64_t nq, uint32_t mode,
                                                                          float* __restrict__ rgb3, uint8_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * kPlaceBlock + threadIdx.x;
    if (q >= nq) return;
    const float p[3] = { points3[3 * q], points3[3 * q + 1], points3[3 * q + 2] };
    const float d[3] = { dirs3[3 * q], dirs3[3 * q + 1], dirs3[3 * q + 2] };
    float nr[3] = { 0.0f, 0.0f, 0.0f };
    if (normals3 != nullptr) { nr[0] = normals3[3 * q]; nr[1] = normals3[3 * q + 1]; nr[2] = normals3[3 * q + 2]; }
    const size_t RR = (size_t)R * R;
    float rgb[3];
    const bool used = sh9_lookup_placed(grid, [n](size_t j) { return n[j]; }, [sh](size_t j, int c) { return sh[27 * j + c]; }, usable != nullptr,
                                        [usable](size_t j) { return usable[j] != 0; }, R, [count, RR](size_t j, uint32_t k) { return count[j * RR + k]; },
                                        [moments, RR](size_t j, uint32_t k, int m) { return moments[2 * (j * RR + k) + m]; }, offsets != nullptr,
                                        [offsets](size_t j, int a) { return offsets[3 * j + a]; }, flags, normal_bias, p, d, normals3 != nullptr, nr, mode, rgb);
    rgb3[3 * q] = rgb[0]; rgb3[3 * q + 1] = rgb[1]; rgb3[3 * q + 2] = rgb[2];
    if (ok != nullptr) ok[q] = used ? 1 : 0;
}

hipError_t launch_probes_survey(hipStream_t stream, uint32_t point0, uint32_t cp, uint32_t cs, bool fresh, bool flip, float max_distance, uint32_t ntri, const float* rays6,
                                const float* tuv, const uint32_t* prim, const void* normals4, uint32_t* out_n, uint32_t* out_back, uint32_t* out_front, float* out_near_back,
                                float* out_near_front, float* out_far)
{
    if (cp == 0) return hipSuccess;
    hipLaunchKernelGGL(probes_survey_kernel, dim3((cp + kPlaceBlock - 1) / kPlaceBlock), dim3(kPlaceBlock), 0, stream, point0, cp, cs, fresh ? 1 : 0, flip ? 1 : 0, max_distance, ntri,
                       rays6, tuv, prim, static_cast<const float4*>(normals4), out_n, out_back, out_front, out_near_back, out_near_front, out_far);
    return hipGetLastError();
}

hipError_t launch_probes_place(hipStream_t stream, const ShGrid& grid, const PlaceConfig& cfg, uint32_t nprobes, const uint32_t* n, const uint32_t* back, const uint32_t* front,
                               const float* near_back, const float* near_front, const float* far, const float* offsets, float* new_offsets, uint8_t* verdict, uint8_t* state)
{
    if (nprobes == 0) return hipSuccess;
    hipLaunchKernelGGL(probes_place_kernel, dim3((nprobes + kPlaceBlock - 1) / kPlaceBlock), dim3(kPlaceBlock), 0, stream, grid, cfg, nprobes, n, back, front, near_back, near_front,
                       far, offsets, new_offsets, verdict, state);
    return hipGetLastError();
}

hipError_t launch_probes_lookup_placed(hipStream_t stream, const ShGrid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, uint32_t R, const uint32_t* count,
                                       const float* moments, const float* offsets, uint32_t flags, float normal_bias, const float* points3, const float* dirs3,
                                       const float* normals3, size_t nq, uint32_t mode, float* rgb3, uint8_t* ok)
{
    if (nq == 0) return hipSuccess;
    if ((nq + kPlaceBlock - 1) / kPlaceBlock > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probes_lookup_placed_kernel, dim3((unsigned)((nq + kPlaceBlock - 1) / kPlaceBlock)), dim3(kPlaceBlock), 0, stream, grid, n, sh, usable, R, count, moments,
                       offsets, flags, normal_bias, points3, dirs3, normals3, (uint64_t)nq, mode, rgb3, ok);
    return hipGetLastError();
}

}  // namespace mi355rt
