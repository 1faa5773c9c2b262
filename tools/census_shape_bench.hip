// Microbenchmark: what the shape of the mesh census' 64-bit integer atomics costs on MI355X.  Three kernels over the same
// synthetic face_idx image (1920 x 1080, runs of geometric length with mean L, every run a random face of F = 1 M) and a random target:
//   packed    the product's kernel (csrc/mesh_census.hip, included as it stands): runs combined in the wavefront, FOUR LANES PER RUN, so a
//             run's 32-byte row is one segment of one atomic wave-instruction
//   per-head  the same run combining, but the run's head lane issues the four adds itself: four wave-instructions, 8 bytes per row each
//   per-pixel no combining: every counted pixel adds its four words
// Every variant must leave the accumulator of a host loop, bit for bit; the times are medians of 10 blocks x 20 launches (device events).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Itriangle-splatting_amd/csrc tools/census_shape_bench.hip -o tools/bin/census_shape_bench
#include "../triangle-splatting_amd/csrc/mesh_census.hip"
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

namespace
{
__global__ void __launch_bounds__(256) census_per_head(size_t npix, int F, const int32_t *__restrict__ face_idx, const float *__restrict__ target,
                                                       unsigned long long *census)
{
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    int32_t key = -1;
    uint32_t r = 0, g = 0, b = 0;
    if (p < npix)
    {
        const int32_t f = face_idx[p];
        if ((uint32_t)f < (uint32_t)F)
        {
            key = f;
            r = census_q16(target[p]); g = census_q16(target[npix + p]); b = census_q16(target[2 * npix + p]);
        }
    }
    const int32_t left = __shfl_up(key, 1);
    const bool head = lane == 0 || left != key;
    const uint64_t heads = __ballot(head);
    const uint64_t after = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = after ? lane + 1 + __builtin_ctzll(after) : 64;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const uint32_t tr = __shfl_down(r, d), tg = __shfl_down(g, d), tb = __shfl_down(b, d);
        if (lane + d < end) { r += tr; g += tg; b += tb; }
    }
    if (head && key >= 0)
    {
        unsigned long long *row = census + 4 * (size_t)key;
        __hip_atomic_fetch_add(row, (unsigned long long)(end - lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (r) __hip_atomic_fetch_add(row + 1, (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g) __hip_atomic_fetch_add(row + 2, (unsigned long long)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b) __hip_atomic_fetch_add(row + 3, (unsigned long long)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(256) census_per_pixel(size_t npix, int F, const int32_t *__restrict__ face_idx, const float *__restrict__ target,
                                                        unsigned long long *census)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int32_t f = face_idx[p];
    if ((uint32_t)f >= (uint32_t)F) return;
    unsigned long long *row = census + 4 * (size_t)f;
    const uint32_t r = census_q16(target[p]), g = census_q16(target[npix + p]), b = census_q16(target[2 * npix + p]);
    __hip_atomic_fetch_add(row, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r) __hip_atomic_fetch_add(row + 1, (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g) __hip_atomic_fetch_add(row + 2, (unsigned long long)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b) __hip_atomic_fetch_add(row + 3, (unsigned long long)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
} // namespace

int main()
{
    const int W = 1920, H = 1080, F = 1000000, BLOCKS = 10, ITERS = 20;
    const size_t npix = (size_t)W * H;
    std::mt19937_64 rng(42);
    std::vector<float> target(3 * npix);
    for (auto &v : target) v = (float)(rng() >> 40) / 16777216.0f;
    int32_t *d_idx; float *d_target; unsigned long long *d_acc;
    CK(hipMalloc(&d_idx, npix * 4)); CK(hipMalloc(&d_target, 3 * npix * 4)); CK(hipMalloc(&d_acc, (size_t)F * 32));
    CK(hipMemcpy(d_target, target.data(), 3 * npix * 4, hipMemcpyHostToDevice));
    hipEvent_t ea, eb;
    CK(hipEventCreate(&ea)); CK(hipEventCreate(&eb));
    const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
    printf("census atomics, %d x %d pixels, F = %d rows of 32 bytes, 64-bit integer adds, agent scope, no return\n", W, H, F);
    printf("%8s %10s | %-10s %9s %14s %12s\n", "mean run", "wave runs", "variant", "ms", "row updates/us", "GB/s added");
    for (const double L : {1.0, 1.76, 4.0, 16.0, 64.0})
    {
        std::vector<int32_t> idx(npix);
        std::geometric_distribution<int> extra(1.0 / L);
        for (size_t p = 0; p < npix;)
        {
            const int32_t f = (int32_t)(rng() % F);
            const size_t n = 1 + (L > 1.0 ? (size_t)extra(rng) : 0);
            for (size_t k = 0; k < n && p < npix; k++) idx[p++] = f;
        }
        std::vector<unsigned long long> want((size_t)F * 4, 0ull), got((size_t)F * 4);
        size_t runs = 0;
        for (size_t p = 0; p < npix; p++)
        {
            unsigned long long *row = want.data() + 4 * (size_t)idx[p];
            row[0] += 1;
            for (int c = 0; c < 3; c++) row[1 + c] += (unsigned long long)rintf(target[c * npix + p] * 65536.0f);
            runs += (p % 64 == 0 || idx[p] != idx[p - 1]);
        }
        CK(hipMemcpy(d_idx, idx.data(), npix * 4, hipMemcpyHostToDevice));
        for (int variant = 0; variant < 3; variant++)
        {
            auto launch = [&]() {
                if (variant == 0) ts_launch_mesh_census(W, H, F, d_idx, d_target, nullptr, d_acc, 0);
                else if (variant == 1) hipLaunchKernelGGL(census_per_head, grid, block, 0, 0, npix, F, d_idx, d_target, d_acc);
                else hipLaunchKernelGGL(census_per_pixel, grid, block, 0, 0, npix, F, d_idx, d_target, d_acc);
            };
            CK(hipMemset(d_acc, 0, (size_t)F * 32));
            launch();
            CK(hipMemcpy(got.data(), d_acc, (size_t)F * 32, hipMemcpyDeviceToHost));
            if (got != want) { printf("variant %d at L = %g: the accumulator differs from the host loop\n", variant, L); return 1; }
            for (int i = 0; i < ITERS; i++) launch();
            std::vector<float> ms(BLOCKS);
            for (int bk = 0; bk < BLOCKS; bk++)
            {
                CK(hipEventRecord(ea));
                for (int i = 0; i < ITERS; i++) launch();
                CK(hipEventRecord(eb));
                CK(hipEventSynchronize(eb));
                CK(hipEventElapsedTime(&ms[bk], ea, eb));
                ms[bk] /= ITERS;
            }
            std::sort(ms.begin(), ms.end());
            const double med = 0.5 * (ms[BLOCKS / 2 - 1] + ms[BLOCKS / 2]);
            const double updates = variant == 2 ? (double)npix : (double)runs;
            printf("%8.2f %10zu | %-10s %9.4f %14.1f %12.1f   (blocks %.4f - %.4f)\n", L, runs, variant == 0 ? "packed" : variant == 1 ? "per-head" : "per-pixel",
                   med, updates / med / 1e3, updates * 32.0 / med / 1e6, ms.front(), ms.back());
        }
    }
    CK(hipGetLastError());
    return 0;
}
