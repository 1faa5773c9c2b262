// knn.hip -- exact 3-NN mean squared distance and nearest-other-group search (include/ts_knn.h).
//
// Reference: submodules/simple-knn/simple_knn.cu ("SK"): bounding box (:241-254, min/max reductions seeded with the
// ORIGIN, a quirk kept here because it shapes the Morton grid and with it the tie order), 30-bit Morton codes (:49-73),
// radix sort of (code, index) (:256-266), min/max box per 1024 sorted points (:82-121, :268-271), then one thread per
// point scanning every box that can still hold a closer point (:153-235).
// Here the sorted points are gathered once into a float4 array (xyz + original index) so every later access is
// contiguous; one 256-lane workgroup owns a box (4 points per lane), scans its own box first to get a search radius,
// and then visits only boxes whose box-to-box distance is within the workgroup's current worst radius, staging each
// visited box through LDS (all lanes read the same candidate: LDS broadcast, no bank conflicts) and skipping per lane
// when the box cannot improve that lane's points.  No host synchronisation anywhere.
#include "../../include/ts_knn.h"
#include "ts_knn_front.h"

#include <cfloat>
#include <cstring>

namespace
{
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz; // SK:43-47
}

// SK:123-133
__device__ __forceinline__ float dist_box_point(const Box &b, float px, float py, float pz)
{
    float dx = 0, dy = 0, dz = 0;
    if (px < b.mnx || px > b.mxx) dx = fminf(fabsf(px - b.mnx), fabsf(px - b.mxx));
    if (py < b.mny || py > b.mxy) dy = fminf(fabsf(py - b.mny), fabsf(py - b.mxy));
    if (pz < b.mnz || pz > b.mxz) dz = fminf(fabsf(pz - b.mnz), fabsf(pz - b.mxz));
    return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ float dist_box_box(const Box &a, const Box &b)
{
    const float dx = fmaxf(0.0f, fmaxf(a.mnx - b.mxx, b.mnx - a.mxx));
    const float dy = fmaxf(0.0f, fmaxf(a.mny - b.mxy, b.mny - a.mxy));
    const float dz = fmaxf(0.0f, fmaxf(a.mnz - b.mxz, b.mnz - a.mxz));
    return dx * dx + dy * dy + dz * dz;
}

// K = 3: mean squared distance to the 3 nearest others.  K = 1: nearest point of another group.
template <int K>
__global__ void __launch_bounds__(TPB) search_kernel(int P, int nboxes, int group, const float4 *__restrict__ sp,
                                                      const Box *__restrict__ boxes, float *__restrict__ out_mean,
                                                      uint32_t *__restrict__ out_nearest)
{
    __shared__ float4 cand[BOX];
    __shared__ uint32_t cand_group[K == 1 ? BOX : 1]; // group id of every staged candidate (one division per candidate per box)
    __shared__ float red[TPB / 64];
    const int mybox = blockIdx.x, tid = threadIdx.x;
    const Box bme = boxes[mybox];

    float px[PPT], py[PPT], pz[PPT], best[PPT][K];
    uint32_t pid[PPT], bestpos[PPT], bestid[PPT], mygroup[PPT];
    bool have[PPT];
#pragma unroll
    for (int q = 0; q < PPT; q++)
    {
        const int i = mybox * BOX + q * TPB + tid;
        have[q] = i < P;
        const float4 p = have[q] ? sp[i] : make_float4(0, 0, 0, 0);
        px[q] = p.x; py[q] = p.y; pz[q] = p.z; pid[q] = __float_as_uint(p.w);
        bestpos[q] = 0xFFFFFFFFu; bestid[q] = pid[q];
        mygroup[q] = pid[q] / (uint32_t)group;
#pragma unroll
        for (int k = 0; k < K; k++) best[q][k] = FLT_MAX;
    }

    auto scan_box = [&](int b) {
        const int n = min(BOX, P - b * BOX);
        __syncthreads(); // previous users of `cand` are done
        for (int i = tid; i < n; i += TPB)
        {
            const float4 c = sp[(size_t)b * BOX + i];
            cand[i] = c;
            if (K == 1) cand_group[i] = __float_as_uint(c.w) / (uint32_t)group;
        }
        __syncthreads();
        const Box bb = boxes[b];
#pragma unroll
        for (int q = 0; q < PPT; q++)
        {
            if (!have[q]) continue;
            if (dist_box_point(bb, px[q], py[q], pz[q]) > best[q][K - 1]) continue; // SK:174-175, 221-222
            const int self = (b == mybox) ? q * TPB + tid : -1;
            for (int i = 0; i < n; i++)
            {
                const float4 c = cand[i];
                const float d = dist2(px[q], py[q], pz[q], c.x, c.y, c.z);
                if (K == 3)
                {
                    if (i == self) continue; // SK:179-180: the point itself (by sorted position), duplicates count
                    float dd = d;            // SK:136-149
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (best[q][k] > dd) { const float t = best[q][k]; best[q][k] = dd; dd = t; }
                }
                else
                {
                    const uint32_t cid = __float_as_uint(c.w);
                    if (cand_group[i] == mygroup[q]) continue; // SK:226-227
                    const uint32_t pos = (uint32_t)(b * BOX + i);
                    if (d < best[q][0] || (d == best[q][0] && pos < bestpos[q])) // first in sorted order wins ties (SK:229)
                    {
                        best[q][0] = d; bestpos[q] = pos; bestid[q] = cid;
                    }
                }
            }
        }
    };

    scan_box(mybox);
    float worst = 0.0f; // this lane's largest current search radius
#pragma unroll
    for (int q = 0; q < PPT; q++)
        if (have[q]) worst = fmaxf(worst, best[q][K - 1]);
    float radius = block_reduce(worst, red, true);
    for (int b = 0; b < nboxes; b++)
    {
        if (b == mybox) continue;
        if (dist_box_box(bme, boxes[b]) > radius) continue; // workgroup-uniform: nobody here can gain from box b
        scan_box(b);
        worst = 0.0f;
#pragma unroll
        for (int q = 0; q < PPT; q++)
            if (have[q]) worst = fmaxf(worst, best[q][K - 1]);
        radius = block_reduce(worst, red, true);
    }
#pragma unroll
    for (int q = 0; q < PPT; q++)
    {
        if (!have[q]) continue;
        if (K == 3) out_mean[pid[q]] = (best[q][0] + best[q][1] + best[q][K - 1]) / 3.0f; // SK:186
        else out_nearest[pid[q]] = bestid[q];                                               // SK:234
    }
}

} // namespace

size_t ts_knn_workspace_bytes(int P) { return knn_carve(nullptr, P).bytes + TS_ALIGN; }

hipError_t ts_knn_mean_dist3(int P, const float *points, float *mean_dist2, void *ws, hipStream_t s)
{
    if (P <= 0) return hipSuccess;
    const KnnCarve c = knn_carve(ws, P);
    hipError_t e = knn_prepare<false>(P, points, c, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(search_kernel<3>, dim3(c.nboxes), dim3(TPB), 0, s, P, c.nboxes, 1, c.sp, c.boxes, mean_dist2, (uint32_t *)nullptr);
    return hipGetLastError();
}

hipError_t ts_knn_nearest_other(int P, int group, const float *points, uint32_t *nearest, void *ws, hipStream_t s)
{
    if (P <= 0) return hipSuccess;
    const KnnCarve c = knn_carve(ws, P);
    hipError_t e = knn_prepare<false>(P, points, c, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(search_kernel<1>, dim3(c.nboxes), dim3(TPB), 0, s, P, c.nboxes, group, c.sp, c.boxes, (float *)nullptr, nearest);
    return hipGetLastError();
}
