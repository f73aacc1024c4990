// topk_select.h -- order statistics by counting over (key, id) candidates parked in LDS: shared by the ranking-metrics kernel
// (topk.hip, 32-bit keys) and the top-N list kernel (recommend.hip, 32- and 64-bit keys).
#pragma once
#include <stdint.h>

#define RTX_TOPK_MAX 1024

#ifdef __HIPCC__
// rank (0 = first) of element (k, id) among the n (key, id) pairs in LDS, ordered by key descending, id ascending among equal keys;
// n4 = ceil(n / 4): the arrays are padded to a multiple of 4 with (key 0, id INT_MAX): below every real element
__device__ __forceinline__ uint32_t topk_rank_of(const uint32_t* __restrict__ keys, const int32_t* __restrict__ ids, int n4, uint32_t k, int32_t id)
{
    uint32_t r0 = 0, r1 = 0;
    const uint4* k4 = (const uint4*)keys;
    const int4* i4 = (const int4*)ids;
    for (int i = 0; i < n4; ++i) {
        const uint4 q = k4[i];
        const int4 d = i4[i];
        r0 += (q.x > k) + ((q.x == k) & (d.x < id)) + (q.y > k) + ((q.y == k) & (d.y < id));
        r1 += (q.z > k) + ((q.z == k) & (d.z < id)) + (q.w > k) + ((q.w == k) & (d.w < id));
    }
    return r0 + r1;
}

// number of keys greater than k among the n4 * 4 keys in LDS (two instructions per key: a compare and an add-with-carry)
__device__ __forceinline__ uint32_t topk_count_gt(const uint32_t* __restrict__ keys, int n4, uint32_t k)
{
    uint32_t g0 = 0, g1 = 0;
    const uint4* k4 = (const uint4*)keys;
    for (int i = 0; i < n4; ++i) {
        const uint4 q = k4[i];
        g0 += (q.x > k) + (q.y > k);
        g1 += (q.z > k) + (q.w > k);
    }
    return g0 + g1;
}

// the same two for 64-bit keys (float64 score rows): 16 bytes = 2 keys per LDS read
__device__ __forceinline__ uint32_t topk_rank_of(const uint64_t* __restrict__ keys, const int32_t* __restrict__ ids, int n4, uint64_t k, int32_t id)
{
    uint32_t r0 = 0, r1 = 0;
    const ulonglong2* k2 = (const ulonglong2*)keys;
    const int4* i4 = (const int4*)ids;
    for (int i = 0; i < n4; ++i) {
        const ulonglong2 qa = k2[2 * i], qb = k2[2 * i + 1];
        const int4 d = i4[i];
        r0 += (qa.x > k) + ((qa.x == k) & (d.x < id)) + (qa.y > k) + ((qa.y == k) & (d.y < id));
        r1 += (qb.x > k) + ((qb.x == k) & (d.z < id)) + (qb.y > k) + ((qb.y == k) & (d.w < id));
    }
    return r0 + r1;
}

__device__ __forceinline__ uint32_t topk_count_gt(const uint64_t* __restrict__ keys, int n4, uint64_t k)
{
    uint32_t g0 = 0, g1 = 0;
    const ulonglong2* k2 = (const ulonglong2*)keys;
    for (int i = 0; i < n4; ++i) {
        const ulonglong2 qa = k2[2 * i], qb = k2[2 * i + 1];
        g0 += (qa.x > k) + (qa.y > k);
        g1 += (qb.x > k) + (qb.y > k);
    }
    return g0 + g1;
}
#endif
