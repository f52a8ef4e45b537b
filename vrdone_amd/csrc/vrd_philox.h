// Keep decisions of the training dropout: a pure function of (step seed, site, element id), the device side of
// vrdone_amd/dropout.py (which documents ids and sites).  Philox4x32-10 (Salmon et al., SC'11; Random123's constants): key = the
// 64-bit seed, counter = (id >> 2 as two words, site, 0), element id takes word id & 3.  keep iff word >= floor(p * 2^32).
#pragma once
#include "vrd_common.h"

namespace vrd {

struct PhiloxWords {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return PhiloxWords{{c0, c1, c2, c3}};
}

// What a dropout call passes to its kernels.  seed: one 64-bit word in device memory, written before the launch (by the step
// that drew it: a replayed graph reads the replay's value); threshold = floor(p * 2^32); scale = 1 / (1 - p) in f32
struct DropSite {
    const uint64_t* seed;
    uint32_t site, threshold;
    float scale;
};
// host: the rate as the kernels use it (p in [0, 1) checked by the caller)
inline DropSite drop_site(const uint64_t* seed, unsigned site, float p) {
    return DropSite{seed, site, (uint32_t)((double)p * 4294967296.0), 1.0f / (1.0f - p)};
}

// the four words of the ids 4 blk .. 4 blk + 3
__device__ __forceinline__ PhiloxWords drop_words(uint64_t seed, uint32_t site, uint64_t blk) {
    return philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), site, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// 1 / (1 - p) or 0: the factor of element `id`
__device__ __forceinline__ float drop_factor(uint64_t seed, const DropSite& d, uint64_t id) {
    const PhiloxWords r = drop_words(seed, d.site, id >> 2);
    const uint32_t lo = (id & 1) ? r.w[1] : r.w[0], hi = (id & 1) ? r.w[3] : r.w[2];
    return ((id & 2) ? hi : lo) >= d.threshold ? d.scale : 0.f;
}

}  // namespace vrd
