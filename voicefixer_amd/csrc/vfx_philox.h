// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): the one counter-based generator of the library.  Mode 2's
// dropout masks (vfx_train.hip; voicefixer_amd/dropout.py) and the dither of the word-length reduction (vfx_wordlength.hip;
// voicefixer_amd/wordlength.py) are both documented functions of its words, so this code does not change.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = M0 * ctr.x, hi0 = __umulhi(M0, ctr.x);
        const uint32_t lo1 = M1 * ctr.z, hi1 = __umulhi(M1, ctr.z);
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += W0;
        key.y += W1;
    }
    return ctr;
}
