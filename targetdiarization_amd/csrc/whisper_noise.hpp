// whisper_noise.hpp — the noise of Whisper's sampled decoding, stated once for the vocabulary head (whisper.hip) and
// the test hook (diag.hip).  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"; the Random123 constants):
// a counter-based generator, so the host restates it word for word (tests/whisper_sample_oracle.py).
//   key      (seed & 0xffffffff, seed >> 32)
//   counter  (n >> 2, p, stream_lo, stream_hi): n the token id, p the context position of the id being chosen, stream the row's own
//            64-bit id; id n takes output word n & 3, so one call serves four adjacent ids
//   uniform  k = word >> 9 (23 bits), u = (k + 0.5) 2^-23: exact in fp32, inside [2^-24, 1 - 2^-24]
//   noise    g = -logf(-logf(u))  (standard Gumbel); argmax_n(v_n / T + g_n) is a draw from softmax(v / T)
// A row's noise depends on (seed, stream, p, n) alone: never on its place in a batch.
#pragma once
#include <hip/hip_runtime.h>

namespace tdx {

struct Philox4 { unsigned w[4]; };

__host__ __device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)M0 * c0, p1 = (unsigned long long)M1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += W0; k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// the four words of the ids 4 q .. 4 q + 3 at position p of the row whose stream is `stream`
__host__ __device__ __forceinline__ Philox4 wh_noise_words(unsigned long long seed, unsigned long long stream, int p, int q) {
    return philox4x32_10((unsigned)q, (unsigned)p, (unsigned)stream, (unsigned)(stream >> 32), (unsigned)seed, (unsigned)(seed >> 32));
}

__device__ __forceinline__ float wh_gumbel(unsigned word) {
    const float u = ((float)(word >> 9) + 0.5f) * 1.1920928955078125e-07f;          // 2^-23
    return -logf(-logf(u));
}

}  // namespace tdx
