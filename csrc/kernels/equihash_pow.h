// Device-side block hash and target filter of the Equihash miner: the part of the mining step
// that follows the solver (reference src/miner.cpp / src/rpc/mining.cpp generateBlocks: encode
// the solution, hash the whole header, compare with the target) as HIP kernels for gfx950.
//
//  * eh_nonce_states: one lane per nonce builds the 140-byte Equihash input of nonce_first + i
//    (256-bit little-endian addition) and its BLAKE2b base state, so the host hashes nothing.
//  * eh_pow_filter: one wave per valid solution of eh_expand's compact list. The lanes pack the
//    2^K indices into the minimal encoding (whole 32-bit words of the big-endian bit stream per
//    lane, no atomics) and assemble the padded message
//        in140 || compactsize(solution bytes) || solution
//    as big-endian words in LDS; the wave then runs SHA-256d over it and compares the digest,
//    read as a little-endian 256-bit integer, with the target. Only entries at or below the
//    target are appended to the winner list (every entry in debug mode).
//  * eh_pow_check: message, hash and compare over caller-supplied (input, solution) pairs.
//
// The hash itself is serial (24 + 1 compressions for (200,9)); every lane of the wave computes
// it from the same LDS words (broadcast reads), which costs what one lane would and leaves the
// result in every lane for the lane-parallel output.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels/blake2b_device.h"
#include "kernels/sha256_device.h"

namespace bcpk {

template <int N_, int K_> struct PowCfg {
    static constexpr int N = N_, K = K_;
    static constexpr int IB = N / (K + 1) + 1;       // bits per index in the minimal encoding
    static constexpr int L = 1 << K;                 // indices per solution
    static constexpr int SOLW = L * IB / 8;          // solution bytes
    static constexpr int SOLWORDS = SOLW / 4;
    static constexpr int CS = SOLW < 253 ? 1 : 3;    // compactsize bytes
    static constexpr int MSG = 140 + CS + SOLW;      // header bytes
    static constexpr int BLOCKS = (MSG + 63) / 64;   // SHA-256 blocks
    static constexpr int MW = BLOCKS * 16;           // message words, padding included
    static constexpr int WINW = 11 + SOLWORDS;       // winner entry: nonce index, candidate, pass, 8 hash words, solution
    static_assert(IB <= 32 && (L * IB) % 32 == 0, "solution is a whole number of words");
    static_assert(SOLW <= 0xffff, "compactsize: one or three bytes");
    static_assert(MSG + 9 <= BLOCKS * 64, "the 0x80 byte and the bit length fit in the last data block");
};

// Kernel arguments of a mining job, as little-endian words (passed by value: no H2D copy).
struct EhPowParams {
    uint32_t prefix[27]; // CEquihashInput, 108 bytes
    uint32_t nonce[8];   // first nonce, 256-bit little-endian
    uint32_t target[8];  // 256-bit little-endian
};
struct EhPowTarget {
    uint32_t w[8];
};

// in140[i] = prefix || (nonce_first + i) mod 2^256, states[i] = its base state.
template <class P>
__global__ __launch_bounds__(64) void eh_nonce_states(EhPowParams p, int count, uint32_t* __restrict__ in140,
                                                      EhBaseState* __restrict__ states) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    uint32_t* o = in140 + (size_t)i * 35;
#pragma unroll
    for (int w = 0; w < 27; ++w) o[w] = p.prefix[w];
    uint64_t carry = (uint64_t)i;
#pragma unroll
    for (int q = 0; q < 4; ++q) { // carry across all four 64-bit words
        const uint64_t a = (uint64_t)p.nonce[2 * q] | ((uint64_t)p.nonce[2 * q + 1] << 32);
        const uint64_t s = a + carry;
        carry = s < a ? 1 : 0;
        o[27 + 2 * q] = (uint32_t)s;
        o[28 + 2 * q] = (uint32_t)(s >> 32);
    }
    EhBaseState bs;
    eh_header_state(reinterpret_cast<const uint8_t*>(o), P::N, P::K, bs); // reads back this lane's own stores
    states[i] = bs;
}

// Word w of the minimal encoding as a big-endian value: index i occupies bits [i*IB, (i+1)*IB)
// of the big-endian bit stream (the inverse of stream_bits in equihash_verify.hip).
template <class P> __device__ __forceinline__ uint32_t eh_pack_word(const uint32_t* idx, int w) {
    const int s = 32 * w;
    const int first = s / P::IB, last = (s + 31) / P::IB;
    uint32_t out = 0;
    for (int i = first; i <= last; ++i) {
        const uint32_t v = idx[i] & (uint32_t)((1ull << P::IB) - 1);
        const int sh = 32 - P::IB - (i * P::IB - s); // left shift that puts the index's top bit at its stream position
        out |= sh >= 0 ? (sh < 32 ? v << sh : 0u) : v >> -sh;
    }
    return out;
}

// Byte b >= 140 of the padded message; sol: the solution as big-endian words.
template <class P> __device__ __forceinline__ uint32_t eh_pow_msg_byte(const uint32_t* sol, int b) {
    constexpr int S0 = 140 + P::CS;
    if (b < S0) {
        const int j = b - 140;
        if (P::CS == 1) return (uint32_t)P::SOLW;
        return j == 0 ? 0xfdu : (j == 1 ? (uint32_t)(P::SOLW & 0xff) : (uint32_t)(P::SOLW >> 8));
    }
    if (b < P::MSG) {
        const int k = b - S0;
        return (sol[k >> 2] >> (24 - 8 * (k & 3))) & 0xff;
    }
    if (b == P::MSG) return 0x80u;
    const int j = b - (P::MW * 4 - 8); // big-endian 64-bit length in bits
    return j >= 0 ? (uint32_t)(((uint64_t)P::MSG * 8) >> (8 * (7 - j))) & 0xff : 0u;
}

// The padded message as big-endian words W[MW]; in140: 35 little-endian words (global memory).
template <class P>
__device__ __forceinline__ void eh_pow_message(uint32_t* W, const uint32_t* __restrict__ in140, const uint32_t* sol,
                                               int t) {
    for (int w = t; w < P::MW; w += 64) {
        uint32_t v;
        if (w < 35) {
            v = bswap32d(in140[w]);
        } else {
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v = (v << 8) | eh_pow_msg_byte<P>(sol, 4 * w + j);
        }
        W[w] = v;
    }
}

// SHA-256d of the padded message; h: the digest as 8 little-endian words (h[7] most significant
// when the digest is read as a 256-bit little-endian integer).
template <class P> __device__ __forceinline__ void eh_pow_hash(const uint32_t* W, uint32_t h[8]) {
    uint32_t s[8];
    sha256_init(s);
#pragma unroll 1
    for (int b = 0; b < P::BLOCKS; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = W[16 * b + i];
        sha256_transform(s, w);
    }
    uint32_t d[8];
    sha256_32(s, d);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = bswap32d(d[i]);
}

// hash <= target, both 256-bit little-endian (word 7 most significant).
__device__ __forceinline__ bool eh_pow_meets(const uint32_t h[8], const uint32_t t[8]) {
    bool le = true; // equal so far
#pragma unroll
    for (int i = 0; i < 8; ++i) { // from the least significant word up: a more significant difference overrides
        if (h[i] != t[i]) le = h[i] < t[i];
    }
    return le;
}

// One wave per entry (nonce, candidate, L indices) of eh_expand's compact list, grid-stride.
// ctr[0]: winners appended, ctr[1]: entries that repeat an earlier candidate's index list (the
// host-side Collect drops those too). keep_all: append every distinct entry with its pass flag.
template <class P>
__global__ __launch_bounds__(64) void eh_pow_filter(EhPowParams p, int count, const uint32_t* __restrict__ in140,
                                                    const uint32_t* __restrict__ nout,
                                                    const uint32_t* __restrict__ list, uint32_t maxent,
                                                    uint32_t* __restrict__ ctr, uint32_t* __restrict__ win,
                                                    int keep_all) {
    constexpr int L = P::L, EW = P::L + 2;
    __shared__ uint32_t idx[L];
    __shared__ uint32_t sol[P::SOLWORDS];
    __shared__ uint32_t W[P::MW];
    __shared__ uint32_t dup, slot;
    const int t = threadIdx.x;
    const uint32_t n = min(*nout, maxent);
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const uint32_t* ent = list + (size_t)e * EW;
        const uint32_t nonce = ent[0], cand = ent[1];
        if (nonce >= (uint32_t)count) continue; // uniform; never written by a correct expansion
        __syncthreads();                         // the previous entry's LDS is done with
        if (t == 0) dup = 0;
        for (int i = t; i < L; i += 64) idx[i] = ent[2 + i];
        __syncthreads();
        // the same index list from an earlier candidate of this nonce: keep the first only
        for (uint32_t j = t; j < n; j += 64) {
            const uint32_t* o = list + (size_t)j * EW;
            if (j == e || o[0] != nonce || o[1] >= cand) continue;
            bool same = true;
            for (int i = 0; i < L && same; ++i) same = o[2 + i] == idx[i];
            if (same) dup = 1;
        }
        for (int w = t; w < P::SOLWORDS; w += 64) sol[w] = eh_pack_word<P>(idx, w);
        __syncthreads();
        if (dup) { // uniform
            if (t == 0) atomicAdd(&ctr[1], 1u);
            continue;
        }
        eh_pow_message<P>(W, in140 + (size_t)nonce * 35, sol, t);
        __syncthreads();
        uint32_t h[8];
        eh_pow_hash<P>(W, h);
        const bool pass = eh_pow_meets(h, p.target);
        if (!pass && !keep_all) continue; // uniform
        if (t == 0) slot = atomicAdd(&ctr[0], 1u);
        __syncthreads();
        uint32_t* o = win + (size_t)slot * P::WINW;
        if (t == 0) {
            o[0] = nonce;
            o[1] = cand;
            o[2] = pass ? 1u : 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[3 + i] = h[i];
        }
        for (int w = t; w < P::SOLWORDS; w += 64) o[11 + w] = bswap32d(sol[w]); // stream order in memory
    }
}

// One wave per (in140, solution) pair: hash and compare, no packing.
template <class P>
__global__ __launch_bounds__(64) void eh_pow_check(const uint32_t* __restrict__ in140, const uint32_t* __restrict__ sols,
                                                   EhPowTarget target, uint32_t* __restrict__ hashes,
                                                   uint8_t* __restrict__ pass) {
    __shared__ uint32_t sol[P::SOLWORDS];
    __shared__ uint32_t W[P::MW];
    const int t = threadIdx.x;
    const size_t item = blockIdx.x;
    for (int w = t; w < P::SOLWORDS; w += 64) sol[w] = bswap32d(sols[item * P::SOLWORDS + w]);
    __syncthreads();
    eh_pow_message<P>(W, in140 + item * 35, sol, t);
    __syncthreads();
    uint32_t h[8];
    eh_pow_hash<P>(W, h);
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) hashes[item * 8 + i] = h[i];
        pass[item] = eh_pow_meets(h, target.w) ? 1 : 0;
    }
}

} // namespace bcpk
