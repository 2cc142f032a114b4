// CheckBlockHeader for a batch of post-fork headers on the device: everything the node checks on
// a header besides the Equihash solution itself (reference src/validation.cpp CheckBlockHeader ->
// src/pow.cpp CheckProofOfWork, src/arith_uint256.cpp SetCompact), from the bytes the verify
// lanes already upload for eh_verify.
//
//  * eh_header_check: one wave per header. The lanes assemble the padded message
//        in140 || compactsize(solution bytes) || solution
//    in LDS and the wave hashes it (eh_pow_message / eh_pow_hash, the miner's device functions).
//    nBits (bytes 104..107 of the input) is decoded as SetCompact does, the target is checked
//    against the chain's pow limit, and hash <= target is eh_pow_meets. The verdicts go into the
//    header's status byte next to eh_verify's, the hash into hashes[8 * i ..].
//  * eh_header_links: one lane per header, stream-ordered after eh_header_check: header i names
//    header i - 1 as its predecessor (hashPrevBlock, bytes 4..35 of the input, equals hash i - 1).
//  * eh_compact_decode: the compact decode alone over a list of nBits values (tests).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels/equihash_pow.h"

namespace bcpk {

// Bits of a header's status byte (mirrored by bcp::gpu::HeaderStatus in gpu_api.h).
enum : uint32_t {
    EH_HDR_SOLUTION_VALID = 1, // eh_verify accepted the solution (and it had the right length)
    EH_HDR_TARGET_LEGAL = 2,   // nBits decodes to a target in (0, pow limit], not negative, no overflow
    EH_HDR_HASH_MEETS = 4,     // TARGET_LEGAL and hash <= target
    EH_HDR_HASH_VALID = 8,     // hashes[i] is the header's hash (clear: the solution has another length)
    EH_HDR_LINKED = 16,        // hashPrevBlock == hash of the header before it (header 0: set)
};

// arith_uint256::SetCompact: t = the target as 8 little-endian words (truncated to 256 bits as
// the reference's shift does), and the negative / overflow flags.
__device__ __forceinline__ void eh_compact_target(uint32_t nbits, uint32_t t[8], bool& negative, bool& overflow) {
    const uint32_t size = nbits >> 24;
    uint32_t word = nbits & 0x007fffffu;
    uint32_t wi = 0, bo = 0; // word index and bit offset of the mantissa's low byte
    if (size <= 3) {
        word >>= 8 * (3 - size);
    } else {
        const uint32_t s = size - 3; // bytes to shift left
        wi = s >> 2;
        bo = (s & 3) * 8;
    }
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) { // compares, not an indexed store: the words stay in registers
        uint32_t v = 0;
        if (i == wi) v = word << bo;
        if (i == wi + 1 && bo != 0) v = word >> (32 - bo);
        t[i] = v;
    }
    negative = word != 0 && (nbits & 0x00800000u) != 0;
    overflow = word != 0 && (size > 34 || (word > 0xffu && size > 33) || (word > 0xffffu && size > 32));
}

// CheckProofOfWork's test of the target alone: not negative, not zero, no overflow, <= limit.
__device__ __forceinline__ bool eh_target_legal(const uint32_t t[8], bool negative, bool overflow,
                                                const uint32_t limit[8]) {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) any |= t[i];
    return !negative && any != 0 && !overflow && eh_pow_meets(t, limit);
}

// One wave per header. status[i] holds eh_verify's 0 / 1 on entry and the status bits (without
// LINKED) on return.
template <class P>
__global__ __launch_bounds__(64) void eh_header_check(const uint32_t* __restrict__ in140,
                                                      const uint32_t* __restrict__ sols,
                                                      const uint8_t* __restrict__ lenok, EhPowTarget limit,
                                                      uint32_t* __restrict__ hashes, uint8_t* __restrict__ status) {
    __shared__ uint32_t sol[P::SOLWORDS];
    __shared__ uint32_t W[P::MW];
    const int t = threadIdx.x;
    const size_t item = blockIdx.x;
    const uint32_t* in = in140 + item * 35;
    for (int w = t; w < P::SOLWORDS; w += 64) sol[w] = bswap32d(sols[item * P::SOLWORDS + w]);
    __syncthreads();
    eh_pow_message<P>(W, in, sol, t);
    __syncthreads();
    uint32_t h[8];
    eh_pow_hash<P>(W, h);
    if (t == 0) {
        uint32_t target[8];
        bool negative, overflow;
        eh_compact_target(in[26], target, negative, overflow); // nBits: bytes 104..107
        const bool valid = lenok[item] != 0;
        const bool legal = eh_target_legal(target, negative, overflow, limit.w);
        uint32_t s = 0;
        if (valid && status[item] != 0) s |= EH_HDR_SOLUTION_VALID;
        if (legal) s |= EH_HDR_TARGET_LEGAL;
        if (valid) s |= EH_HDR_HASH_VALID;
        if (valid && legal && eh_pow_meets(h, target)) s |= EH_HDR_HASH_MEETS;
#pragma unroll
        for (int i = 0; i < 8; ++i) hashes[item * 8 + i] = valid ? h[i] : 0u;
        status[item] = (uint8_t)s;
    }
}

// One lane per header, after eh_header_check on the same stream.
__global__ __launch_bounds__(64) void eh_header_links(const uint32_t* __restrict__ in140,
                                                      const uint8_t* __restrict__ lenok,
                                                      const uint32_t* __restrict__ hashes,
                                                      uint8_t* __restrict__ status, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    bool linked = true;
    if (i > 0) {
        linked = lenok[i] != 0 && lenok[i - 1] != 0; // both hashes valid (lanes touch only their own status byte)
        const uint32_t* prev = in140 + (size_t)i * 35 + 1; // hashPrevBlock: bytes 4..35
        const uint32_t* h = hashes + (size_t)(i - 1) * 8;
#pragma unroll
        for (int w = 0; w < 8; ++w) linked = linked && prev[w] == h[w];
    }
    if (linked) status[i] = (uint8_t)(status[i] | EH_HDR_LINKED);
}

// targets[8 * i ..] = SetCompact(nbits[i]) as little-endian words, flags[i] = negative | overflow << 1.
__global__ __launch_bounds__(64) void eh_compact_decode(const uint32_t* __restrict__ nbits, int n,
                                                        uint32_t* __restrict__ targets, uint8_t* __restrict__ flags) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t t[8];
    bool negative, overflow;
    eh_compact_target(nbits[i], t, negative, overflow);
#pragma unroll
    for (int w = 0; w < 8; ++w) targets[(size_t)i * 8 + w] = t[w];
    flags[i] = (uint8_t)((negative ? 1 : 0) | (overflow ? 2 : 0));
}

} // namespace bcpk
