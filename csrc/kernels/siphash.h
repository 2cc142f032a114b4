// SipHash-2-4 over 64-bit words, for the device and the host: the one copy behind the BIP152 short
// ids (relay.hip), the wallet match table's fingerprints (wallet_match.h) and the coin selection's
// random words (coin_select.h). On the device the four words stay in VGPR pairs (v_lshl_add_u64
// adds, v_alignbit rotates).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCP_SIP_HD __host__ __device__ __forceinline__
#else
#define BCP_SIP_HD inline
#endif

namespace bcp {
namespace sip {

BCP_SIP_HD uint64_t Rotl64(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

struct Sip {
    uint64_t v0, v1, v2, v3;
    BCP_SIP_HD void Init(uint64_t k0, uint64_t k1) {
        v0 = 0x736f6d6570736575ULL ^ k0;
        v1 = 0x646f72616e646f6dULL ^ k1;
        v2 = 0x6c7967656e657261ULL ^ k0;
        v3 = 0x7465646279746573ULL ^ k1;
    }
    BCP_SIP_HD void Round() {
        v0 += v1; v1 = Rotl64(v1, 13); v1 ^= v0; v0 = Rotl64(v0, 32);
        v2 += v3; v3 = Rotl64(v3, 16); v3 ^= v2;
        v0 += v3; v3 = Rotl64(v3, 21); v3 ^= v0;
        v2 += v1; v1 = Rotl64(v1, 17); v1 ^= v2; v2 = Rotl64(v2, 32);
    }
    // one 8-byte little-endian word of the message; the last word carries the length in its top byte
    BCP_SIP_HD void Word(uint64_t m) {
        v3 ^= m;
        Round();
        Round();
        v0 ^= m;
    }
    BCP_SIP_HD uint64_t Final() {
        v2 ^= 0xff;
        Round();
        Round();
        Round();
        Round();
        return v0 ^ v1 ^ v2 ^ v3;
    }
};

} // namespace sip
} // namespace bcp
