// The wallet match table and the per-item match, shared by the device kernel
// (csrc/kernels/wallet_match.hip) and its host twin (csrc/wallet/walletmatch.cpp): one source, so
// fingerprints, probe order and flags are the same on both sides, false positives included.
//
// Table: open addressing over 64-bit entries, a power-of-two number of slots, load factor at most
// 1/2. An entry is the salted fingerprint of a member (SipHash-2-4 under the table's 128-bit salt)
// with its low three bits replaced by 4 | tag, so no entry is 0 (an empty slot) and the four sets
// share one table. The home slot comes from the fingerprint's high half. The builder places every
// entry within WM_MAX_PROBE slots of its home (it grows the table otherwise), so a lookup reads at
// most that many slots and stops at the first empty one.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels/siphash.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCP_WM_HD __host__ __device__ __forceinline__
#else
#define BCP_WM_HD inline
#endif

namespace bcp {
namespace wm {

enum Tag : uint32_t {
    TAG_K = 0, // key ids and script ids (20 bytes)
    TAG_W = 1, // watch-only scripts, the whole scriptPubKey
    TAG_T = 2, // wallet txids (32 bytes)
    TAG_S = 3, // spent outpoints (36 bytes)
};
// One flag byte per item: a bit per set hit. NOT_READ (the bloom kernel's 2) alone marks an item
// that reaches past the blob, has a length its kind cannot have, or is of no known kind: nothing of
// it is read.
enum Flag : uint8_t { HIT_K = 1, NOT_READ = 2, HIT_W = 4, HIT_T = 8, HIT_S = 16 };
enum Kind : uint8_t {
    ITEM_TXID = 0,   // 32 bytes: probes T
    ITEM_INPUT = 1,  // a 36-byte prevout: probes S with all of it and T with its first 32 bytes
    ITEM_OUTPUT = 2, // a scriptPubKey of 0..10,000 bytes: its pushes probe K, the whole probes W
};
constexpr uint32_t KIND_MASK_ALL = 7;
constexpr uint32_t KIND_MASK_COINS = 3; // txids and inputs: what a table of T and S entries can hit
constexpr uint32_t WM_MAX_PROBE = 32;
constexpr uint32_t WM_MIN_SLOTS = 8;
constexpr uint32_t WM_MAX_SCRIPT = 10000;
// A table of at most this many bytes (8,192 slots: up to 4,096 entries) is staged to LDS.
constexpr uint32_t WM_LDS_MAX_BYTES = 65536;

struct TableView {
    const uint64_t* slots;
    uint32_t mask; // slots - 1
    uint64_t k0, k1;
    uint32_t hasWatch; // the table holds W entries
};

using sip::Rotl64;
using sip::Sip; // SipHash-2-4 (kernels/siphash.h)
BCP_WM_HD uint32_t Rotl32(uint32_t x, int b) { return (x << b) | (x >> (32 - b)); }

// Members sit at any byte offset: byte loads, never past the last byte.
BCP_WM_HD uint32_t LoadLE32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
BCP_WM_HD uint64_t LoadLE64(const uint8_t* p) { return (uint64_t)LoadLE32(p) | ((uint64_t)LoadLE32(p + 4) << 32); }

// SipHash-2-4 of len bytes
BCP_WM_HD uint64_t Fingerprint(uint64_t k0, uint64_t k1, const uint8_t* p, uint32_t len) {
    Sip s;
    s.Init(k0, k1);
    const uint32_t full = len >> 3;
    for (uint32_t w = 0; w < full; ++w) s.Word(LoadLE64(p + 8 * (size_t)w));
    uint64_t last = (uint64_t)(len & 0xff) << 56;
    const uint8_t* tail = p + 8 * (size_t)full;
    for (uint32_t b = 0; b < (len & 7); ++b) last |= (uint64_t)tail[b] << (8 * b);
    s.Word(last);
    return s.Final();
}
// The same of a 20-byte id given as five little-endian words
BCP_WM_HD uint64_t Fingerprint20(uint64_t k0, uint64_t k1, const uint32_t w[5]) {
    Sip s;
    s.Init(k0, k1);
    s.Word((uint64_t)w[0] | ((uint64_t)w[1] << 32));
    s.Word((uint64_t)w[2] | ((uint64_t)w[3] << 32));
    s.Word((uint64_t)w[4] | ((uint64_t)20 << 56));
    return s.Final();
}

BCP_WM_HD uint64_t EntryOf(uint64_t fp, uint32_t tag) { return (fp & ~(uint64_t)7) | 4 | tag; }
BCP_WM_HD uint32_t HomeOf(uint64_t fp, uint32_t mask) { return (uint32_t)(fp >> 32) & mask; }

BCP_WM_HD bool Probe(const uint64_t* slots, uint32_t mask, uint64_t fp, uint32_t tag) {
    const uint64_t want = EntryOf(fp, tag);
    uint32_t s = HomeOf(fp, mask);
    for (uint32_t i = 0; i < WM_MAX_PROBE; ++i) {
        const uint64_t e = slots[s];
        if (e == want) return true;
        if (e == 0) return false;
        s = (s + 1) & mask;
    }
    return false;
}

// ------------------------------------------------------------------ RIPEMD-160
// One compression of the 64-byte block that pads a 32-byte message (a SHA-256 digest): x[0..7] are
// the digest as little-endian words, out the RIPEMD-160 digest as little-endian words. The two
// lines of 80 steps are fully unrolled over constant tables, so the sixteen message words are
// named values (VGPRs on the device) and nothing is indexed at run time.
BCP_WM_HD uint32_t RmdF(int j, uint32_t x, uint32_t y, uint32_t z) {
    switch (j >> 4) {
    case 0: return x ^ y ^ z;
    case 1: return (x & y) | (~x & z);
    case 2: return (x | ~y) ^ z;
    case 3: return (x & z) | (y & ~z);
    default: return x ^ (y | ~z);
    }
}
BCP_WM_HD void Ripemd160Of32(const uint32_t d[8], uint32_t out[5]) {
    constexpr uint8_t RL[80] = {0, 1, 2,  3,  4,  5,  6,  7, 8,  9, 10, 11, 12, 13, 14, 15, 7, 4,  13, 1,  10, 6,  15, 3,  12, 0, 9,
                                5, 2, 14, 11, 8,  3,  10, 14, 4, 9,  15, 8,  1,  2,  7,  0,  6, 13, 11, 5,  12, 1,  9,  11, 10, 0, 8,
                                12, 4, 13, 3,  7,  15, 14, 5,  6, 2,  4,  0,  5,  9,  7,  12, 2, 10, 14, 1,  3,  8,  11, 6,  15, 13};
    constexpr uint8_t RR[80] = {5,  14, 7,  0, 9, 2,  11, 4, 13, 6,  15, 8,  1,  10, 3, 12, 6, 11, 3,  7,  0, 13, 5,  10, 14, 15, 8,
                                12, 4,  9,  1, 2, 15, 5,  1, 3,  7,  14, 6,  9,  11, 8, 12, 2, 10, 0,  4,  13, 8, 6,  4,  1,  3,  11,
                                15, 0,  5,  12, 2, 13, 9,  7, 10, 14, 12, 15, 10, 4,  1, 5,  8, 7,  6,  2,  13, 14, 0,  3,  9,  11};
    constexpr uint8_t SL[80] = {11, 14, 15, 12, 5,  8,  7,  9,  11, 13, 14, 15, 6,  7,  9,  8,  7,  6,  8,  13, 11, 9,  7,  15, 7, 12, 15,
                                9,  11, 7,  13, 12, 11, 13, 6,  7,  14, 9,  13, 15, 14, 8,  13, 6,  5,  12, 7,  5,  11, 12, 14, 15, 14, 15,
                                9,  8,  9,  14, 5,  6,  8,  6,  5,  12, 9,  15, 5,  11, 6,  8,  13, 12, 5,  12, 13, 14, 11, 8,  5,  6};
    constexpr uint8_t SR[80] = {8,  9,  9,  11, 13, 15, 15, 5,  7,  7,  8,  11, 14, 14, 12, 6,  9,  13, 15, 7,  12, 8,  9,  11, 7, 7,  12,
                                7,  6,  15, 13, 11, 9,  7,  15, 11, 8,  6,  6,  14, 12, 13, 5,  14, 13, 13, 7,  5,  15, 5,  8,  11, 14, 14,
                                6,  14, 6,  9,  12, 9,  12, 5,  15, 8,  8,  5,  12, 9,  12, 5,  14, 6,  8,  13, 6,  5,  15, 13, 11, 11};
    constexpr uint32_t KL[5] = {0x00000000u, 0x5A827999u, 0x6ED9EBA1u, 0x8F1BBCDCu, 0xA953FD4Eu};
    constexpr uint32_t KR[5] = {0x50A28BE6u, 0x5C4DD124u, 0x6D703EF3u, 0x7A6D76E9u, 0x00000000u};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = d[i];
    x[8] = 0x80;
#pragma unroll
    for (int i = 9; i < 16; ++i) x[i] = 0;
    x[14] = 256; // message bits
    const uint32_t h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
    uint32_t al = h0, bl = h1, cl = h2, dl = h3, el = h4;
    uint32_t ar = h0, br = h1, cr = h2, dr = h3, er = h4;
#pragma unroll
    for (int j = 0; j < 80; ++j) {
        uint32_t t = Rotl32(al + RmdF(j, bl, cl, dl) + x[RL[j]] + KL[j >> 4], SL[j]) + el;
        al = el; el = dl; dl = Rotl32(cl, 10); cl = bl; bl = t;
        t = Rotl32(ar + RmdF(79 - j, br, cr, dr) + x[RR[j]] + KR[j >> 4], SR[j]) + er;
        ar = er; er = dr; dr = Rotl32(cr, 10); cr = br; br = t;
    }
    out[0] = h1 + cl + dr;
    out[1] = h2 + dl + er;
    out[2] = h3 + el + ar;
    out[3] = h4 + al + br;
    out[4] = h0 + bl + cr;
}

// What CPubKey(push).GetID() hashes: the push when its header byte says its own length, else
// nothing (CPubKey::Set clears an ill-formed key, and GetID is then the HASH160 of no bytes).
BCP_WM_HD uint32_t PubKeyIdLen(const uint8_t* p, uint32_t n) {
    const uint8_t h = p[0];
    if (n == 33 && (h == 2 || h == 3)) return 33;
    if (n == 65 && (h == 4 || h == 6 || h == 7)) return 65;
    return 0;
}

// The flags of one item. kindMask: bit k set = items of kind k are matched, others get 0.
// hash160(p, len, id): id = five little-endian words of RIPEMD160(SHA256(p[0..len))).
// An output is walked by CScript::GetOp's rules up to its first failure (a length byte missing, or
// a push that runs past the end): a 20-byte push probes K, a push of 33..65 bytes probes K with
// the key id CPubKey would give it, and the walk ends at the first K hit.
template <typename H160>
BCP_WM_HD uint8_t MatchItem(const TableView& t, uint32_t kindMask, uint32_t kind, const uint8_t* p, uint32_t len,
                            H160&& hash160) {
    if (kind > ITEM_OUTPUT) return NOT_READ;
    if (!((kindMask >> kind) & 1)) return 0;
    uint8_t f = 0;
    if (kind == ITEM_TXID) {
        if (len != 32) return NOT_READ;
        if (Probe(t.slots, t.mask, Fingerprint(t.k0, t.k1, p, 32), TAG_T)) f |= HIT_T;
        return f;
    }
    if (kind == ITEM_INPUT) {
        if (len != 36) return NOT_READ;
        if (Probe(t.slots, t.mask, Fingerprint(t.k0, t.k1, p, 36), TAG_S)) f |= HIT_S;
        if (Probe(t.slots, t.mask, Fingerprint(t.k0, t.k1, p, 32), TAG_T)) f |= HIT_T;
        return f;
    }
    if (len > WM_MAX_SCRIPT) return NOT_READ;
    if (t.hasWatch && Probe(t.slots, t.mask, Fingerprint(t.k0, t.k1, p, len), TAG_W)) f |= HIT_W;
    uint32_t pc = 0;
    while (pc < len) {
        const uint32_t op = p[pc++];
        if (op > 0x4e) continue; // not a push
        uint32_t n;
        if (op < 0x4c) {
            n = op;
        } else if (op == 0x4c) { // OP_PUSHDATA1
            if (len - pc < 1) break;
            n = p[pc++];
        } else if (op == 0x4d) { // OP_PUSHDATA2
            if (len - pc < 2) break;
            n = (uint32_t)p[pc] | ((uint32_t)p[pc + 1] << 8);
            pc += 2;
        } else { // OP_PUSHDATA4
            if (len - pc < 4) break;
            n = LoadLE32(p + pc);
            pc += 4;
        }
        if (len - pc < n) break;
        uint32_t id[5];
        bool probe = false;
        if (n == 20) {
#pragma unroll
            for (int w = 0; w < 5; ++w) id[w] = LoadLE32(p + pc + 4 * w);
            probe = true;
        } else if (n >= 33 && n <= 65) {
            hash160(p + pc, PubKeyIdLen(p + pc, n), id);
            probe = true;
        }
        if (probe && Probe(t.slots, t.mask, Fingerprint20(t.k0, t.k1, id), TAG_K)) {
            f |= HIT_K;
            break;
        }
        pc += n;
    }
    return f;
}

} // namespace wm
} // namespace bcp
