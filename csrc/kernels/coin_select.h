// The coin selection's stochastic subset search, one trial at a time, shared by the device kernel
// (csrc/kernels/coin_select.hip) and its host twin (csrc/wallet/coinselect.cpp): one source, so
// both pick the same candidate, bit for bit.
//
// The search (reference src/wallet/wallet.cpp ApproximateBestSubset): `trials` independent trials
// over n amounts, sorted descending by the caller, each > 0, their sum below 2^63. A trial starts
// at total 0 and makes up to two passes over the coins in order. Pass 0 takes coin i iff its
// random bit is 1, pass 1 iff it is 0. Taking a coin adds its value; if the total then reaches
// the target, (total, trial, pass, i) is a candidate and the coin is put back. Pass 1 runs only
// when pass 0 recorded no candidate: pass 0 then put nothing back, so the coins it took are
// exactly those with bit 1 and pass 1 needs no memory of them, only the bits again. The result is
// the smallest candidate in the order (total, trial, pass, i): the reference's "strictly smaller
// total wins" with the trials in order.
//
// Random bits come from a counter, so a trial's bits depend on nothing but (seed, run, trial,
// coin): word w of trial t is SipHash-2-4 under (k0, k1 + run) of the 8-byte message
// (t << 32) | w, and coin i reads bit i & 63 of word i >> 6. Run 1 is the wallet's second search,
// at target + MIN_CHANGE.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels/siphash.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCP_CS_HD __host__ __device__ __forceinline__
#define BCP_CS_UNROLL16 _Pragma("unroll 16")
#else
#define BCP_CS_HD inline
#define BCP_CS_UNROLL16
#endif

namespace bcp {
namespace cs {

constexpr uint32_t CS_MAX_TRIALS = 65536;
constexpr uint64_t CS_MAX_COINS = 1ULL << 31;
constexpr uint64_t CS_NONE = ~0ULL;

// A candidate: its total, and (trial, pass, coin) packed so that integer order is their
// lexicographic order. No candidate: both words CS_NONE, which sorts after every real one.
struct Cand {
    uint64_t total, key;
};
BCP_CS_HD uint64_t KeyOf(uint32_t trial, uint32_t pass, uint32_t coin) {
    return ((uint64_t)trial << 33) | ((uint64_t)pass << 32) | coin;
}
BCP_CS_HD uint32_t TrialOf(uint64_t key) { return (uint32_t)(key >> 33); }
BCP_CS_HD uint32_t PassOf(uint64_t key) { return (uint32_t)(key >> 32) & 1; }
BCP_CS_HD uint32_t CoinOf(uint64_t key) { return (uint32_t)key; }
BCP_CS_HD bool Less(const Cand& a, const Cand& b) { return a.total < b.total || (a.total == b.total && a.key < b.key); }

// Word w of trial t under the run's key (k0, k1r = k1 + run)
BCP_CS_HD uint64_t RandomWord(uint64_t k0, uint64_t k1r, uint32_t t, uint32_t w) {
    sip::Sip s;
    s.Init(k0, k1r);
    s.Word(((uint64_t)t << 32) | w);
    s.Word(8ULL << 56); // the message is 8 bytes, no tail bytes
    return s.Final();
}

// One coin of a pass. Returns whether the coin stays taken. Branch-free: on the device every
// lane of a wave steps through the same coin.
BCP_CS_HD bool Step(int64_t& total, Cand& best, int64_t v, bool take, int64_t target, uint64_t key) {
    const int64_t nt = total + v;
    const bool hit = take & (nt >= target);
    const bool better = hit & ((uint64_t)nt < best.total);
    best.total = better ? (uint64_t)nt : best.total;
    best.key = better ? key : best.key;
    const bool keep = take & !hit;
    total = keep ? nt : total;
    return keep;
}

// The best candidate of trial t. A trial that has met the target exactly cannot do better and
// stops at the next word.
BCP_CS_HD Cand RunTrial(const int64_t* __restrict__ values, uint32_t n, int64_t target, uint64_t k0, uint64_t k1r,
                        uint32_t t) {
    Cand best{CS_NONE, CS_NONE};
    int64_t total = 0;
    const uint32_t words = (n + 63) >> 6;
    for (uint32_t pass = 0; pass < 2; ++pass) {
        if (pass == 1 && best.key != CS_NONE) break;
        for (uint32_t w = 0; w < words; ++w) {
            if (best.total == (uint64_t)target) return best;
            uint64_t bits = RandomWord(k0, k1r, t, w);
            if (pass) bits = ~bits;
            const uint32_t base = w << 6;
            const uint64_t key = KeyOf(t, pass, base);
            if (n - base >= 64) {
                BCP_CS_UNROLL16 // sixteen amounts per scalar load on the device
                for (uint32_t j = 0; j < 64; ++j) Step(total, best, values[base + j], (bits >> j) & 1, target, key + j);
            } else {
                for (uint32_t j = 0; j < n - base; ++j) Step(total, best, values[base + j], (bits >> j) & 1, target, key + j);
            }
        }
    }
    return best;
}

} // namespace cs
} // namespace bcp
