// equihash_key_slots_tests: the slot rounds of the Equihash solver (EhCfg::ks) as
// csrc/kernels/equihash_layout.h describes them: which rounds keep key slots instead of the key
// sort, their LDS bytes (pinned to what the compiler reports for eh_round<Cfg200_9, S, *, CARRY>,
// profiles/raw/r10/resources.md), the workgroup barriers per bucket of either round variant, the
// size of the overflow list and the per-nonce counters.
#include "test/unittest.h"

#include "kernels/equihash_layout.h"

#include <initializer_list>
#include <vector>

namespace {

using namespace bcpk;

// the rounds that are slot rounds
template <class C> std::vector<int> SlotRounds() {
    std::vector<int> r;
    for (int s = 0; s <= C::K + 1; ++s)
        if (C::ks(s) > 0) r.push_back(s);
    return r;
}

} // namespace

TEST_CASE(equihash_key_slots_tests, slot_rounds) {
    // (200,9): rounds 3..8; 1 and 2 would need ~174 KB of LDS, the final round keeps the sort
    CHECK(SlotRounds<Cfg200_9>() == (std::vector<int>{3, 4, 5, 6, 7, 8}));
    // (96,5): every collision round (512 keys, ~1024 rows per bucket); (48,5): none (32 keys)
    CHECK(SlotRounds<Cfg96_5>() == (std::vector<int>{1, 2, 3, 4}));
    CHECK(SlotRounds<Cfg48_5>().empty());
    for (int s : SlotRounds<Cfg200_9>()) CHECK_EQ(Cfg200_9::ks(s), 8);
    for (int s : SlotRounds<Cfg96_5>()) CHECK_EQ(Cfg96_5::ks(s), 8);
    using C = Cfg200_9;
    for (int s : {1, 2}) {
        CHECK(slot_lds<C>(s, round_prunes<C>(s), false) > C::LDS_BUDGET);
        CHECK(!slot_round_fits<C>(s));
    }
}

// slot_lds against the LDS bytes per block the compiler reports for the slot rounds of (200,9)
TEST_CASE(equihash_key_slots_tests, lds_matches_compiler) {
    using C = Cfg200_9;
    const int plain[6] = {156492, 156492, 145996, 129612, 129612, 113228};
    const int carrying[6] = {161728, 161728, 151232, 134848, 134848, 117440};
    const int ovl_default = 128 * 4; // the pinned bytes are those of the default overflow list
    for (int s = 3; s <= 8; ++s) {
        CHECK_EQ(slot_lds<C>(s, round_prunes<C>(s, false), false) - BCP_EH_OVL * 4 + ovl_default, plain[s - 3]);
        CHECK_EQ(slot_lds<C>(s, round_prunes<C>(s, true), true) - BCP_EH_OVL * 4 + ovl_default, carrying[s - 3]);
        CHECK(slot_lds<C>(s, round_prunes<C>(s, false), false) <= C::LDS_BUDGET);
        CHECK(slot_lds<C>(s, round_prunes<C>(s, true), true) <= C::LDS_BUDGET);
        CHECK(C::LDS_BUDGET == 160 * 1024);
        // a slot round prunes like the sorted one: round_prunes is about the sorted round's bytes
        CHECK(round_prunes<C>(s, false) == round_prunes<C>(s, true));
    }
    // (96,5): within budget, plain and carrying
    for (int s : SlotRounds<Cfg96_5>()) {
        CHECK(slot_lds<Cfg96_5>(s, round_prunes<Cfg96_5>(s, false), false) <= Cfg96_5::LDS_BUDGET);
        CHECK(slot_lds<Cfg96_5>(s, round_prunes<Cfg96_5>(s, true), true) <= Cfg96_5::LDS_BUDGET);
    }
}

TEST_CASE(equihash_key_slots_tests, union_layout) {
    using C = Cfg200_9;
    // ktab: 16 bytes per key at the 16-byte aligned start of the union, then the key counters, the
    // overflow list and the pair list
    CHECK_EQ(un_slot_bend<C>(), C::NRESTS * 16);
    CHECK_EQ(un_slot_bend<C>(), 32 * 1024);
    CHECK_EQ(un_slot_ovl<C>(), un_slot_bend<C>() + C::NRESTS * 4);
    CHECK_EQ(un_slot_list<C>(), un_slot_ovl<C>() + BCP_EH_OVL * 4);
    CHECK(un_slot_list<C>() % 4 == 0);
    for (int s = 3; s <= 8; ++s)
        for (bool carry : {false, true})
            CHECK_EQ(slot_un<C>(s, carry), un_slot_list<C>() + round_mp<C>(s, carry) * round_nt<C>(s, carry) * 4);
    // the overflow list: at least four times the fullest bucket of the bench's 20 default steps
    // (profiles/equihash_r10.md), one lane per entry in the smallest round workgroup
    constexpr int MOST_SEEN = 16;
    CHECK(BCP_EH_OVL >= 4 * MOST_SEEN);
    CHECK(BCP_EH_OVL <= round_nt<Cfg96_5>(1, true));
    CHECK(BCP_EH_OVL <= round_nt<C>(3, true));
    // ranks and the two overflow flags share 16 bits
    CHECK(C::AREA_NF < 0x4000);
    CHECK(Cfg96_5::AREA_NF < 0x4000);
}

// The barriers of a bucket iteration: one constant per round variant, which the round waves and
// the generation waves both take from eh_bars.
TEST_CASE(equihash_key_slots_tests, barriers) {
    constexpr EhBars sorted = eh_bars(false), slot = eh_bars(true);
    CHECK_EQ(sorted.n, 10);
    CHECK_EQ(slot.n, 7);
    // commit, [key scan x2, key placement], listing, filter, destination scan x2, pair sort, emit
    CHECK_EQ(sorted.list, 5);
    CHECK_EQ(slot.list, 2);
    for (const EhBars& b : {sorted, slot}) {
        CHECK_EQ(b.filter, b.list + 1);
        CHECK_EQ(b.scan, b.filter + 1);
        CHECK_EQ(b.sort, b.scan + 2);
        CHECK_EQ(b.n, b.sort + 1);
    }
    CHECK_EQ(sorted.n - slot.n, 3);
}

TEST_CASE(equihash_key_slots_tests, counters) {
    using C = Cfg200_9;
    // [1..K] pair drops, [K+1..2K] row drops; slot rounds add [2K+2..3K+1] and [3K+2..4K+1]
    CHECK_EQ(C::PDW, 4 * C::K + 2);
    CHECK_EQ(Cfg96_5::PDW, 4 * 5 + 2);
    CHECK(3 * C::K + 1 + C::K < C::PDW); // the last round's bucket maximum is inside
}
