// equihash_layout_tests: the Equihash solver's layout description (csrc/kernels/equihash_layout.h),
// checked on the host for the three configurations: slot widths and padding bits, the stages with
// table parents, the parent decoders against slots built as the rounds' emit builds them, the
// pair-table and LDS sizes (pinned to what the compiler reports for the round kernels,
// profiles/raw/r9/resources.md), the per-instantiation geometry (EhRoundGeom) against the functions
// it gathers, and the coverage of the carried generation.
#include "test/unittest.h"

#include "kernels/equihash_layout.h"

#include <random>
#include <set>
#include <utility>

namespace {

using namespace bcpk;

int Popcount(uint32_t x) { return __builtin_popcount(x); }

// the stages whose parents sit in tables
template <class C> std::set<int> TableStages() {
    std::set<int> s;
    for (int st = 0; st < C::K; ++st)
        if (C::tp(st)) s.insert(st);
    return s;
}

template <class C> void CheckSlotWidths() {
    CHECK(C::AREA < (1 << C::IB));
    for (int s = 0; s < C::K; ++s) {
        // one parent form per stage: table parents take precedence over the compact word
        const int extra = s == 0 || C::tp(s) ? 0 : C::cp(s) ? 1 : 2;
        CHECK_EQ(C::sw(s), C::words(s) + extra);
        CHECK_EQ(C::rmask(s), C::tp(s) ? (uint32_t)C::NB - 1 : C::cp(s) ? C::RMASK : 0u);
        CHECK(Popcount(C::rmask(s)) <= C::pad(s));
        CHECK(C::rmask(s) == 0 || C::rmask(s) < (1ull << C::pad(s))); // the parent bits are padding bits
        if (C::tp(s)) {
            CHECK(C::tpmask(s) >= (uint32_t)C::NB - 1);
            CHECK(Popcount(C::tpmask(s)) <= C::pad(s));
            CHECK(s >= 1 && s <= C::K - 2);
        }
    }
}

// A random row of stage s whose padding carries `parent_bits`, as the emit leaves it: the shift by
// one digit zeroes the padding, then the parent bits are ORed in.
template <class C> std::vector<uint32_t> RandomRow(int s, std::mt19937& rng, uint32_t parent_bits) {
    std::vector<uint32_t> row(C::words(s));
    for (auto& w : row) w = rng();
    row.back() &= ~(uint32_t)((1ull << C::pad(s)) - 1);
    row.back() |= parent_bits;
    return row;
}

template <class C> void CheckSlotRoundTrip() {
    std::mt19937 rng(20260901);
    const uint32_t ends[4] = {0, 1, (uint32_t)C::AREA - 2, (uint32_t)C::AREA - 1};
    for (int s = 1; s < C::K; ++s) {
        if (C::tp(s)) continue; // CheckTableWalk
        for (uint32_t d = 0; d < (uint32_t)C::NB; ++d)
            for (uint32_t i : ends)
                for (uint32_t j : ends) {
                    const std::vector<uint32_t> row = RandomRow<C>(s, rng, 0);
                    std::vector<uint32_t> slot(row);
                    if (C::cp(s)) {
                        slot.back() |= (d >> C::DX) & C::rmask(s);
                        slot.push_back(cpack<C>(d, i, j));
                    } else {
                        slot.push_back((j << 16) | i);
                        slot.push_back(d);
                    }
                    REQUIRE((int)slot.size() == C::sw(s));
                    CHECK_EQ(slot_parent<C>(s, slot.data()), pack_tri(d, i, j));
                    for (int w = 0; w < C::words(s); ++w)
                        CHECK_EQ(slot[w] & ~(w == C::words(s) - 1 ? C::rmask(s) : 0u), row[w]);
                }
    }
}

// One producing bucket's emit into synthetic tables: destination area b receives cnt[b] rows, the
// ordinals F[b] .. F[b] + cnt[b] - 1 in destination order, at the claimed run start[b] of that area.
template <class C> void CheckTableWalk() {
    std::mt19937 rng(20260902);
    constexpr uint32_t NB = C::NB;
    for (int s : TableStages<C>()) {
        const uint32_t PT = C::ptab(s);
        std::vector<uint32_t> btab((size_t)NB * NB, 0x5a5a5a5au), ptab((size_t)NB * PT);
        for (auto& w : ptab) w = rng();
        for (uint32_t d : {0u, 1u, NB - 1}) {
            // a full pair table: PT ordinals over the NB destinations, some of them empty
            std::vector<uint32_t> cnt(NB, 0), first(NB), start(NB);
            uint32_t left = PT;
            for (uint32_t b = 0; b < NB; ++b) {
                cnt[b] = b == NB - 1 ? left : std::min<uint32_t>(left, b % 3 == 2 ? 0 : PT / NB + b % 5);
                left -= cnt[b];
            }
            REQUIRE(cnt[NB - 1] < (uint32_t)C::AREA / 2);
            uint32_t t0 = 0;
            for (uint32_t b = 0; b < NB; ++b) {
                first[b] = t0;
                t0 += cnt[b];
                start[b] = (b * 37 + d) % ((uint32_t)C::AREA / 2);
                btab[(size_t)d * NB + b] = start[b] - first[b]; // may wrap: unsigned, as on the device
            }
            REQUIRE(t0 == PT);
            auto walk = [&](uint32_t b, uint32_t t, uint32_t extra_bits, bool* in) {
                const std::vector<uint32_t> row = RandomRow<C>(s, rng, (d & C::rmask(s)) | extra_bits);
                return table_parent<C>(s, row.data(), b, start[b] + (t - first[b]), btab.data(), ptab.data(), in);
            };
            for (uint32_t b = 0; b < NB; ++b) {
                if (!cnt[b]) continue;
                for (uint32_t t : {first[b], first[b] + cnt[b] - 1}) { // both ends of every run: the first and the
                    bool in = false;                                   // last ordinal and every run boundary
                    CHECK_EQ(walk(b, t, 0, &in), ((uint64_t)d << 32) | ptab[(size_t)d * PT + t]);
                    CHECK(in);
                }
            }
            // a set padding bit above the bucket: a producing bucket >= NB (DebugExpandCorrupt mode 3)
            bool in = true;
            if (C::pad(s) > C::BB) {
                CHECK(C::tpmask(s) > NB - 1);
                CHECK_EQ(walk(0, first[0], NB, &in), ((uint64_t)(d | NB) << 32) | NIL);
                CHECK(!in);
            }
            // a run base that puts the slot one past the pair table (mode 4)
            const uint32_t b = NB - 1;
            const std::vector<uint32_t> row = RandomRow<C>(s, rng, d & C::rmask(s));
            btab[(size_t)d * NB + b] = start[b] - PT;
            in = true;
            CHECK_EQ(table_parent<C>(s, row.data(), b, start[b], btab.data(), ptab.data(), &in), ((uint64_t)d << 32) | NIL);
            CHECK(!in);
            btab[(size_t)d * NB + b] = start[b] - (PT - 1); // the last ordinal is still inside
            CHECK_EQ(table_parent<C>(s, row.data(), b, start[b], btab.data(), ptab.data(), &in),
                     ((uint64_t)d << 32) | ptab[(size_t)d * PT + PT - 1]);
            CHECK(in);
        }
    }
}

template <class C> void CheckSizes() {
    for (int s = 1; s < C::K; ++s) {
        CHECK(C::ptab(s) >= round_mp<C>(s, false) * round_nt<C>(s, false));
        if (C::GW > 0) CHECK(C::ptab(s) >= round_mp<C>(s, true) * round_nt<C>(s, true));
    }
    for (int s = 1; s <= C::K; ++s) {
        CHECK(round_lds<C>(s, round_prunes<C>(s, false), false) <= C::LDS_BUDGET);
        if (C::GW > 0 && s < C::K) CHECK(round_lds<C>(s, round_prunes<C>(s, true), true) <= C::LDS_BUDGET);
    }
}

// EhRoundGeom<C, S, CARRY> against the functions it gathers
template <class C, int S, bool CARRY> void CheckGeom() {
    using G = EhRoundGeom<C, S, CARRY>;
    CHECK_EQ(G::FINAL, S == C::K);
    CHECK_EQ(G::WI, C::words(S - 1));
    CHECK_EQ(G::WO, S < C::K ? C::words(S) : 1);
    CHECK_EQ(G::CAP, C::cap(S));
    CHECK_EQ(G::PRUNE, round_prunes<C>(S, CARRY));
    CHECK_EQ(G::SLOT, C::ks(S) > 0);
    CHECK_EQ(G::NBAR, eh_bars(G::SLOT).n);
    CHECK_EQ(G::BAR.list, eh_bars(G::SLOT).list);
    CHECK_EQ(G::BAR.sort, eh_bars(G::SLOT).sort);
    CHECK_EQ(G::NT, round_nt<C>(S, CARRY));
    CHECK_EQ(G::MP, round_mp<C>(S, CARRY));
    CHECK_EQ(G::RPL, (C::cap(S) + G::NT - 1) / G::NT);
    CHECK_EQ(G::SLI, (G::RPL + BCP_EH_PF_SLICES - 1) / BCP_EH_PF_SLICES);
    CHECK_EQ(G::BPT, (C::NB + G::NT - 1) / G::NT);
    CHECK_EQ(G::SWI, C::sw(S - 1));
    CHECK_EQ(G::SWO, S < C::K ? C::sw(S) : 1);
    CHECK_EQ(G::TPO, S < C::K && C::tp(S));
    CHECK_EQ(G::PTW, G::TPO ? C::ptab(S) : 1);
    CHECK_EQ(G::CPI, C::cp(S - 1));
    CHECK_EQ(G::RMI, C::rmask(S - 1));
    CHECK_EQ(G::RMO, C::rmask(S));
    CHECK_EQ(G::OCAP, (uint32_t)C::cap(S < C::K ? S + 1 : C::K));
    CHECK_EQ(G::LWI, G::WI + (G::PRUNE ? (G::CPI ? 1 : 2) : 0));
    CHECK_EQ(sizeof(typename G::HT), C::H16 ? 2u : 4u);
    CHECK_EQ(G::UN_BYTES, G::SLOT ? slot_un<C>(S, CARRY) : round_un<C>(S, CARRY));
    CHECK_EQ(G::UN_BEND, G::SLOT ? un_slot_bend<C>() : un_walk_bend<C>(C::cap(S)));
    CHECK_EQ(G::UN_OVL, un_slot_ovl<C>());
    CHECK_EQ(G::UN_PLIST, G::SLOT ? un_slot_list<C>() : un_walk_list<C>(C::cap(S)));
    CHECK_EQ(G::LDS_BYTES, G::SLOT ? slot_lds<C>(S, G::PRUNE, CARRY) : round_lds<C>(S, G::PRUNE, CARRY));
    // the LDS arrays the kernel declares add up to LDS_BYTES (rows rounded to 16 bytes, pdw to 4; a
    // final round keeps one-word placeholders the compiler drops; a carrying slot round rounds to 8)
    if (S < C::K) {
        const int gen = CARRY ? 2 * C::NB * 4 + 16 * 8 : 0;
        const int sum = (int)sizeof(typename G::Rows) + (G::PRUNE ? (int)sizeof(typename G::Psig) : 0) +
                        (G::PRUNE && !G::CPI ? ((int)sizeof(typename G::Pdw) + 3) / 4 * 4 : 0) + 4 + (G::SLOT ? 4 : 0) +
                        G::UN_BYTES + 2 * (int)sizeof(typename G::Hist) + ((int)sizeof(typename G::Base) + 3) / 4 * 4 +
                        (int)sizeof(typename G::Wsum) + gen;
        CHECK_EQ(G::SLOT && CARRY ? (sum + 7) / 8 * 8 : sum, G::LDS_BYTES);
    }
}
template <class C, int... S> void CheckGeoms(std::integer_sequence<int, S...>) {
    (CheckGeom<C, S + 1, false>(), ...);
    if constexpr (C::GW > 0) ((S + 1 < C::K ? CheckGeom<C, (S + 1 < C::K ? S + 1 : 1), true>() : void()), ...);
}

} // namespace

TEST_CASE(equihash_layout_tests, round_geometry) {
    CheckGeoms<Cfg200_9>(std::make_integer_sequence<int, Cfg200_9::K>{});
    CheckGeoms<Cfg96_5>(std::make_integer_sequence<int, Cfg96_5::K>{});
    CheckGeoms<Cfg48_5>(std::make_integer_sequence<int, Cfg48_5::K>{});
}

TEST_CASE(equihash_layout_tests, slot_widths) {
    CheckSlotWidths<Cfg200_9>();
    CheckSlotWidths<Cfg96_5>();
    CheckSlotWidths<Cfg48_5>();
}

TEST_CASE(equihash_layout_tests, table_stages) {
    CHECK(TableStages<Cfg200_9>() == (std::set<int>{1, 2, 3, 4, 6, 7}));
    CHECK(TableStages<Cfg96_5>().empty());
    CHECK(TableStages<Cfg48_5>().empty());
}

TEST_CASE(equihash_layout_tests, slot_parent_round_trip) {
    CheckSlotRoundTrip<Cfg200_9>();
    CheckSlotRoundTrip<Cfg96_5>();
    CheckSlotRoundTrip<Cfg48_5>();
}

TEST_CASE(equihash_layout_tests, table_parent_walk) {
    CheckTableWalk<Cfg200_9>();
    CheckTableWalk<Cfg96_5>();
    CheckTableWalk<Cfg48_5>();
}

TEST_CASE(equihash_layout_tests, pair_table_and_lds_sizes) {
    CheckSizes<Cfg200_9>();
    CheckSizes<Cfg96_5>();
    CheckSizes<Cfg48_5>();
    // two final-round workgroups of (200,9) share a CU
    using C = Cfg200_9;
    CHECK(2 * round_lds<C>(C::K, round_prunes<C>(C::K), false) <= 160 * 1024);
}

// round_lds against the LDS bytes per block the compiler reports for eh_round<Cfg200_9, S, *, CARRY>
TEST_CASE(equihash_layout_tests, lds_matches_compiler) {
    using C = Cfg200_9;
    const int plain[9] = {149704, 149704, 132040, 132040, 122440, 106568, 106568, 90184, 80456};
    const int carrying[8] = {154936, 154936, 137272, 137272, 127672, 111800, 111800, 94392};
    for (int s = 1; s <= 9; ++s) CHECK_EQ(round_lds<C>(s, round_prunes<C>(s, false), false), plain[s - 1]);
    for (int s = 1; s <= 8; ++s) CHECK_EQ(round_lds<C>(s, round_prunes<C>(s, true), true), carrying[s - 1]);
}

TEST_CASE(equihash_layout_tests, carried_generation) {
    using G200 = GenCarry<Cfg200_9>;
    using G96 = GenCarry<Cfg96_5>;
    CHECK((long long)G200::CH * G200::ITERS >= G200::NHASH);
    CHECK((long long)G96::CH * G96::ITERS >= G96::NHASH);
    CHECK((GenReg<Cfg200_9, Cfg200_9::GNT, Cfg200_9::GHPT>::OK));
    CHECK(!(GenReg<Cfg96_5, Cfg96_5::GNT, Cfg96_5::GHPT>::OK));
    CHECK(!(GenReg<Cfg48_5, Cfg48_5::GNT, Cfg48_5::GHPT>::OK));
}
