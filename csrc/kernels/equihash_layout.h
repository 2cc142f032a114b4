// Equihash solver (equihash_solver.hip): the memory layout of the stage arrays and the geometry of
// the kernels as compile-time arithmetic, read by the kernels and by the host side. No HIP header:
// csrc/test/equihash_layout_tests.cpp checks it on the CPU.
//
// Memory layout: every stage has its own slot array. Where the round that reads a stage prunes
// (or the row has no room for the producing bucket), a stage-s slot holds the row followed by its
// parent word(s), so the emit writes one contiguous slot per output row and the pruning round
// gets the parents with the rows. The other stages ((200,9): 1-4, 6, 7) keep "table parents"
// (EhCfg::tp): the slot is the row alone with the producing bucket d in its
// padding, so rounds 2..K-1 do not fetch parent words they never use (they share the rows' cache
// lines); the (j << 16 | i) word of every output row goes, in the emit's destination order, to a
// per-bucket pair table (consecutive lanes store consecutive words) and the run bases of the
// bucket to a run-base table, which only eh_expand reads. Keeping all K stage arrays and tables
// costs ~50 words per slot per nonce (≈17 GB per 32-nonce solver, against 288 GB of HBM); the
// parents must outlive the rows anyway for the final expansion. Per row per round: one contiguous
// slot read, one slot write into a claimed run, one pair-table word.
// The layouts of earlier merges (every slot with its parent words, TABLE_PARENTS=0; every round
// sorted, KEY_SLOTS=0) are no longer build options: commit 3ff18da is the last tree that builds them.
// EhRoundGeom (below) gathers the geometry of one round instantiation for the kernel and the host.
#ifndef BCP_KERNELS_EQUIHASH_LAYOUT_H
#define BCP_KERNELS_EQUIHASH_LAYOUT_H

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <type_traits>

#if defined(__HIPCC__)
#define BCP_EH_HD __host__ __device__
#else
#define BCP_EH_HD
#endif

// Build options that shape the layout (the solver's other options are in equihash_solver.hip):
#ifndef BCP_EH_GEN_HPT // (200,9) register generation: hashes per thread
#define BCP_EH_GEN_HPT 2
#endif
#ifndef BCP_EH_GEN_NT // (200,9) register generation: threads per workgroup
#define BCP_EH_GEN_NT 512
#endif
#ifndef BCP_EH_PRUNE_FROM // first round that drops pairs sharing a parent (reads the parent words with the rows);
                          // the final round always does.
#define BCP_EH_PRUNE_FROM 9 //  9 = the final round only: +4.2% Sol/s over 2 at the same recall (profiles/equihash_r5.md)
#endif
#ifndef BCP_EH_MP_LATE // extra pair slots per lane in the late collision rounds (see round_mp)
#define BCP_EH_MP_LATE 1
#endif
#ifndef BCP_EH_MP_LATE_FROM
#define BCP_EH_MP_LATE_FROM 8
#endif
#ifndef BCP_EH_GW // (200,9) generation waves of a carrying round workgroup (the round keeps 1024 - 64*GW threads)
#define BCP_EH_GW 4
#endif
#ifndef BCP_EH_PF_SLICES // the next bucket's rows are prefetched in this many slices (EhRoundGeom::SLI)
#define BCP_EH_PF_SLICES 3
#endif
#ifndef BCP_EH_OVL // slot rounds: entries of the overflow list (rows of rank >= EH_KEY_SLOTS in their key group).
#define BCP_EH_OVL 128 //   The fullest bucket of the bench's 20 default steps held 16 (profiles/equihash_r10.md)
#endif
static_assert(BCP_EH_OVL >= 1 && BCP_EH_OVL <= 128, "the overflow list is walked by the first BCP_EH_OVL lanes");

namespace bcpk {

// Slots per key of a "slot round" (EhCfg::ks): the commit files each row's id under its key, which
// replaces the key sort. Eight 16-bit row ids are one 16-byte LDS read.
constexpr int EH_KEY_SLOTS = 8;

// (defined with the round kernels' geometry below; EhCfg's table-parent layout follows from them)
template <class C> constexpr int round_nt(int stage, bool carry);
template <class C> constexpr int round_mp(int stage, bool carry = false);
template <class C> constexpr bool round_prunes(int stage, bool carry = false);
template <class C> constexpr bool slot_round_fits(int stage);

// N, K: Equihash parameters. BB: bucket bits. CAP/CAP4/CAP3: LDS row capacity of rounds reading
// rows of >= 5, 4, <= 3 words. NT: threads per round workgroup; WGCU: round workgroups per CU
// the LDS budget must allow. GENWG/NTG: LDS-sorted generation geometry; GNT x GHPT: register
// generation (threads x hashes per thread; 0 = use the LDS-sorted kernel).
template <int N_, int K_, int BB_, int CAP_, int NT_, int GENWG_, int NTG_, int MAXCAND_, int CAP4_ = CAP_,
          int CAP3_ = CAP_, int WGCU_ = 1, int GNT_ = 512, int GHPT_ = 2, int CAPF_ = 0, int MPX_ = 0, int GW_ = 0>
struct EhCfg {
    static constexpr int N = N_, K = K_;
    static constexpr int DB = N / (K + 1);           // digit bits
    static constexpr int BB = BB_;                   // bucket bits
    static constexpr int RB = DB - BB_;              // in-bucket collision bits
    static constexpr int NB = 1 << BB_;              // buckets (= areas of every stage)
    static constexpr int NRESTS = 1 << RB;
    // LDS row capacity of a round by the width of the rows it reads: the narrow late rounds
    // hold more rows (their buckets and pair lists overflow most, from duplicate subtrees)
    static constexpr int CAP = CAP_;                 // rounds reading >= 5-word rows
    // CAPF: the final round's capacity (0 = CAP3). Without depth-1 pruning before the final round,
    // duplicate subtrees pile up in a few stage-(K-1) buckets; a larger final area keeps the valid
    // rows of such a bucket from being crowded out (which rows are dropped follows the atomics).
    static constexpr int CAPF = CAPF_ > 0 ? CAPF_ : CAP3_;
    static constexpr int MPX = MPX_;                 // extra pair-list slots per lane in every collision round
    static constexpr int cap(int round) {
        return round == K_ ? CAPF : words(round - 1) >= 5 ? CAP_ : words(round - 1) == 4 ? CAP4_ : CAP3_;
    }
    // largest non-final capacity (sizes the per-lane pair registers) and the area of every stage
    static constexpr int AREA_NF = CAP_ > CAP4_ ? (CAP_ > CAP3_ ? CAP_ : CAP3_) : (CAP4_ > CAP3_ ? CAP4_ : CAP3_);
    static constexpr int AREA = AREA_NF > CAPF ? AREA_NF : CAPF;
    static constexpr int NT = NT_;                   // threads per round workgroup
    static constexpr int NW = NT_ / 64;
    // GW: generation waves a carrying collision round (eh_round with CARRY) runs beside its
    // NT - 64*GW round threads; 0 = the configuration never carries generation
    static constexpr int GW = GW_;
    static constexpr int RNT = NT_ - 64 * GW_;       // round threads of a carrying round
    static constexpr int WGCU = WGCU_;
    static constexpr int LDS_BUDGET = 160 * 1024 / WGCU_;
    static constexpr int INIT = 1 << (DB + 1);
    static constexpr int GENWG = GENWG_;             // LDS-sorted generation: workgroups per nonce
    static constexpr int NTG = NTG_;                 // LDS-sorted generation: threads per workgroup
    static constexpr int GNT = GNT_, GHPT = GHPT_;   // register generation geometry
    static constexpr int RPW = INIT / GENWG_;        // rows per generation workgroup
    static constexpr int IPH = 512 / N;
    static constexpr int NBYTES = N / 8;
    static constexpr int MAXCAND = MAXCAND_;
    static constexpr int L = 1 << K;
    static constexpr int bits(int stage) { return N - stage * DB - BB_; }
    static constexpr int words(int stage) { return (bits(stage) + 31) / 32; }
    static constexpr int WMAX = words(0);
    // Compact parents: the triple (d, i, j) as ONE word. i and j take IB bits each in the two
    // halves of the word, the 16 - IB spare bits of each half carry DX bits of d, and the DR
    // remaining bits of d ride in the low (padding) bits of the row's last word.
    static constexpr int IB = AREA <= 4096 ? 12 : 13;
    static constexpr int DH = 16 - IB;
    static constexpr uint32_t DHM = (1u << DH) - 1;
    static constexpr int DX = 2 * DH;
    static constexpr int DR = BB_ > DX ? BB_ - DX : 0;
    static constexpr uint32_t RMASK = (1u << DR) - 1;
    static constexpr uint32_t IMASK = ((1u << IB) - 1) * 0x10001u;
    static constexpr bool cp(int stage) {
        return stage >= 1 && stage < K && 32 * words(stage) - bits(stage) >= DR;
    }
    // Table parents: a stage whose reading round does not prune (plain or carrying) and whose rows
    // have BB padding bits keeps NO parent word in its slots. The whole producing bucket d rides
    // in the row's padding, the (j << 16 | i) word of output ordinal t (the emit's destination
    // order) goes to the pair table P[stage][nonce][d][t] (ptab() words per bucket, a coalesced
    // store), and the run-base table B[stage][nonce][d][b] holds (claimed run start in area b) -
    // (first ordinal of destination b), so a slot at position pos of area b has t = pos - B.
    // Only eh_expand reads P and B: the rounds 2..K-1 that read such a stage fetch rows alone.
    static constexpr int pad(int stage) { return 32 * words(stage) - bits(stage); }
    static constexpr bool tp(int stage) {
        return stage >= 1 && stage <= K - 2 && !round_prunes<EhCfg>(stage + 1) && !round_prunes<EhCfg>(stage + 1, true) &&
               pad(stage) >= BB;
    }
    // pair-table words per producing bucket: every ordinal the emit of either variant can hold
    static constexpr int ptab(int stage) {
        const int a = round_mp<EhCfg>(stage, false) * round_nt<EhCfg>(stage, false);
        const int b = GW_ > 0 ? round_mp<EhCfg>(stage, true) * round_nt<EhCfg>(stage, true) : 0;
        return a > b ? a : b;
    }
    // eh_expand reads the producing bucket of a table stage through every padding bit (up to BB + 1):
    // the rounds leave the bits above BB zero, so a set one marks a corrupt row
    static constexpr uint32_t tpmask(int stage) { return (1u << (pad(stage) > BB ? BB + 1 : BB)) - 1; }
    // parent bits in a row's padding
    static constexpr uint32_t rmask(int stage) { return tp(stage) ? (uint32_t)NB - 1 : cp(stage) ? RMASK : 0u; }
    // words per slot of stage s: the row, plus (s >= 1, no table parents) its parent word(s)
    static constexpr int sw(int stage) {
        return stage == 0 || tp(stage) ? words(stage) : words(stage) + (cp(stage) ? 1 : 2);
    }
    static constexpr size_t ROWS = (size_t)NB * AREA; // slots per stage per nonce
    // Slot rounds: ks(stage) > 0 when the collision round producing `stage` keeps, instead of the
    // key sort, a table of ks row ids per key filled at the commit (slot_lds below). Such a round
    // needs a key space worth the table (>= 256 keys: (48,5) has 32) and the table next to its
    // rows in LDS, plain and carrying: (200,9) rounds 3..8 (1 and 2 would take ~174 KB), every collision
    // round of (96,5). The final round keeps the sort.
    static constexpr int ks(int stage) {
        return stage >= 1 && stage < K && NRESTS >= 256 && slot_round_fits<EhCfg>(stage) ? EH_KEY_SLOTS : 0;
    }
    // Counters per nonce (pdrop): [1..K] pairs dropped per round, [K+1..2K] rows dropped per
    // stage, [2K+2..3K+1] overflow rows per slot round (2K+1+round) and [3K+2..4K+1] the most
    // overflow rows one bucket of the round had (3K+1+round).
    static constexpr int PDW = 4 * K + 2;
    // 16-bit LDS histograms (two counters per word) where 32-bit ones would not fit two per CU
    static constexpr bool H16 = NB > 512;
    static constexpr int HW = H16 ? NB / 2 : NB;      // words per histogram
    static_assert(RPW * GENWG_ == INIT && RPW < 65535, "generation split");
    static_assert(RB > 0 && DB < 32, "digit geometry");
    static_assert(AREA < (1 << IB), "LDS row indices in parent words and signatures");
    static_assert(NT_ % 64 == 0 && NT_ <= 1024 && (NB <= NT_ || NB % NT_ == 0) && NB <= NTG_ && NT_ / 64 <= 64,
                  "workgroup shape");
    static_assert(words(K - 1) == 1, "final round keeps whole rows in one LDS word");
    static_assert(GW_ == 0 || (WGCU_ == 1 && RNT >= 128 && (NB <= RNT || NB % RNT == 0)), "carrying workgroup shape");
};

// Mainnet/testnet (200,9): 512 buckets x ~4096 rows, one 1024-thread round workgroup per CU;
// (96,5); regtest (48,5).
#ifndef BCP_EH_CAPF // (200,9) final-round capacity (rows per bucket; the stage areas grow to match)
#define BCP_EH_CAPF 6016 // 5120 overflowed by 2-140 rows in ~12 buckets per 32 nonces (recall_base.json, round 5); 6016 keeps two final-round WGs per CU
#endif
using Cfg200_9 = EhCfg<200, 9, 9, 4416, 1024, 512, 1024, 256, 4864, 5120, 1, BCP_EH_GEN_NT, BCP_EH_GEN_HPT, BCP_EH_CAPF, 0, BCP_EH_GW>;
// (96,5): one extra pair slot per lane. ~1024 rows per bucket over 512 keys make ~1024 pairs, and
// a list of 1280 overflowed in some bucket of most nonces: 84 + 18 + 36 + ~80 pairs per 16 nonces
// in rounds 1-4, which pairs depending on the atomics' order, so a solution was lost now and then
// (tools/eh_crosscheck.py --n 96 --k 5, profiles/equihash_r6.md).
using Cfg96_5 = EhCfg<96, 5, 7, 1280, 256, 256, 256, 256, 1280, 1280, 1, 512, 2, 0, 1, 1>;
using Cfg48_5 = EhCfg<48, 5, 3, 512, 64, 8, 64, 256>; // 512-slot areas: 8 pairs per lane (a 256-pair list overflowed on duplicate-heavy nonces)

constexpr uint32_t NIL = 0xffffffffu;

// Register-resident generation (eh_gen_reg), for configs whose rows split evenly over hashes (IPH | RPW).
template <class C, int NTG, int HPT> struct GenReg {
    static constexpr int RPT = HPT * C::IPH;            // rows per thread
    static constexpr int RPW = NTG > 0 ? NTG * RPT : 1; // rows per workgroup
    static constexpr bool OK = NTG > 0 && C::INIT % RPW == 0;
    static constexpr int GWG = OK ? C::INIT / RPW : 1;  // workgroups per nonce
};

// Parent triple of a stage-s row (s >= 1): (producing bucket << 32) | (j << 16) | i; its parents
// are the stage-(s-1) slots bucket*AREA + i and bucket*AREA + j.
BCP_EH_HD inline __attribute__((always_inline)) uint64_t pack_tri(uint32_t d, uint32_t i, uint32_t j) {
    return ((uint64_t)d << 32) | (j << 16) | i;
}
// Compact parent word (EhCfg::cp): i | j << 16, the spare high bits of each half holding d's bits
// 0..DH-1 and DH..DX-1; d's bits DX.. ride in the low bits of the row's last word.
template <class C> BCP_EH_HD inline __attribute__((always_inline)) uint32_t cpack(uint32_t d, uint32_t i, uint32_t j) {
    return i | (j << 16) | ((d & C::DHM) << C::IB) | (((d >> C::DH) & C::DHM) << (16 + C::IB));
}
template <class C> BCP_EH_HD inline __attribute__((always_inline)) uint32_t cunpack_d(uint32_t pw, uint32_t lastword) {
    return ((pw >> C::IB) & C::DHM) | (((pw >> (16 + C::IB)) & C::DHM) << C::DH) | ((lastword & C::RMASK) << C::DX);
}

// LDS bytes of a round. Phase-D union `un` (bytes): {sidx[CAP] u16, bend[NRESTS] u32, then the
// pair list plist[MP*NT] u32} during the collision search; the slot -> pair table spair[MP*NT]
// u32 (aliasing plist) after it.
template <class C> constexpr int un_walk_bend(int cap) { return (cap * 2 + 3) / 4 * 4; }
template <class C> constexpr int un_walk_list(int cap) { return un_walk_bend<C>(cap) + C::NRESTS * 4; }
// Pairs per lane: one lane per LDS row slot, plus the configuration's MPX, plus BCP_EH_MP_LATE
// extra from round BCP_EH_MP_LATE_FROM on ((200,9) only): without depth-1 pruning the late rounds'
// pair lists grow past the row count (duplicate subtrees) and overflowed in round 8.
// Round threads of a round workgroup: all NT, or NT - 64*GW in a round that carries generation
// (the final round never carries: two of its workgroups share a CU and the generation tables
// would not fit).
template <class C> constexpr int round_nt(int stage, bool carry) { return carry && stage < C::K ? C::RNT : C::NT; }
template <class C> constexpr int round_mp(int stage, bool carry) {
    const int nt = round_nt<C>(stage, carry);
    return stage == C::K ? 1
                         : (C::AREA_NF + nt - 1) / nt + C::MPX +
                               (C::K == 9 && stage >= BCP_EH_MP_LATE_FROM ? BCP_EH_MP_LATE : 0);
}
template <class C> constexpr int round_un(int stage, bool carry = false) {
    const int cap = C::cap(stage);
    if (stage == C::K) return un_walk_list<C>(cap); // final round: sidx and bend only
    const int pairs = round_mp<C>(stage, carry) * round_nt<C>(stage, carry) * 4; // spair: every pair a lane may hold
    const int walk = un_walk_list<C>(cap) + pairs; // + the pair list
    return walk > pairs ? walk : pairs;
}
// (a carrying round adds the generation waves' two NB-entry tables and the round-0 prefix)
template <class C> constexpr int round_lds(int stage, bool prune, bool carry = false) {
    const int WR = C::words(stage - 1);
    const int WI = WR; // LDS words per row
    const int cap = C::cap(stage);
    const int pruneb = prune ? cap * 4 + (C::cp(stage - 1) ? 0 : (cap * 2 + 3) / 4 * 4) : 0;
    // (the final round never touches its one-word hist_, cur_ and base placeholders: the compiler drops them)
    const int hists = stage == C::K ? 0 : 2 * C::HW * 4 + (C::NB * (C::H16 ? 2 : 4) + 3) / 4 * 4;
    const int gen = carry ? 2 * C::NB * 4 + 16 * 8 : 0;
    return (cap * WI + 3) / 4 * 16 + pruneb + 4 + round_un<C>(stage, carry) + hists +
           (round_nt<C>(stage, carry) / 64 + 1) * 4 + gen;
}
// A slot round (EhCfg::ks). Its union `un` (bytes): {ktab[NRESTS][8] u16, the row ids of each key
// by rank (never cleared: reads are bounded by the key's count); bend[NRESTS] u32, the key counts;
// ovl[BCP_EH_OVL] u32, (key << 16 | row) of the rows of rank >= 8; the pair list plist[MP*NT] u32}
// during the collision search, spair aliasing plist after it. Beside `un` one more word, the
// overflow list's fill. round_lds, round_un and un_walk_* keep describing the sorted round.
template <class C> constexpr int un_slot_bend() { return C::NRESTS * 8 * 2; }
template <class C> constexpr int un_slot_ovl() { return un_slot_bend<C>() + C::NRESTS * 4; }
template <class C> constexpr int un_slot_list() { return un_slot_ovl<C>() + BCP_EH_OVL * 4; }
template <class C> constexpr int slot_un(int stage, bool carry = false) {
    return un_slot_list<C>() + round_mp<C>(stage, carry) * round_nt<C>(stage, carry) * 4;
}
template <class C> constexpr int slot_lds(int stage, bool prune, bool carry = false) {
    const int b = round_lds<C>(stage, prune, carry) - round_un<C>(stage, carry) + slot_un<C>(stage, carry) + 4;
    return carry ? (b + 7) / 8 * 8 : b; // (the generation waves' 8-byte round-0 prefix words come last)
}
// Workgroup barriers of one bucket iteration, by round variant: the count and the barrier that
// ends the pair listing, the pair filter, the first of the destination scan's two, the pair sort
// (the emit ends with the last one). The sorted round has three more before the listing: the key
// scan's two and the key placement's. eh_round and eh_carry_gen both take them from here.
struct EhBars {
    int n, list, filter, scan, sort;
};
constexpr EhBars eh_bars(bool slot) { return slot ? EhBars{7, 2, 3, 4, 6} : EhBars{10, 5, 6, 7, 9}; }
// Depth-1 duplicate pruning wherever its parent words fit next to the full rows.
template <class C> constexpr bool round_prunes(int stage, bool carry) {
    // (the pruning start was measured on (200,9); the small configurations keep pruning from round 2)
    constexpr int from = C::K == 9 ? BCP_EH_PRUNE_FROM : 2;
    return (stage >= from || stage == C::K) && stage >= 2 && round_lds<C>(stage, true, carry) <= C::LDS_BUDGET;
}

template <class C> constexpr bool slot_round_fits(int stage) {
    return slot_lds<C>(stage, round_prunes<C>(stage, false), false) <= C::LDS_BUDGET &&
           (C::GW == 0 || slot_lds<C>(stage, round_prunes<C>(stage, true), true) <= C::LDS_BUDGET);
}

// The geometry of one instantiation of the round kernel, eh_round<C, STAGE, *, CARRY>: what the
// kernel, its phase functions, the generation waves it carries (eh_carry_gen) and the host launch
// read. STAGE < K: the collision round producing stage STAGE; STAGE == K: the final round.
template <class C, int STAGE_, bool CARRY_> struct EhRoundGeom {
    using Cfg = C;
    static constexpr int STAGE = STAGE_;
    static constexpr bool CARRY = CARRY_;
    static constexpr bool FINAL = STAGE == C::K;
    static constexpr int WI = C::words(STAGE - 1);             // words per input row (LDS words per row)
    static constexpr int WO = FINAL ? 1 : C::words(STAGE);     // words per output row
    static constexpr int CAP = C::cap(STAGE);                  // LDS rows
    static constexpr bool PRUNE = round_prunes<C>(STAGE, CARRY);
    static constexpr bool SLOT = C::ks(STAGE) > 0;             // slot round: key slots filled at the commit, no key sort
    static constexpr EhBars BAR = eh_bars(SLOT);
    static constexpr int NBAR = BAR.n;                         // workgroup barriers per bucket, round and generation waves alike
    static constexpr int NT = round_nt<C>(STAGE, CARRY);       // round threads
    static constexpr int RPL = (CAP + NT - 1) / NT;            // prefetched rows per lane
    static constexpr int MP = round_mp<C>(STAGE, CARRY);       // pairs per lane (registers)
    static constexpr int NPAIR = MP * NT;                      // pair-list entries
    static constexpr int SWI = C::sw(STAGE - 1);               // words per input slot
    static constexpr int SWO = FINAL ? 1 : C::sw(STAGE);       // words per output slot
    static constexpr bool TPO = !FINAL && C::tp(STAGE);        // output stage keeps its parents in tables (Pout, Bout)
    static constexpr int PTW = TPO ? C::ptab(STAGE) : 1;       // pair-table words per producing bucket
    static constexpr bool CPI = C::cp(STAGE - 1);              // input slots carry one compact parent word
    static constexpr uint32_t RMI = C::rmask(STAGE - 1);       // parent bits in the input rows' padding
    static constexpr uint32_t RMO = C::rmask(STAGE);           // ... and in the output rows'
    static constexpr uint32_t OCAP = C::cap(FINAL ? C::K : STAGE + 1); // capacity of the round that reads the output
    static constexpr int SLI = (RPL + BCP_EH_PF_SLICES - 1) / BCP_EH_PF_SLICES; // prefetch slice (rows per phase)
    static constexpr int BPT = (C::NB + NT - 1) / NT;          // destination buckets per thread (claims)
    static constexpr int LWI = PRUNE ? (CPI ? WI + 1 : WI + 2) : WI; // words loaded per slot: a round that does not prune loads the row alone
    static constexpr int OVL = BCP_EH_OVL;                     // slot round: overflow list entries
    using HT = std::conditional_t<C::H16, uint16_t, uint32_t>; // histogram / run-base entry
    // the LDS arrays beside the union, as eh_round declares them and its phases take them
    using Rows = uint32_t[(CAP * WI + 3) / 4 * 4];
    using Psig = uint32_t[PRUNE ? CAP : 1];                    // the input rows' parent word (pruning round)
    using Pdw = uint16_t[PRUNE && !CPI ? CAP : 1];             // two-word parents: the producing bucket
    using Hist = uint32_t[FINAL ? 1 : C::HW];                  // H16: two 16-bit counters per word
    using Base = HT[FINAL ? 1 : C::NB];
    using Wsum = uint32_t[NT / 64 + 1];
    // the phase-D union: its bytes and the offsets of bend, ovl (slot round only) and plist inside it
    static constexpr int UN_BYTES = SLOT ? slot_un<C>(STAGE, CARRY) : round_un<C>(STAGE, CARRY);
    static constexpr int UN_BEND = SLOT ? un_slot_bend<C>() : un_walk_bend<C>(CAP);
    static constexpr int UN_OVL = un_slot_ovl<C>();
    static constexpr int UN_PLIST = SLOT ? un_slot_list<C>() : un_walk_list<C>(CAP);
    static constexpr int LDS_BYTES = SLOT ? slot_lds<C>(STAGE, PRUNE, CARRY) : round_lds<C>(STAGE, PRUNE, CARRY);

    static_assert(!CARRY || (C::GW > 0 && !FINAL), "only collision rounds carry generation");
    static_assert(PRUNE == round_prunes<C>(STAGE), "a carrying round prunes like the plain one");
    static_assert(LDS_BYTES <= C::LDS_BUDGET, "round LDS budget");
    static_assert(!CARRY || NT / 64 > 1, "block_exscan runs its two barriers only with more than one wave");
    static_assert(!TPO || PTW >= NPAIR, "the pair table holds every ordinal this round's emit can have (the spair bound)");
    static_assert(!(PRUNE && C::tp(STAGE - 1)), "a pruning round reads its parents from the slots");
    static_assert(FINAL || SLOT || UN_BYTES >= UN_PLIST + NPAIR * 4, "the union holds sidx, bend and this round's MP * NT pairs");
    static_assert(!SLOT || (UN_BYTES >= UN_PLIST + NPAIR * 4 && OVL <= NT && CAP < 0x4000),
                  "the union holds ktab, bend, ovl and this round's MP * NT pairs; one lane per overflow entry; ranks below the flags");
};

// Generation carried by the collision rounds of the previous nonce group. The (K-1)*NB bucket
// iterations that rounds 1..K-1 spend on a nonce hash that nonce's partner in the next group:
// bucket d of round S generates chunk (S-1)*NB + d, CH consecutive hashes, HB per generation thread.
template <class C> struct GenCarry {
    static constexpr int GT = C::GW > 0 ? 64 * C::GW : 64;       // generation threads
    static constexpr int NHASH = (C::INIT + C::IPH - 1) / C::IPH; // hashes per nonce
    static constexpr int ITERS = (C::K - 1) * C::NB;
    static constexpr int HB = ((NHASH + ITERS - 1) / ITERS + GT - 1) / GT;
    static constexpr int CH = HB * GT;
    static constexpr int RPT = HB * C::IPH;                       // rows per thread per chunk
    static constexpr int BPT = (C::NB + GT - 1) / GT;             // run claims per thread
    static_assert((long long)CH * ITERS >= NHASH, "the carrying rounds cover every hash");
};

// The parent triple of a slot, decoded on the host as eh_expand decodes it on the device.
// A stage without table parents: `slot` is the whole slot, the row and then the compact word
// (cp) or the (j << 16 | i) and d words.
template <class C> BCP_EH_HD inline uint64_t slot_parent(int stage, const uint32_t* slot) {
    const uint32_t* q = slot + C::words(stage);
    if (C::cp(stage)) return ((uint64_t)cunpack_d<C>(q[0], q[-1]) << 32) | (q[0] & C::IMASK);
    return ((uint64_t)q[1] << 32) | q[0];
}
// A stage with table parents: `row` is the slot at position pos of area `area`, btab and ptab the
// nonce's run-base and pair tables of the stage. d comes from the row's padding through tpmask,
// the slot's ordinal in d's emit is pos - B[d][area], and the pair word is P[d][ordinal]. A d or
// an ordinal outside its table (eh_expand rejects the candidate) clears *in_range, and the pair
// word returned is NIL: i = j = 0xffff, no LDS row.
template <class C>
BCP_EH_HD inline uint64_t table_parent(int stage, const uint32_t* row, uint32_t area, uint32_t pos,
                                       const uint32_t* btab_of_nonce, const uint32_t* ptab_of_nonce, bool* in_range) {
    const uint32_t d = row[C::words(stage) - 1] & C::tpmask(stage);
    const uint32_t o = d < (uint32_t)C::NB ? pos - btab_of_nonce[(size_t)d * C::NB + area] : NIL;
    *in_range = d < (uint32_t)C::NB && o < (uint32_t)C::ptab(stage);
    return ((uint64_t)d << 32) | (*in_range ? ptab_of_nonce[(size_t)d * C::ptab(stage) + o] : NIL);
}

} // namespace bcpk

namespace bcp {
namespace gpu {

template <class F> static void dispatch_cfg(unsigned n, unsigned k, F&& f) {
    if (n == 200 && k == 9) f(bcpk::Cfg200_9{});
    else if (n == 96 && k == 5) f(bcpk::Cfg96_5{});
    else if (n == 48 && k == 5) f(bcpk::Cfg48_5{});
    else throw std::invalid_argument("EquihashGpuSolver: unsupported (N,K); GPU supports (200,9),(96,5),(48,5)");
}

} // namespace gpu
} // namespace bcp

#endif // BCP_KERNELS_EQUIHASH_LAYOUT_H
