// The batched subset search of the wallet's coin selection (wallet/coinselect.h): the host twin of
// coin_select_kernel against the reference's loop (src/wallet/wallet.cpp ApproximateBestSubset)
// rewritten to keep its vfIncluded bitmap and fed the same bits, and SelectCoinsMinConf's
// contract (reference src/wallet/test/wallet_tests.cpp coin_selection_tests) on lists at or
// above -gpucoinselectthreshold.
#include "test/unittest.h"
#include "kernels/coin_select.h"
#include "wallet/coinselect.h"
#include "wallet/wallet.h"

#include <algorithm>
#include <deque>
#include <numeric>
#include <random>
#include <set>

namespace bcp {
namespace {

struct BitmapResult {
    bool found = false;
    Amount best = 0;
    uint32_t trial = 0, pass = 0, index = 0;
    std::vector<char> vfBest;
};
// ApproximateBestSubset as the reference writes it, vfIncluded and all; only the source of the
// bits differs (the counter-based words instead of one stream), and the first candidate to reach
// a total is remembered by where it was found.
BitmapResult BitmapLoop(const std::vector<Amount>& v, Amount target, uint32_t trials, uint64_t k0, uint64_t k1, unsigned run) {
    BitmapResult r;
    std::vector<char> vfIncluded;
    for (uint32_t rep = 0; rep < trials && !(r.found && r.best == target); rep++) {
        vfIncluded.assign(v.size(), false);
        Amount nTotal = 0;
        bool fReachedTarget = false;
        for (uint32_t pass = 0; pass < 2 && !fReachedTarget; pass++) {
            for (size_t i = 0; i < v.size(); i++) {
                const bool bit = (cs::RandomWord(k0, k1 + run, rep, (uint32_t)(i >> 6)) >> (i & 63)) & 1;
                if (pass == 0 ? bit : !vfIncluded[i]) {
                    nTotal += v[i];
                    vfIncluded[i] = true;
                    if (nTotal >= target) {
                        fReachedTarget = true;
                        if (!r.found || nTotal < r.best) {
                            r.found = true;
                            r.best = nTotal;
                            r.vfBest = vfIncluded;
                            r.trial = rep;
                            r.pass = pass;
                            r.index = (uint32_t)i;
                        }
                        nTotal -= v[i];
                        vfIncluded[i] = false;
                    }
                }
            }
        }
    }
    return r;
}

std::vector<Amount> RandomAmounts(std::mt19937_64& rng, size_t n, Amount top) {
    std::vector<Amount> v(n);
    for (Amount& a : v) a = 1 + (Amount)(rng() % (uint64_t)top);
    std::sort(v.begin(), v.end(), std::greater<Amount>());
    return v;
}

typedef std::set<std::pair<const CWalletTx*, unsigned int>> CoinSet;
struct Pool {
    CWallet wallet{"test", "", true};
    std::deque<CWalletTx> txs;
    std::vector<COutput> coins;
    uint32_t lockTime = 0;
    void Add(Amount v) {
        CMutableTransaction t;
        t.nLockTime = lockTime++;
        t.vout.push_back(CTxOut(v, CScript() << OP_TRUE));
        txs.emplace_back(&wallet, MakeTransactionRef(std::move(t)));
        coins.push_back({&txs.back(), 0, 144, true, true});
    }
    bool Select(Amount target, CoinSet& set, Amount& value) {
        return wallet.SelectCoinsMinConf(target, 1, 6, 0, coins, set, value);
    }
};
// the batched search from one coin up, on the twin: no device is needed
struct BatchedSelection {
    size_t threshold = GetGpuCoinSelectThreshold();
    BatchedSelection() {
        SetGpuCoinSelectThreshold(1);
        SetCoinSelectTwinOnly(true);
    }
    ~BatchedSelection() {
        SetCoinSelectTwinOnly(false);
        SetGpuCoinSelectThreshold(threshold);
    }
};
Amount SumOf(const CoinSet& s) {
    Amount t = 0;
    for (const auto& c : s) t += c.first->tx->vout[c.second].nValue;
    return t;
}

} // namespace

TEST_CASE(coinselect_tests, twin_equals_bitmap_loop) {
    std::mt19937_64 rng(20260101);
    for (size_t n : {1, 2, 5, 63, 64, 65, 130, 300}) {
        for (int shape = 0; shape < 6; shape++) {
            std::vector<Amount> v = shape == 4 ? std::vector<Amount>(n, 7) : RandomAmounts(rng, n, shape == 5 ? 4 : 100000000);
            const Amount sum = std::accumulate(v.begin(), v.end(), (Amount)0);
            Amount target;
            switch (shape) {
            case 0: target = std::max<Amount>(1, sum / 3); break;
            case 1: target = std::max<Amount>(1, sum - v.back()); break; // pass 0 cannot reach it: pass 1 decides
            case 2: target = sum; break;
            case 3: target = sum + 1; break;                             // out of reach
            default: target = std::max<Amount>(1, sum / 2); break;       // equal and tiny amounts: ties
            }
            const uint64_t k0 = rng(), k1 = shape == 2 ? ~0ULL : rng();
            for (unsigned run = 0; run < 2; run++) {
                const uint32_t trials = n > 100 ? 40 : 200;
                const CoinSelectPick p = CoinSelectCpu(v.data(), n, target, trials, k0, k1, run);
                const BitmapResult b = BitmapLoop(v, target, trials, k0, k1, run);
                CHECK_EQ(p.found, b.found);
                CHECK_EQ(p.found, sum >= target);
                if (!p.found || !b.found) continue;
                CHECK_EQ(p.total, b.best);
                CHECK_EQ(p.trial, b.trial);
                CHECK_EQ(p.pass, b.pass);
                CHECK_EQ(p.index, b.index);
                // the replay rebuilds the bitmap the loop kept
                std::vector<char> replayed(n, false);
                for (uint32_t i : CoinSelectReplay(v.data(), n, target, k0, k1, run, p)) replayed[i] = true;
                CHECK(replayed == b.vfBest);
                if (shape == 1 && n >= 63) CHECK_EQ(p.pass, 1u);
            }
        }
    }
}

TEST_CASE(coinselect_tests, batched_subset_matches_its_pick) {
    std::mt19937_64 rng(7);
    const std::vector<Amount> v = RandomAmounts(rng, 500, 50 * CENT);
    const Amount sum = std::accumulate(v.begin(), v.end(), (Amount)0);
    for (Amount target : {sum / 7, sum / 2, sum - MIN_CHANGE / 2, sum - 1}) {
        std::vector<char> vfBest;
        Amount nBest = 0;
        CoinSelectInfo info;
        ApproximateBestSubsetBatched(v, sum, target, MIN_CHANGE, false, vfBest, nBest, 1000, &info);
        CHECK(!info.usedGpu && !info.fellBack);
        CHECK_EQ(vfBest.size(), v.size());
        Amount got = 0;
        for (size_t i = 0; i < v.size(); i++)
            if (vfBest[i]) got += v[i];
        CHECK_EQ(got, nBest);
        CHECK(nBest >= target);
        // run 1 is taken exactly when run 0 missed the target and the coins allow for change
        const bool second = sum >= target + MIN_CHANGE;
        const CoinSelectPick p0 = CoinSelectCpu(v.data(), v.size(), target, 1000, info.k0, info.k1, 0);
        CHECK_EQ(info.run, (second && p0.total != target) ? 1u : 0u);
        if (info.run == 1) {
            CHECK(nBest >= target + MIN_CHANGE);
            CHECK(info.pick == CoinSelectCpu(v.data(), v.size(), target + MIN_CHANGE, 1000, info.k0, info.k1, 1));
        } else {
            CHECK(info.pick == p0);
        }
    }
}

// reference coin_selection_tests, on lists the wallet hands to the batched search
TEST_CASE(coinselect_tests, select_coins_min_conf_above_threshold) {
    BatchedSelection batched;
    const CoinSelectStats before = GetCoinSelectStats();
    for (int rep = 0; rep < 20; rep++) {
        Pool p;
        CoinSet set;
        Amount v = 0;
        for (int c : {3, 4, 9, 25, 50}) p.Add(c * CENT);
        // an exact subset of the small coins: 3 + 4
        CHECK(p.Select(7 * CENT, set, v));
        CHECK_EQ(v, 7 * CENT);
        CHECK_EQ(set.size(), (size_t)2);
        // 20: the small coins (3+4+9 = 16) cannot reach it, so the smallest larger coin
        CHECK(p.Select(20 * CENT, set, v));
        CHECK_EQ(v, 25 * CENT);
        CHECK_EQ(set.size(), (size_t)1);
        // 15: 3+4+9 = 16 beats the next larger coin (25)
        CHECK(p.Select(15 * CENT, set, v));
        CHECK_EQ(v, 16 * CENT);
        CHECK_EQ(set.size(), (size_t)3);
        p.Add(16 * CENT);
        // now a single 16 ties with 3+4+9: the single larger coin wins a tie
        CHECK(p.Select(15 * CENT, set, v));
        CHECK_EQ(v, 16 * CENT);
        CHECK_EQ(set.size(), (size_t)1);
        // everything, and not a satoshi more
        CHECK(p.Select(107 * CENT, set, v));
        CHECK_EQ(v, 107 * CENT);
        CHECK(!p.Select(107 * CENT + 1, set, v));
    }
    // a long list: an exact match is found when one exists, and the result covers the target
    std::mt19937_64 rng(99);
    Pool p;
    for (int i = 0; i < 3000; i++) p.Add(CENT + (Amount)(rng() % (uint64_t)(10 * CENT)));
    for (int i = 0; i < 40; i++) p.Add(COIN); // equal coins: 7 of them make the target below exactly
    p.Add(500 * COIN);
    CoinSet set;
    Amount v = 0;
    CHECK(p.Select(7 * COIN, set, v));
    CHECK_EQ(v, 7 * COIN);
    CHECK_EQ(SumOf(set), v);
    CHECK_EQ(set.size(), (size_t)7);
    for (int rep = 0; rep < 5; rep++) {
        const Amount target = COIN + (Amount)(rng() % (uint64_t)(100 * COIN));
        CHECK(p.Select(target, set, v));
        CHECK(v >= target);
        CHECK_EQ(SumOf(set), v);
        // either the target exactly, or enough change to be worth an output
        CHECK(v == target || v >= target + MIN_CHANGE);
    }
    const CoinSelectStats after = GetCoinSelectStats();
    CHECK(after.cpu_selections > before.cpu_selections);
    CHECK_EQ(after.gpu_selections, before.gpu_selections);
    CHECK_EQ(after.gpu_failures, before.gpu_failures);
}

TEST_CASE(coinselect_tests, threshold_and_switches) {
    const size_t keep = GetGpuCoinSelectThreshold();
    CHECK(DEFAULT_GPU_COIN_SELECT_THRESHOLD == 0 || DEFAULT_GPU_COIN_SELECT_THRESHOLD >= 2048);
    bool allowGpu = true;
    SetCoinSelectTwinOnly(true);
    SetGpuCoinSelectThreshold(0);
    CHECK(!GpuCoinSelectWanted(1000000, &allowGpu)); // 0: never
    SetGpuCoinSelectThreshold(100);
    CHECK(!GpuCoinSelectWanted(99, &allowGpu));
    CHECK(GpuCoinSelectWanted(100, &allowGpu));
    CHECK(!allowGpu);
    SetCoinSelectTwinOnly(false);
    SetGpuCoinSelectEnabled(false); // -gpu=0 keeps the old loop
    CHECK(!GpuCoinSelectWanted(100, &allowGpu));
    SetGpuCoinSelectEnabled(true);
    SetGpuCoinSelectThreshold(keep);
}

} // namespace bcp
