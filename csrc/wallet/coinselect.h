// The stochastic subset search of CWallet::SelectCoinsMinConf with its trials side by side
// (kernels/coin_select.h): on the device one lane per trial (csrc/kernels/coin_select.hip
// coin_select_kernel), the same code on the host as its twin. Below -gpucoinselectthreshold, and
// with -gpu=0, the wallet keeps the reference's serial loop (wallet.cpp ApproximateBestSubset),
// which draws its bits from one stream across the trials and so cannot be split over lanes; the
// batched search draws them from a counter (seed, run, trial, coin) instead, and searches the same
// space: independent trials, pass 0 by random bits, pass 1 over the coins pass 0 left out, the
// smallest total at or above the target wins, the earliest trial among equals.
#pragma once
#include "primitives/amount.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bcp {

// The winning candidate of a run: the total reached when coin `index` was added in pass `pass`
// of trial `trial`. found = false: the amounts sum to less than the target.
struct CoinSelectPick {
    bool found = false;
    Amount total = 0;
    uint32_t trial = 0, pass = 0, index = 0;
    bool operator==(const CoinSelectPick& o) const {
        return found == o.found && total == o.total && trial == o.trial && pass == o.pass && index == o.index;
    }
};

// Run `run` (0, or 1 for the wallet's second search) of `trials` (1..65536) trials at `target`
// over n amounts (each > 0, sum below 2^63, sorted descending) under the seed (k0, k1), on the
// host. Stops at the first trial that meets the target exactly: no later one can win.
CoinSelectPick CoinSelectCpu(const Amount* values, size_t n, Amount target, uint32_t trials, uint64_t k0, uint64_t k1,
                             unsigned run);
// The same on the device: nRuns = 1 gives run firstRun at targets[0], nRuns = 2 runs 0 and 1 at
// targets[0] and targets[1] in one launch. Throws what the device path throws.
void CoinSelectGpu(const Amount* values, size_t n, const Amount* targets, unsigned firstRun, unsigned nRuns,
                   uint32_t trials, uint64_t k0, uint64_t k1, CoinSelectPick* out, int device = -1);
// The coins of a pick, ascending: trial `pick.trial` replayed up to (pass, index); the coins it
// holds there, and coin `index`.
std::vector<uint32_t> CoinSelectReplay(const Amount* values, size_t n, Amount target, uint64_t k0, uint64_t k1,
                                       unsigned run, const CoinSelectPick& pick);

struct CoinSelectInfo {
    bool usedGpu = false;  // the search ran on the device
    bool fellBack = false; // the device path threw and the twin finished
    unsigned run = 0;      // the run whose pick was taken
    uint64_t k0 = 0, k1 = 0;
    CoinSelectPick pick;
};
// What SelectCoinsMinConf does with ApproximateBestSubset, once or twice, as one batched search:
// run 0 at nTargetValue and, when minChange > 0 and nTotalLower >= nTargetValue + minChange, run 1
// at nTargetValue + minChange, whose pick is taken iff run 0 did not meet its target exactly.
// values: the candidate amounts, sorted descending, nTotalLower their sum (>= nTargetValue).
// vfBest / nBest as ApproximateBestSubset leaves them. On the device both runs go in one launch
// when allowGpu and a device is usable; any device error is logged and the twin finishes (three
// consecutive errors turn the device path off). The seed comes from GetRand per call.
void ApproximateBestSubsetBatched(const std::vector<Amount>& values, Amount nTotalLower, Amount nTargetValue,
                                  Amount minChange, bool allowGpu, std::vector<char>& vfBest, Amount& nBest,
                                  int iterations = 1000, CoinSelectInfo* info = nullptr);

// -gpucoinselectthreshold: the smallest candidate list SelectCoinsMinConf searches this way
// (0: never). The default is derived from the measurement in profiles/coin_select.md.
static const size_t DEFAULT_GPU_COIN_SELECT_THRESHOLD = 2048;
void SetGpuCoinSelectThreshold(size_t n);
size_t GetGpuCoinSelectThreshold();
// -gpu: whether the node may use the device for this at all
void SetGpuCoinSelectEnabled(bool on);
// Take the batched search at the threshold even without a device, on the twin (unit tests and
// the benchmark's twin arm).
void SetCoinSelectTwinOnly(bool on);
// true when a list of n candidates should go through ApproximateBestSubsetBatched; allowGpu
// receives whether it may use the device
bool GpuCoinSelectWanted(size_t n, bool* allowGpu);

struct CoinSelectStats {
    uint64_t gpu_selections = 0, cpu_selections = 0, gpu_failures = 0;
};
CoinSelectStats GetCoinSelectStats();
void ResetCoinSelectFailures(); // re-enable the device path (tests)

} // namespace bcp
