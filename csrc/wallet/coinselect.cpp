// The batched subset search of the wallet's coin selection: host twin, device call, dispatch.
#include "wallet/coinselect.h"

#include "kernels/coin_select.h"
#include "kernels/gpu_api.h"
#include "keys/key.h"
#include "util/util.h"

#include <algorithm>
#include <atomic>
#include <limits>
#include <stdexcept>

namespace bcp {

namespace {

std::atomic<size_t> g_threshold{DEFAULT_GPU_COIN_SELECT_THRESHOLD};
std::atomic<bool> g_enabled{true}, g_twinOnly{false};
std::atomic<int> g_consecutiveFailures{0};
std::atomic<uint64_t> g_gpuSelections{0}, g_cpuSelections{0}, g_gpuFailures{0};

bool DevicePathOpen() { return g_consecutiveFailures.load() < 3 && (GpuFaultInjection() || gpu::GpuAvailable()); }

void CheckArgs(const Amount* values, size_t n, Amount target, uint32_t trials, unsigned run) {
    if (!n || n > cs::CS_MAX_COINS) throw std::invalid_argument("coin select: 1..2^31 coins");
    if (!trials || trials > cs::CS_MAX_TRIALS) throw std::invalid_argument("coin select: 1..65536 trials");
    if (run > 1) throw std::invalid_argument("coin select: runs are 0 and 1");
    if (target <= 0) throw std::invalid_argument("coin select: target not above 0");
    uint64_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        if (values[i] <= 0) throw std::invalid_argument("coin select: amount not above 0");
        sum += (uint64_t)values[i];
        if (sum >> 63) throw std::invalid_argument("coin select: the amounts sum to 2^63 or more");
    }
}

CoinSelectPick PickOf(const cs::Cand& c) {
    CoinSelectPick p;
    if (c.key == cs::CS_NONE) return p;
    p.found = true;
    p.total = (Amount)c.total;
    p.trial = cs::TrialOf(c.key);
    p.pass = cs::PassOf(c.key);
    p.index = cs::CoinOf(c.key);
    return p;
}

} // namespace

CoinSelectPick CoinSelectCpu(const Amount* values, size_t n, Amount target, uint32_t trials, uint64_t k0, uint64_t k1,
                             unsigned run) {
    CheckArgs(values, n, target, trials, run);
    cs::Cand best{cs::CS_NONE, cs::CS_NONE};
    for (uint32_t t = 0; t < trials; ++t) {
        const cs::Cand c = cs::RunTrial(values, (uint32_t)n, target, k0, k1 + run, t);
        if (cs::Less(c, best)) best = c;
        if (best.total == (uint64_t)target) break;
    }
    return PickOf(best);
}

void CoinSelectGpu(const Amount* values, size_t n, const Amount* targets, unsigned firstRun, unsigned nRuns,
                   uint32_t trials, uint64_t k0, uint64_t k1, CoinSelectPick* out, int device) {
    gpu::CoinSelectRun r[2];
    if (nRuns < 1 || nRuns > 2) throw std::invalid_argument("coin select: runs are 0 and 1");
    gpu::CoinSelectBatch(values, n, targets, firstRun, nRuns, trials, k0, k1, r, device);
    for (unsigned i = 0; i < nRuns; ++i) {
        CoinSelectPick p;
        if (r[i].total >= 0) {
            if (r[i].trial < 0 || r[i].trial >= (int64_t)trials || r[i].pass < 0 || r[i].pass > 1 || r[i].index < 0 ||
                r[i].index >= (int64_t)n || r[i].total < targets[i])
                throw std::runtime_error("coin select: the device returned a candidate out of range");
            p.found = true;
            p.total = r[i].total;
            p.trial = (uint32_t)r[i].trial;
            p.pass = (uint32_t)r[i].pass;
            p.index = (uint32_t)r[i].index;
        }
        out[i] = p;
    }
}

std::vector<uint32_t> CoinSelectReplay(const Amount* values, size_t n, Amount target, uint64_t k0, uint64_t k1,
                                       unsigned run, const CoinSelectPick& pick) {
    std::vector<uint32_t> in;
    if (!pick.found) return in;
    if (pick.index >= n || pick.pass > 1 || run > 1) throw std::invalid_argument("coin select: pick out of range");
    std::vector<char> held(n, 0);
    cs::Cand best{cs::CS_NONE, cs::CS_NONE};
    int64_t total = 0;
    for (uint32_t pass = 0; pass <= pick.pass; ++pass) {
        const uint32_t end = pass == pick.pass ? pick.index : (uint32_t)n;
        uint64_t bits = 0;
        for (uint32_t i = 0; i < end; ++i) {
            if ((i & 63) == 0) bits = cs::RandomWord(k0, k1 + run, pick.trial, i >> 6);
            const bool take = (((bits >> (i & 63)) & 1) != 0) == (pass == 0);
            if (cs::Step(total, best, values[i], take, target, cs::KeyOf(pick.trial, pass, i))) held[i] = 1;
        }
    }
    held[pick.index] = 1;
    for (uint32_t i = 0; i < n; ++i)
        if (held[i]) in.push_back(i);
    return in;
}

void SetGpuCoinSelectThreshold(size_t n) { g_threshold = n; }
size_t GetGpuCoinSelectThreshold() { return g_threshold.load(); }
void SetGpuCoinSelectEnabled(bool on) { g_enabled = on; }
void SetCoinSelectTwinOnly(bool on) { g_twinOnly = on; }
bool GpuCoinSelectWanted(size_t n, bool* allowGpu) {
    const size_t th = g_threshold.load();
    const bool twin = g_twinOnly.load();
    if (allowGpu) *allowGpu = !twin;
    return th != 0 && n >= th && n <= cs::CS_MAX_COINS && (twin || (g_enabled.load() && DevicePathOpen()));
}
CoinSelectStats GetCoinSelectStats() {
    CoinSelectStats s;
    s.gpu_selections = g_gpuSelections;
    s.cpu_selections = g_cpuSelections;
    s.gpu_failures = g_gpuFailures;
    return s;
}
void ResetCoinSelectFailures() { g_consecutiveFailures = 0; }

void ApproximateBestSubsetBatched(const std::vector<Amount>& values, Amount nTotalLower, Amount nTargetValue,
                                  Amount minChange, bool allowGpu, std::vector<char>& vfBest, Amount& nBest, int iterations,
                                  CoinSelectInfo* info) {
    const size_t n = values.size();
    const uint32_t trials = (uint32_t)std::max(1, std::min(iterations, (int)cs::CS_MAX_TRIALS));
    const bool second = minChange > 0 && nTotalLower >= nTargetValue + minChange;
    const Amount targets[2] = {nTargetValue, nTargetValue + minChange};
    CoinSelectInfo I;
    I.k0 = GetRand(std::numeric_limits<uint64_t>::max());
    I.k1 = GetRand(std::numeric_limits<uint64_t>::max());
    CoinSelectPick picks[2];
    bool have[2] = {false, false};
    if (allowGpu && DevicePathOpen()) {
        try {
            if (GpuFaultInjection()) throw std::runtime_error("injected GPU coin-selection fault");
            CoinSelectGpu(values.data(), n, targets, 0, second ? 2 : 1, trials, I.k0, I.k1, picks);
            have[0] = true;
            have[1] = second;
            I.usedGpu = true;
            g_consecutiveFailures = 0;
        } catch (const std::exception& e) {
            const int f = ++g_consecutiveFailures;
            g_gpuFailures++;
            I.fellBack = true;
            LogPrintf("GPU coin selection failed (%s); searching %zu coins on the CPU%s\n", e.what(), n,
                      f >= 3 ? " (GPU path now disabled)" : "");
        }
    }
    if (!have[0]) picks[0] = CoinSelectCpu(values.data(), n, targets[0], trials, I.k0, I.k1, 0);
    I.run = (second && !(picks[0].found && picks[0].total == nTargetValue)) ? 1 : 0;
    if (I.run == 1 && !have[1]) picks[1] = CoinSelectCpu(values.data(), n, targets[1], trials, I.k0, I.k1, 1);
    (I.usedGpu ? g_gpuSelections : g_cpuSelections)++;
    I.pick = picks[I.run];
    // as the reference's loop starts out: every coin, their sum
    vfBest.assign(n, true);
    nBest = nTotalLower;
    if (I.pick.found && I.pick.total < nTotalLower) {
        vfBest.assign(n, false);
        for (uint32_t i : CoinSelectReplay(values.data(), n, targets[I.run], I.k0, I.k1, I.run, I.pick)) vfBest[i] = true;
        nBest = I.pick.total;
    }
    if (info) *info = I;
}

} // namespace bcp
