// Coin selection for CDNA4: the stochastic subset search behind CWallet::SelectCoinsMinConf
// (reference src/wallet/wallet.cpp ApproximateBestSubset) with its trials side by side.
//   K13 coin_select_kernel: one lane per trial, every lane of a wave at the same coin of the same
//       pass. The trial code is kernels/coin_select.h, compiled here for the device and in
//       csrc/wallet/coinselect.cpp for the host, so both pick the same candidate.
//       coin_select_final_kernel: the smallest of the waves' candidates, one wave per run.
// A latency kernel: 1000 trials are 16 waves, each a workgroup of its own, so each gets a SIMD
// and a scalar cache to itself; nothing here tries to fill the device. A trial is a chain of
// dependent 64-bit adds and compares (VGPR pairs, v_cndmask for the candidate), one SipHash word
// per 64 coins per lane. The amounts are read at wave-uniform addresses (the coin index and the
// pointer are the same in every lane), so they come through the scalar cache, sixteen at a time,
// and cost the vector pipe nothing; no LDS staging and no barrier. The order (total, trial,
// pass, coin) is kept exactly: lanes compare whole candidates by butterfly shuffles, lane 0 of
// each wave writes the wave's to its own slot, and the second kernel reduces the slots the same
// way. No atomics anywhere, so nothing depends on which wave finishes first.
#include <hip/hip_runtime.h>

#include "kernels/coin_select.h"
#include "kernels/gpu_api.h"
#include "kernels/hip_util.h"
#include "kernels/relay_ctx.h"

#include <cstring>
#include <mutex>
#include <stdexcept>

namespace bcpk {

using namespace bcp::cs;

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t x, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, mask, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), mask, 64);
    return ((uint64_t)hi << 32) | lo;
}
// every lane ends with the smallest candidate of the wave
__device__ __forceinline__ Cand wave_min(Cand c) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const Cand o{shfl_xor_u64(c.total, m), shfl_xor_u64(c.key, m)};
        if (Less(o, c)) c = o;
    }
    return c;
}

// Wave blockIdx.x of run firstRun + blockIdx.y: trials 64 * blockIdx.x + lane at target0 (run slot
// 0) or target1 (slot 1). partial[2 * (blockIdx.y * gridDim.x + blockIdx.x) ..] = the wave's
// smallest candidate (total, key). Lanes past `trials` carry no candidate.
__global__ __launch_bounds__(64) void coin_select_kernel(const int64_t* __restrict__ values, uint32_t n, int64_t target0,
                                                         int64_t target1, uint32_t firstRun, uint32_t trials, uint64_t k0,
                                                         uint64_t k1, uint64_t* __restrict__ partial) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    const int64_t target = blockIdx.y ? target1 : target0;
    Cand c{CS_NONE, CS_NONE};
    if (t < trials) c = RunTrial(values, n, target, k0, k1 + firstRun + blockIdx.y, t);
    c = wave_min(c);
    if (threadIdx.x == 0) {
        uint64_t* p = partial + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        p[0] = c.total;
        p[1] = c.key;
    }
}

// out[4 * run ..] = (total, trial, pass, coin) of the smallest of run blockIdx.x's nPartial
// candidates, all -1 when there is none.
__global__ __launch_bounds__(64) void coin_select_final_kernel(const uint64_t* __restrict__ partial, uint32_t nPartial,
                                                               int64_t* __restrict__ out) {
    const uint64_t* p = partial + 2 * (size_t)blockIdx.x * nPartial;
    Cand c{CS_NONE, CS_NONE};
    for (uint32_t i = threadIdx.x; i < nPartial; i += 64) {
        const Cand o{p[2 * i], p[2 * i + 1]};
        if (Less(o, c)) c = o;
    }
    c = wave_min(c);
    if (threadIdx.x == 0) {
        int64_t* o = out + 4 * (size_t)blockIdx.x;
        const bool none = c.key == CS_NONE;
        o[0] = none ? -1 : (int64_t)c.total;
        o[1] = none ? -1 : (int64_t)TrialOf(c.key);
        o[2] = none ? -1 : (int64_t)PassOf(c.key);
        o[3] = none ? -1 : (int64_t)CoinOf(c.key);
    }
}

} // namespace bcpk

namespace bcp {
namespace gpu {

namespace {
void CheckCoinSelect(size_t n, const int64_t* targets, unsigned firstRun, unsigned nRuns, uint32_t trials) {
    if (!n || n > cs::CS_MAX_COINS) throw std::invalid_argument("coin select: 1..2^31 coins");
    if (!trials || trials > cs::CS_MAX_TRIALS) throw std::invalid_argument("coin select: 1..65536 trials");
    if (nRuns < 1 || nRuns > 2 || firstRun + nRuns > 2) throw std::invalid_argument("coin select: runs are 0 and 1");
    for (unsigned r = 0; r < nRuns; ++r)
        if (targets[r] <= 0) throw std::invalid_argument("coin select: target not above 0");
}
uint32_t Waves(uint32_t trials) { return (trials + 63) / 64; }
void LaunchCoinSelect(hipStream_t s, const int64_t* d_values, size_t n, const int64_t* targets, unsigned firstRun,
                      unsigned nRuns, uint32_t trials, uint64_t k0, uint64_t k1, uint64_t* d_partial, int64_t* d_out) {
    const uint32_t waves = Waves(trials);
    hipLaunchKernelGGL(bcpk::coin_select_kernel, dim3(waves, nRuns), dim3(64), 0, s, d_values, (uint32_t)n, targets[0],
                       nRuns > 1 ? targets[1] : targets[0], firstRun, trials, k0, k1, d_partial);
    BCP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bcpk::coin_select_final_kernel, dim3(nRuns), dim3(64), 0, s, d_partial, waves, d_out);
    BCP_HIP_CHECK(hipGetLastError());
}
} // namespace

size_t CoinSelectScratchBytes(uint32_t trials, unsigned nRuns) { return (size_t)Waves(trials) * nRuns * 16; }

void CoinSelectBatch(const int64_t* values, size_t n, const int64_t* targets, unsigned firstRun, unsigned nRuns,
                     uint32_t trials, uint64_t k0, uint64_t k1, CoinSelectRun* out, int device) {
    CheckCoinSelect(n, targets, firstRun, nRuns, trials);
    uint64_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        if (values[i] <= 0) throw std::invalid_argument("coin select: amount not above 0");
        sum += (uint64_t)values[i];
        if (sum >> 63) throw std::invalid_argument("coin select: the amounts sum to 2^63 or more");
    }
    device = UseDevice(device);
    RelayCtx& c = Ctx(device);
    auto l = Lock(c);
    const size_t scratch = CoinSelectScratchBytes(trials, nRuns), outBytes = (size_t)nRuns * sizeof(CoinSelectRun);
    unsigned char* h_in = c.st.Host(0, n * 8);
    unsigned char* d_in = c.st.Dev(0, n * 8);
    unsigned char* h_out = c.st.Host(1, outBytes);
    unsigned char* d_out = c.st.Dev(1, scratch + outBytes);
    memcpy(h_in, values, n * 8);
    try {
        BCP_HIP_CHECK(hipMemcpyAsync(d_in, h_in, n * 8, hipMemcpyHostToDevice, c.s));
        LaunchCoinSelect(c.s, reinterpret_cast<const int64_t*>(d_in), n, targets, firstRun, nRuns, trials, k0, k1,
                         reinterpret_cast<uint64_t*>(d_out), reinterpret_cast<int64_t*>(d_out + scratch));
        BCP_HIP_CHECK(hipMemcpyAsync(h_out, d_out + scratch, outBytes, hipMemcpyDeviceToHost, c.s));
        BCP_HIP_CHECK(hipStreamSynchronize(c.s));
    } catch (...) {
        (void)hipStreamSynchronize(c.s); // nothing may still read the pinned staging
        throw;
    }
    memcpy(out, h_out, outBytes);
}

void CoinSelectDevice(const void* values, size_t n, const int64_t* targets, unsigned firstRun, unsigned nRuns,
                      uint32_t trials, uint64_t k0, uint64_t k1, void* scratch, void* out, int device, uintptr_t stream) {
    CheckCoinSelect(n, targets, firstRun, nRuns, trials);
    if (reinterpret_cast<uintptr_t>(values) % 8 || reinterpret_cast<uintptr_t>(scratch) % 8 ||
        reinterpret_cast<uintptr_t>(out) % 8)
        throw std::invalid_argument("CoinSelectDevice: values, scratch or out not 8-byte aligned");
    DeviceScope ds(device);
    LaunchCoinSelect(reinterpret_cast<hipStream_t>(stream), static_cast<const int64_t*>(values), n, targets, firstRun,
                     nRuns, trials, k0, k1, static_cast<uint64_t*>(scratch), static_cast<int64_t*>(out));
}

} // namespace gpu
} // namespace bcp
