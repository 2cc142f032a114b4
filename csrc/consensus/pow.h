// Proof of work: difficulty schedule and checks.
// Parity: reference src/pow.{h,cpp}
//   GetNextWorkRequired     pow.cpp:71   genesis -> powLimit(false); regtest no-retarget;
//                                        pre-fork legacy 2016-block retarget; premine window ->
//                                        powLimit; averaging window -> powLimitStart; else DAA
//   CalculateNextWorkRequired pow.cpp:105 (legacy)
//   CheckProofOfWork        pow.cpp:141  (range check against PowLimit(postfork))
//   GetNextCashPlusWorkRequired pow.cpp:252 (144-block work-weighted DAA, median-of-3)
//   CheckEquihashSolution   pow.cpp:298
#pragma once
#include "consensus/chain.h"
#include "consensus/params.h"

#include <vector>

namespace bcp {

uint32_t GetNextWorkRequired(const CBlockIndex* pindexPrev, const CBlockHeader* pblock,
                             const Consensus::Params& params);
uint32_t CalculateNextWorkRequired(const CBlockIndex* pindexPrev, int64_t nFirstBlockTime,
                                   const Consensus::Params& params);
uint32_t GetNextCashPlusWorkRequired(const CBlockIndex* pindexPrev, const CBlockHeader* pblock,
                                     const Consensus::Params& params);
bool CheckProofOfWork(const uint256& hash, uint32_t nBits, bool postfork, const Consensus::Params& params);
// The same against an explicit limit (CheckProofOfWork passes params.PowLimit(postfork)).
bool CheckProofOfWork(const uint256& hash, uint32_t nBits, const arith_uint256& powLimit);

// CPU consensus check of one header's Equihash solution.
bool CheckEquihashSolution(const CBlockHeader* pblock, const CChainParams& params);
// Batched check (GPU when available, CPU otherwise); result[i] for headers[i].
std::vector<bool> CheckEquihashSolutions(const std::vector<const CBlockHeader*>& headers, const CChainParams& params,
                                         bool allow_gpu = true);

// The whole of CheckBlockHeader for one post-fork header of a batch.
struct HeaderCheck {
    bool solutionOk = false; // CheckEquihashSolution
    bool powOk = false;      // CheckProofOfWork(hash, nBits, postfork = true)
    bool hashKnown = false;  // `hash` is set (always, for every header of a returned batch)
    bool fromDevice = false; // hash and powOk were computed on the GPU
    uint256 hash;            // GetHash()
};
// Batched CheckBlockHeader of post-fork headers: solution, hash and proof of work. With a GPU
// (>= 4 headers, a parameter set the device hashes) one device pass computes all three from the
// bytes uploaded for the solution check; a header whose solution has another length is hashed on
// the CPU. GPU failures are handled as in CheckEquihashSolutions (log, redo on the CPU, three in
// a row disable the path).
std::vector<HeaderCheck> CheckBlockHeaders(const std::vector<const CBlockHeader*>& headers, const CChainParams& params,
                                           bool allow_gpu = true);

} // namespace bcp
