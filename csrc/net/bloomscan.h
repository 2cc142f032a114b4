// A peer's BIP37 filter over a whole transaction list (a block for getdata MSG_FILTERED_BLOCK,
// the pool for a mempool request): every element of every transaction is extracted once, the
// membership tests run as batches (on the device, csrc/kernels/relay.hip bloom_match_kernel), and
// an in-order walk keeps the result equal to calling CBloomFilter::IsRelevantAndUpdate on each
// transaction in turn, inserts under BLOOM_UPDATE_ALL / P2PUBKEY_ONLY included.
#pragma once
#include "consensus/merkleblock.h"
#include "primitives/transaction.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bcp {

// What IsRelevantAndUpdate tests of a transaction, in the order it tests it.
enum BloomElementKind : uint8_t {
    BLOOM_EL_TXID = 0,       // the transaction's hash
    BLOOM_EL_OUT_PUSH = 1,   // a non-empty push of scriptPubKey `index`
    BLOOM_EL_PREVOUT = 2,    // the serialized prevout of input `index`
    BLOOM_EL_IN_PUSH = 3,    // a non-empty push of the scriptSig of input `index`
};
struct BloomElement {
    uint32_t tx;    // position in the list
    uint8_t kind;   // BloomElementKind
    uint32_t index; // output or input index (0 for the txid)
    std::vector<unsigned char> data;
};
// Every element of every transaction: the txid, each non-empty push of each scriptPubKey up to
// the first GetOp failure, then per input its prevout and the non-empty pushes of its scriptSig.
std::vector<BloomElement> BloomExtractElements(const std::vector<CTransactionRef>& txs);

struct BloomScanInfo {
    size_t elements = 0;  // elements extracted (0 when a shortcut or the plain loop answered)
    size_t rounds = 0;    // batched membership passes
    size_t cpuReruns = 0; // transactions with a flagged output push, run through IsRelevantAndUpdate
    bool usedGpu = false; // at least one pass ran on the device
};
// out[i] = filter.IsRelevantAndUpdate(*txs[i]) as a loop over the list would give it, and the
// filter afterwards is that loop's, bit for bit. allowGpu: run the passes on the device when one
// is visible and the path is not disabled; false (and a host without a device) runs the same
// extraction and walk with CBloomFilter::contains. A device failure is logged and the rest of
// the list finished by the plain loop; three consecutive failures turn the device path off.
std::vector<bool> BloomScanTransactions(const std::vector<CTransactionRef>& txs, CBloomFilter& filter, bool allowGpu,
                                        BloomScanInfo* info = nullptr);

// -gpubloomthreshold: the smallest list net processing hands to BloomScanTransactions (0: never).
void SetGpuBloomThreshold(size_t n);
size_t GetGpuBloomThreshold();
// -gpu: whether the node may use the device for this at all
void SetGpuBloomEnabled(bool on);
// true when a list of n transactions should go through BloomScanTransactions(allowGpu = true)
bool GpuBloomScanWanted(size_t n);

struct BloomScanStats {
    uint64_t gpu_scans = 0, gpu_elements = 0, rounds = 0, cpu_reruns = 0, cpu_scans = 0, gpu_failures = 0;
};
BloomScanStats GetBloomScanStats();
void ResetBloomScanFailures(); // re-enable the device path (tests)

} // namespace bcp
