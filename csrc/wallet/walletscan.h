// A whole transaction list (a block of a rescan, a connected block) against the wallet: every
// txid, prevout and scriptPubKey is extracted once, matched as a batch against the wallet's match
// table (on the device, csrc/kernels/wallet_match.hip wallet_match_kernel; the same code on the
// host without one), and an in-order walk calls the unchanged CWallet::AddToWalletIfInvolvingMe
// for the transactions the match flagged. Verdicts, mapWallet, mapTxSpends, conflict marks and
// the wallet db end up exactly as a loop of AddToWalletIfInvolvingMe over the list leaves them.
//
// Why an unflagged transaction may be skipped. The table holds four sets: K, the 20-byte ids of
// every key of the keystore and of every script of mapScripts; W, the watch-only scripts; T, the
// txids of mapWallet; S, the keys of mapTxSpends. Lookups go by salted 61-bit fingerprints, so a
// member is always found and a non-member seldom is: the flags are a superset. For a transaction
// with no flag, AddToWalletIfInvolvingMe (wallet.cpp) is a no-op:
//   - no input is in S, so mapTxSpends.equal_range finds nothing and MarkConflicted is not called;
//   - the txid is not in T, so fExisted is false: neither the early return nor the update path;
//   - IsMine(tx) is false. IsMine(script) answers from Solver's solutions only:
//       TX_PUBKEYHASH  HaveKey(the 20-byte push): a 20-byte push, which probed K;
//       TX_SCRIPTHASH  GetCScript(the 20-byte push) and then IsMine of that script: without the
//                      id in mapScripts there is no recursion, and the id is a 20-byte push;
//       TX_PUBKEY      HaveKey(CPubKey(push).GetID()), the push being 33..65 bytes: the lane
//                      hashed what CPubKey hashes. A push whose header byte does not announce its
//                      own length (33 bytes under 0x05, any of 34..64 bytes) makes CPubKey::Set
//                      clear the key, and GetID is then HASH160 of no bytes: the lane probes K
//                      with exactly that id, so even this case needs no argument about preimages;
//       TX_MULTISIG    spendable only when every key is ours: then the first is, and it is a
//                      33..65-byte push, probed as above;
//       nonstandard and null data: nothing of the keystore but HaveWatchOnly.
//     Every solution is a push GetOp returned before any failure, and the lane walks by GetOp's
//     rules to the first failure. Last, HaveWatchOnly(script) looks the whole script up in
//     setWatchOnly: the lane probed W with it (skipped when W is empty, as HaveWatchOnly is false);
//   - IsFromMe(tx) is false: GetDebit needs an input whose prevout hash is in mapWallet, and
//     every input probed T with its first 32 bytes.
//   A script longer than 10,000 bytes is not given to the device; its transaction is flagged.
//
// Growth inside the list. A transaction the walk adds puts its txid into T and (unless it is a
// coinbase) its inputs into S, so later transactions may now concern the wallet: A pays us and B,
// later in the list, spends A. After such an add the additions are uploaded as a small second
// table and the remaining txids and inputs are matched against it (K and W do not grow during a
// scan: AddToWallet marks no keypool keys), up to 16 passes; past that the remaining transactions
// are checked against the exact additions on the host. Flags only ever gain bits, and a
// transaction is judged only after every addition made before it was matched, so B listed before A
// is not found, as in the loop.
#pragma once
#include "primitives/transaction.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bcp {

class CWallet;
class CBlockIndex;

struct WalletScanInfo {
    size_t items = 0;     // items extracted
    size_t passes = 0;    // batched match passes (1 + one per in-list addition, up to 16)
    size_t cpuReruns = 0; // flagged transactions run through AddToWalletIfInvolvingMe
    bool usedGpu = false; // at least one pass ran on the device
    // where the time went, microseconds: the table (built or checked) and the items' extraction
    // into staging; the passes (uploads, kernel, download, wait; the twin on the host); the walk
    int64_t extractMicros = 0, matchMicros = 0, walkMicros = 0;
};
// out[i] = wallet.AddToWalletIfInvolvingMe(txs[i], pindex, i, fUpdate) as a loop over the list
// would give it, the wallet afterwards being that loop's. allowGpu: run the passes on the device
// when one is visible and the path is not disabled; otherwise the same table, extraction and walk
// run on the host. A device failure is logged and the rest of the list finished by the plain
// loop; three consecutive failures turn the device path off.
std::vector<bool> WalletScanTransactions(CWallet& wallet, const std::vector<CTransactionRef>& txs,
                                         const CBlockIndex* pindex, bool fUpdate, bool allowGpu,
                                         WalletScanInfo* info = nullptr);

// The wallet's cached match table (built at the first scan, appended to by every scan, rebuilt
// when the wallet's sets changed behind its back). Opaque outside walletscan.cpp.
struct WalletScanCache;

// -gpuwalletscanthreshold: the smallest list the wallet hands to WalletScanTransactions (0: never).
// The default is the smallest list at which the scan beat the loop (profiles/wallet_scan.md).
static const size_t DEFAULT_GPU_WALLET_SCAN_THRESHOLD = 250;
void SetGpuWalletScanThreshold(size_t n);
size_t GetGpuWalletScanThreshold();
// -gpu: whether the node may use the device for this at all
void SetGpuWalletScanEnabled(bool on);
// true when a list of n transactions should go through WalletScanTransactions(allowGpu = true)
bool GpuWalletScanWanted(size_t n);

struct WalletScanStats {
    uint64_t wallet_scans = 0, items = 0, passes = 0, cpu_reruns = 0, cpu_scans = 0, gpu_failures = 0;
};
WalletScanStats GetWalletScanStats();
void ResetWalletScanFailures(); // re-enable the device path (tests)

} // namespace bcp
