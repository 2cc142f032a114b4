// Host-side API of the CDNA4 (gfx950) kernels. Every function here is
// implemented in a csrc/kernels/*.hip translation unit and launches hand-written
// HIP kernels; nothing here falls back to the CPU. Callers that must run
// without a GPU (the node on a CPU-only host) check GpuAvailable() first and
// use the CPU consensus code instead.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <functional>
#include <vector>

namespace bcp {
class CBlake2b;
namespace gpu {

bool GpuAvailable();
int DeviceCount();
std::string DeviceName(int device);
// Throws std::runtime_error with the HIP error string.
void Check(int hip_status, const char* what);

// --------------------------------------------------------------- Equihash
// Host mirror of bcpk::EhBaseState (csrc/kernels/blake2b_device.h).
struct EhBaseState {
    uint64_t h[8];
    uint64_t m[16];
    uint64_t t0;
    uint32_t g_byte;
    uint32_t outlen;
};
// Build the g-independent state from a BLAKE2b state that already absorbed
// CEquihashInput || nNonce (the solver/verifier then appends le32(g)).
EhBaseState MakeEhBaseState(const CBlake2b& st);
// Bytes of a minimal-encoded (N, K) solution (1344 for (200, 9)).
size_t EquihashSolutionBytes(unsigned N, unsigned K);

struct EhGpuStats {
    uint64_t nonces = 0;
    uint64_t candidates = 0;
    uint64_t duplicates = 0;
    uint64_t solutions = 0;
    uint64_t dropped_rows = 0;   // rows lost to bucket overflow (debug mode, nonce 0 of each batch)
    uint64_t cand_dropped = 0;   // final-round candidates past the per-nonce list (MAXCAND), every nonce
    uint64_t cand_max = 0;       // largest per-nonce final-round candidate count seen
    double gpu_ms = 0;
    uint64_t carry_launches = 0; // round kernels launched with generation waves (carrying the next nonce group)
    std::vector<uint64_t> stage_rows, stage_dropped, stage_maxfill; // debug mode, last batch
    std::vector<std::vector<uint64_t>> stage_top;
    std::vector<uint64_t> pair_dropped;
    std::vector<uint64_t> stage_dropped_all;  // every nonce: rows past a round's capacity per stage (accumulated)
    std::vector<uint64_t> pair_dropped_all;   // every nonce: pairs past a round's pair list, per round (accumulated)
    // slot rounds (EhCfg::ks), every nonce, per round: rows that found their key's slots taken
    // (accumulated), and the most of them in one bucket (index = round; zero for the sorted rounds)
    std::vector<uint64_t> overflow_rows_all, overflow_bucket_max;
    std::vector<uint64_t> pair_dropped_nonce;  // last batch, per nonce: pairs dropped in all rounds
    std::vector<uint64_t> stage_dropped_nonce; // last batch, per nonce: rows dropped in all stages
    std::vector<uint64_t> stage_maxfill_all;  // debug: fullest bucket per stage, last batch
    std::vector<uint64_t> overflow_fills; // debug: (stage << 32 | fill) of every bucket past its capacity (accumulated)
    std::vector<std::vector<uint32_t>> debug_cands;                  // debug: every candidate of nonce 0 (valid or not)
};

// "Mine this header to this target" on the device (csrc/kernels/equihash_pow.h): the nonces
// nonce_first + i, i < count (256-bit little-endian, wrapping), of the header whose
// CEquihashInput is `prefix`; a solution wins when SHA256d(header), read as a 256-bit
// little-endian integer, is at or below the target.
struct EhPowJob {
    unsigned char prefix[108];
    unsigned char nonce_first[32];
    int count;
    unsigned char target_le[32];
};
struct EhPowHit {
    unsigned char nonce[32];
    std::vector<unsigned char> solution; // minimal encoding
    unsigned char hash[32];              // the block hash (SHA256d of the whole header)
};
struct EhPowResult {
    std::vector<EhPowHit> hits; // sorted by position in the nonce range, then by hash (as an integer)
    uint64_t solutions = 0;     // all valid solutions of the batch, winners or not
    // debug mode only: every valid solution in the same order, and whether it met the target
    std::vector<EhPowHit> all;
    std::vector<uint8_t> all_pass;
};

// Batched Equihash solver: one launch sequence solves `batch` nonces at once
// (8 + 3 kernels per batch, bucket-per-workgroup collision rounds in LDS).
class EquihashGpuSolver {
public:
    EquihashGpuSolver(unsigned n, unsigned k, int batch, int device = -1);
    ~EquihashGpuSolver();
    unsigned N() const;
    unsigned K() const;
    int Batch() const;
    // states.size() <= batch. Returns, per nonce, canonical index lists of all
    // valid (distinct-index) solutions found.
    std::vector<std::vector<std::vector<uint32_t>>> Solve(const std::vector<EhBaseState>& states);
    // Asynchronous split used by the pipelined miner/bench: Launch enqueues the
    // whole sequence on the solver's stream; Collect waits and decodes.
    void Launch(const std::vector<EhBaseState>& states);
    // The same, pipelined behind `prev` (another solver on the same device whose batch was
    // launched just before this one): this batch's generation starts once prev's generation is
    // done, and its collision rounds once prev's rounds are done. Generation (VALU-bound) then
    // runs beside the previous batch's rounds (LDS/latency-bound) instead of beside another
    // generation.
    void Launch(const std::vector<EhBaseState>& states, const EquihashGpuSolver& prev);
    std::vector<std::vector<std::vector<uint32_t>>> Collect();
    // The mining step without the host: the nonce states are built on the device, the unchanged
    // solve sequence runs, and a filter kernel encodes every valid solution, hashes its header
    // and keeps the ones at or below the target; only those are copied back. job.count <=
    // Batch(). The second form is pipelined like Launch(states, prev). CollectPow updates the
    // statistics as Collect does. A LaunchPow is collected with CollectPow and a Launch with
    // Collect; the other pairing throws.
    void LaunchPow(const EhPowJob& job);
    void LaunchPow(const EhPowJob& job, const EquihashGpuSolver& prev);
    EhPowResult CollectPow();
    const EhGpuStats& Stats() const;
    void SetDebug(bool on);   // collect per-stage bucket statistics (extra D2H copies)
    void SetStampMode(bool on); // diagnostic: launch phase-timestamped round kernels
    std::vector<uint64_t> DebugDump(int nonce = 0); // diagnostic: leaf indices + parent triples of one nonce of the last batch
    std::vector<uint32_t> DebugFills(int nonce);    // debug mode: the nonce's bucket fill counters, K stages x NB
    // Test hook (after a Solve): re-run the tree expansion of nonce 0's candidates with the first
    // candidate's left stage-(K-1) parent corrupted - mode 1: bucket out of range, mode 2: LDS
    // row out of range, 0: untouched. Modes 3 and 4 corrupt the table walk of that slot's left
    // stage-(K-2) parent (a stage with table parents, else they throw) - 3: producing bucket out of
    // range in the row's padding, 4: a run base that puts the slot's ordinal past its pair table.
    // Returns each candidate's valid flag; the expansion must reject the corrupted candidate
    // without touching memory outside the stage arrays and tables.
    std::vector<uint32_t> DebugExpandCorrupt(int mode);
    std::vector<std::vector<double>> PhaseCycles(int nonces);
    void ResetStats();
    size_t DeviceBytes() const;
    struct Impl;
private:
    std::unique_ptr<Impl> impl;
};

// Batched consensus verifier (reference CheckEquihashSolution / IsValidSolution).
// One workgroup per solution: 2^K lanes hash their index, LDS tree reduction.
std::vector<uint8_t> EquihashVerifyBatch(unsigned n, unsigned k, const std::vector<EhBaseState>& states,
                                         const std::vector<std::vector<unsigned char>>& solutions,
                                         int device = -1);

// Which checks of the verifier kernel failed, one mask byte per item (diagnostics and tests; the
// accepting paths only use the verdict). A solution of another length gets EH_WHY_LENGTH from
// the host and nothing else: the kernel's bits for it are not reported.
enum EhVerifyReason : uint8_t {
    EH_WHY_COLLISION = 1, // some node's two children differ in the digit of the node's level
    EH_WHY_ORDER = 2,     // some node's left first index is not below its right first index
    EH_WHY_DUPLICATE = 4, // two positions hold the same index
    EH_WHY_FINAL = 8,     // the root's last digit is not zero
    EH_WHY_LENGTH = 16,   // the solution has another length
};
// Same lane, staging and kernel as EquihashVerifyBatch, the same four parameter sets; mask == 0
// iff EquihashVerifyBatch accepts.
std::vector<uint8_t> EquihashVerifyReasons(unsigned n, unsigned k, const std::vector<EhBaseState>& states,
                                           const std::vector<std::vector<unsigned char>>& solutions,
                                           int device = -1);

// Block hashes of cnt headers given as (140-byte Equihash input, minimal solution) pairs:
// hashes[32*i ..] = SHA256d(in140_i || compactsize || sol_i), pass[i] = 1 iff that hash, as a
// 256-bit little-endian integer, is at or below the target. One workgroup per pair, the device
// functions of the miner's filter kernel.
void EquihashPowCheckBatch(unsigned n, unsigned k, const unsigned char* in140, const unsigned char* sols, size_t cnt,
                           const unsigned char target_le[32], std::vector<unsigned char>& hashes,
                           std::vector<uint8_t>& pass, int device = -1);

// Status bits of a header checked by VerifyLane::CheckHeaders / EquihashCheckHeadersDevice
// (csrc/kernels/equihash_header.h): the whole of CheckBlockHeader for a post-fork header.
enum HeaderStatus : uint8_t {
    HDR_SOLUTION_VALID = 1, // the Equihash solution is valid (IsValidSolution)
    HDR_TARGET_LEGAL = 2,   // nBits decodes (SetCompact) to a target in (0, pow limit], not negative, no overflow
    HDR_HASH_MEETS = 4,     // TARGET_LEGAL and hash <= target: CheckProofOfWork
    HDR_HASH_VALID = 8,     // the returned hash is the header's; clear where the solution has another length
                            // (the serialization then has another length too: the caller hashes on the CPU)
    HDR_LINKED = 16,        // hashPrevBlock equals the hash of the header before it, both hashes valid (header 0: set)
};
// Debug entry: arith_uint256::SetCompact on the device over n nBits values. targets_le = n x 32
// bytes (256-bit little-endian), flags[i] = negative | overflow << 1.
void EquihashCompactDecodeBatch(const uint32_t* nbits, size_t n, std::vector<unsigned char>& targets_le,
                                std::vector<uint8_t>& flags, int device = -1);

// --------------------------------------------------------------- SHA-256d
// out[i] = SHA256d(in[offs[i] .. offs[i]+lens[i]))
std::vector<unsigned char> Sha256dBatch(const std::vector<unsigned char>& data, const std::vector<uint64_t>& offs,
                                        const std::vector<uint32_t>& lens, int device = -1);
// out[i] = SHA256d(in[64*i .. 64*i+64))
std::vector<unsigned char> Sha256d64Batch(const std::vector<unsigned char>& data, int device = -1);
// Merkle root of 32-byte leaves with the reference's mutation flag
// (reference src/consensus/merkle.cpp:47-175, CVE-2012-2459).
std::vector<unsigned char> MerkleRoot(const std::vector<unsigned char>& leaves, bool* mutated, int device = -1);
// Legacy 80-byte header nonce sweep: returns the first nonce in
// [start, start+count) with SHA256d(header) <= target, or -1.
int64_t Sha256dScanNonces(const unsigned char header80[80], const unsigned char target_le[32], uint32_t start,
                          uint64_t count, int device = -1);

// --------------------------------------------------------------- relay: BIP152 short ids
// out[i] = SipHash-2-4(k0, k1, txid_i) & (2^48 - 1), txids32 = n x 32 bytes (reference
// src/blockencodings.cpp:37-42 GetShortID, src/hash.cpp:181-300 SipHashUint256). Used for the
// mempool side of compact-block reconstruction when the pool is large.
std::vector<uint64_t> ShortTxIdBatch(uint64_t k0, uint64_t k1, const unsigned char* txids32, size_t n,
                                     int device = -1);

// --------------------------------------------------------------- relay: BIP37 bloom filters
// CBloomFilter::contains for a batch of byte strings (reference src/bloom.cpp:82-91): element i is
// blob[offs[i] .. offs[i] + lens[i]), filter = vData (1..36000 bytes), nHashFuncs 1..50.
// match[i] = 1 iff every probe MurmurHash3(h * 0xFBA4C795 + nTweak, element) % (filterBytes * 8),
// h < nHashFuncs, finds its bit set. Both forms throw std::invalid_argument on an empty or
// oversized filter, on a hash function count outside 1..50 and (the host forms) on an empty
// element or one that reaches past the blob.
//
// The element table (blob, offsets, lengths; pinned staging and its device copy) is an object of
// its own, so that a second filter over the same elements costs only the filter's upload and the
// kernel. One thread drives a table at a time; tables of one device share the relay stream.
class BloomElementTable {
public:
    explicit BloomElementTable(int device = -1);
    ~BloomElementTable();
    BloomElementTable(const BloomElementTable&) = delete;
    BloomElementTable& operator=(const BloomElementTable&) = delete;
    int Device() const;
    // Pinned staging for n elements and blobBytes of element data, to be written by the caller
    // (threads may write disjoint parts). Discards the table staged before.
    void Stage(size_t n, size_t blobBytes, uint32_t** offs, uint32_t** lens, unsigned char** blob);
    // Checks every staged (offset, length) against the blob; throws and leaves the table unusable
    // if one fails. The upload rides on the first Match.
    void Commit();
    size_t Size() const; // committed elements
    // match[i - first] = contains(element i) for first <= i < Size(): one H2D copy (filter and,
    // the first time, the table), one launch, one D2H copy, then a wait.
    void Match(const unsigned char* filter, uint32_t filterBytes, uint32_t nHashFuncs, uint32_t nTweak, size_t first,
               uint8_t* match);
    struct Impl;

private:
    std::unique_ptr<Impl> impl;
};
// From host memory through a per-device table of the relay context.
void BloomMatchBatch(const unsigned char* filter, uint32_t filterBytes, uint32_t nHashFuncs, uint32_t nTweak,
                     const unsigned char* blob, size_t blobBytes, const uint32_t* offs, const uint32_t* lens, size_t n,
                     std::vector<uint8_t>& match, int device = -1);

// --------------------------------------------------------------- relay: wallet matching
// out[20 * i ..] = RIPEMD160(SHA256(blob[offs[i] .. offs[i] + lens[i]))), messages of 0..520 bytes
// (CHash160). Throws std::invalid_argument on a longer message or one that reaches past the blob.
std::vector<unsigned char> Hash160Batch(const unsigned char* blob, size_t blobBytes, const uint32_t* offs,
                                        const uint32_t* lens, size_t n, int device = -1);

// A wallet match table as kernels/wallet_match.h defines it (built by bcp::WalletMatchTable,
// csrc/wallet/walletmatch.h): nSlots 64-bit entries, a power of two, under the salt (k0, k1).
struct WalletMatchTableDesc {
    const uint64_t* slots;
    uint32_t nSlots;
    uint64_t k0, k1;
    bool hasWatch; // the table holds watch-only script entries: outputs probe them
};
// The items of one transaction list (kind, offset, length into one blob; pinned staging and its
// device copy) and up to two tables they are matched against: 0, the wallet's table, and 1, a
// small table of what a scan added. A later pass over the same items costs a table upload (or a
// few patched slots) and the kernel. One thread drives an object at a time; all share the relay
// stream of their device.
class WalletMatchItems {
public:
    explicit WalletMatchItems(int device = -1);
    ~WalletMatchItems();
    WalletMatchItems(const WalletMatchItems&) = delete;
    WalletMatchItems& operator=(const WalletMatchItems&) = delete;
    int Device() const;
    // Pinned staging for n items and blobBytes of item data, to be written by the caller (threads
    // may write disjoint parts). Discards the items staged before.
    void Stage(size_t n, size_t blobBytes, uint8_t** kinds, uint32_t** offs, uint32_t** lens, unsigned char** blob);
    // Checks every staged kind and (offset, length); throws and leaves the items unusable if one
    // fails. The upload rides on the first Match.
    void Commit();
    size_t Size() const; // committed items
    // Copies the table into pinned memory; the upload rides on the next Match against it.
    void SetTable(int which, const WalletMatchTableDesc& table);
    // The table set before, with the listed slots changed (an append that did not grow it): only
    // those are uploaded, or all of it past 64 of them.
    void PatchTable(int which, const uint32_t* slotIdx, size_t n, const WalletMatchTableDesc& table);
    // flags[i - first] = the wm::Flag bits of item i for first <= i < Size(); items whose kind is
    // not in kindMask get 0. Pending uploads, one launch, one D2H copy, then a wait.
    void Match(int which, size_t first, uint32_t kindMask, uint8_t* flags);
    struct Impl;

private:
    std::unique_ptr<Impl> impl;
};
// From host memory through a per-device WalletMatchItems of the relay context, every kind.
void WalletMatchBatch(const WalletMatchTableDesc& table, const uint8_t* kinds, const unsigned char* blob, size_t blobBytes,
                      const uint32_t* offs, const uint32_t* lens, size_t n, std::vector<uint8_t>& flags, int device = -1);

// --------------------------------------------------------------- wallet: coin selection
// The stochastic subset search of kernels/coin_select.h on the device, one lane per trial: the
// smallest candidate (total, trial, pass, coin) of `trials` (1..65536) trials over n amounts (each
// > 0, sum below 2^63, sorted descending by the caller) under the seed (k0, k1). nRuns = 1
// searches run firstRun (0 or 1) at targets[0]; nRuns = 2 (firstRun 0) searches run 0 at
// targets[0] and run 1 at targets[1] in the same launch. A run without a candidate (the sum is
// below its target) has every field -1.
struct CoinSelectRun {
    int64_t total, trial, pass, index;
};
// From host memory through the relay context's pinned staging: one H2D copy, two launches, one
// D2H copy, then a wait. Throws std::invalid_argument on counts or amounts out of range.
void CoinSelectBatch(const int64_t* values, size_t n, const int64_t* targets, unsigned firstRun, unsigned nRuns,
                     uint32_t trials, uint64_t k0, uint64_t k1, CoinSelectRun* out, int device = -1);

// --------------------------------------------------------------- secp256k1
// ECDSA verification batch: N jobs, msg32 = N*32 (big-endian digest bytes as signed),
// sig64 = N*64 (r||s big-endian, s low-S-normalised, r,s in [1,n-1] checked on host),
// pub33 = N*33 compressed keys (0x02/0x03 || x; the host converts uncompressed/hybrid
// keys after its on-curve check). The GPU decompresses, computes u1*G + u2*Q and
// compares x(R) mod n with r. result[i] = 1 iff valid. Batches below the GPU
// threshold should stay on the CPU (launch latency ~10 us).
std::vector<uint8_t> EcdsaVerifyBatch(const std::vector<unsigned char>& msg32, const std::vector<unsigned char>& sig64,
                                      const std::vector<unsigned char>& pub33, int device = -1);

// Batches of at most EcdsaFusedMax() signatures run one fused latency kernel (scalar work,
// key decompression and the two GLV halves on separate waves, 10 x 26-bit field); larger ones
// the prep + verify throughput kernels. Process-wide; the default is measured
// (profiles/ecdsa_r5.md).
void SetEcdsaFusedMax(size_t n);
size_t EcdsaFusedMax();
// Verify kernel of the split (prep + verify) path: 0 = 8 x 32-bit field with an inverted
// table, 1 = 10 x 26-bit field with the global-z table (one lane per signature for whole rounds
// of the device, one GLV half per lane for a last round at most half full), 2 / 3 = only the
// one-lane / only the half-lane 10 x 26 kernel (tests pin each).
void SetEcdsaSplitKernel(int k);
int EcdsaSplitKernel();

// --------------------------------------------------------------- device-resident entry points
// The tensor API (bitcoincashplus_amd.ops with torch tensors on the GPU): every pointer is
// device memory on `device`, the kernels are enqueued on `stream` (a hipStream_t passed as an
// integer, e.g. torch.cuda.current_stream().cuda_stream) after the work already queued there,
// and nothing is copied or synchronised. The caller keeps the buffers alive until the stream
// has run (torch's caching allocator does this for tensors used on their own stream).
// out32[i] = SHA256d(in64[64*i .. 64*i+64))
void Sha256d64Device(const void* in64, void* out32, size_t n, int device, uintptr_t stream);
// out[i] = BIP152 short id of txid i (48 bits in a uint64); txids32 16-byte aligned
void ShortTxIdsDevice(uint64_t k0, uint64_t k1, const void* txids32, void* out64, size_t n, int device,
                      uintptr_t stream);
// BloomMatchBatch on device memory: filter, blob, offs (uint32, 4-byte aligned), lens (the same)
// and match (n bytes) are device pointers of any other alignment. The element ranges cannot be
// checked here: the kernel reads nothing of an empty element or one that reaches past blobBytes
// and writes 2 for it.
void BloomMatchDevice(const void* filter, uint32_t filterBytes, uint32_t nHashFuncs, uint32_t nTweak, const void* blob,
                      size_t blobBytes, const void* offs, const void* lens, void* match, size_t n, int device,
                      uintptr_t stream);
// Hash160Batch on device memory: out20 = n x 20 bytes, status = n bytes (1, or 2 for a message
// longer than 520 bytes or reaching past blobBytes: nothing of it is read, its 20 bytes are zero).
// offs and lens are 4-byte aligned, everything else of any alignment.
void Hash160Device(const void* blob, size_t blobBytes, const void* offs, const void* lens, void* out20, void* status,
                   size_t n, int device, uintptr_t stream);
// WalletMatchBatch on device memory: slots 8-byte aligned, offs and lens 4-byte aligned, kinds,
// blob and flags (n bytes) of any alignment. An item that reaches past blobBytes is not read and
// gets wm::NOT_READ.
void WalletMatchDevice(const void* slots, uint32_t nSlots, uint64_t k0, uint64_t k1, bool hasWatch, uint32_t kindMask,
                       const void* kinds, const void* blob, size_t blobBytes, const void* offs, const void* lens,
                       void* flags, size_t n, int device, uintptr_t stream);
// CoinSelectBatch on device memory: values = n int64 (8-byte aligned; the amounts cannot be
// checked here), scratch = CoinSelectScratchBytes(trials, nRuns) bytes (8-byte aligned), out =
// nRuns x 4 int64 (a CoinSelectRun each). targets is host memory.
size_t CoinSelectScratchBytes(uint32_t trials, unsigned nRuns);
void CoinSelectDevice(const void* values, size_t n, const int64_t* targets, unsigned firstRun, unsigned nRuns,
                      uint32_t trials, uint64_t k0, uint64_t k1, void* scratch, void* out, int device, uintptr_t stream);
// Device scratch the ECDSA kernels need per signature (the prep kernel's job records).
size_t EcdsaJobBytes();
// result[i] = 1 iff signature i verifies; inputs as EcdsaVerifyBatch (msg32 n x 32, sig64 compact
// r||s n x 64, pub33 compressed n x 33), jobs = n x EcdsaJobBytes() of scratch.
void EcdsaVerifyDevice(const void* msg32, const void* sig64, const void* pub33, void* jobs, void* result, size_t n,
                       int device, uintptr_t stream);

// Whole header checks of n post-fork headers: in140 = n x 140 bytes (CEquihashInput || nNonce),
// sols = n x EquihashSolutionBytes(N, K), lenok = n bytes (0: the header's solution had another
// length; its slot's content is ignored), powLimitLE = the chain's pow limit (256-bit
// little-endian, host memory), scratch = EquihashCheckHeadersScratchBytes(n) bytes for the
// BLAKE2b base states (8-byte aligned), status = n HeaderStatus bytes, hashes = n x 32 bytes.
// in140, sols and hashes are 4-byte aligned. (N, K) as EquihashPowCheckBatch; others throw.
size_t EquihashCheckHeadersScratchBytes(size_t n);
void EquihashCheckHeadersDevice(unsigned N, unsigned K, const void* in140, const void* sols, const void* lenok,
                                const unsigned char powLimitLE[32], void* scratch, void* status, void* hashes, size_t n,
                                int device, uintptr_t stream);

// The same from host memory through the device's default lane (pinned staging, the lane's
// stream, one H2D and one D2H copy): status = cnt HeaderStatus bytes, hashes = cnt x 32 bytes.
void EquihashCheckHeadersBatch(unsigned n, unsigned k, const unsigned char* in140, const unsigned char* sols,
                               const uint8_t* lenok, size_t cnt, const unsigned char powLimitLE[32],
                               std::vector<uint8_t>& status, std::vector<unsigned char>& hashes, int device = -1);

// --------------------------------------------------------------- verification lanes
// A verification lane is one device plus one HIP stream (created at the device's greatest
// priority when `highPriority`, so a validation batch is scheduled ahead of the persistent
// solver kernels the miner keeps on the same device) plus grow-only pinned host staging and
// device buffers that every batch reuses (one H2D and one D2H copy per batch, no pageable
// transfers, no per-batch allocation). A lane is driven by one thread at a time; the node's
// GpuVerifyService gives each lane its own service thread (csrc/node/gpuverify.h).
class VerifyLane {
public:
    VerifyLane(int device, bool highPriority);
    ~VerifyLane();
    VerifyLane(const VerifyLane&) = delete;
    VerifyLane& operator=(const VerifyLane&) = delete;
    int Device() const;
    int Priority() const;
    // Same contract as EcdsaVerifyBatch: n packed jobs, result[i] = 1 iff valid.
    void Ecdsa(const unsigned char* msg32, const unsigned char* sig64, const unsigned char* pub33, size_t n,
               uint8_t* result);
    // Same, with the inputs written by `fill` straight into the lane's pinned staging buffer
    // (msg32: n x 32 B, sig64: n x 64 B, pub33: n x 33 B) instead of being copied there.
    void EcdsaFill(size_t n, const std::function<void(unsigned char* msg32, unsigned char* sig64,
                                                        unsigned char* pub33)>& fill,
                   uint8_t* result);
    // Same with DER signatures parsed on the device: sig73 holds n slots of [length byte][up to
    // 72 DER bytes] (hash type stripped), parsed with the reference's lax rules
    // (src/pubkey.cpp ecdsa_signature_parse_der_lax) and low-S normalised by the prep kernel; a
    // signature that does not parse verifies false. (The host then only copies bytes.)
    static constexpr size_t DER_SLOT = 73;
    void EcdsaDerFill(size_t n, const std::function<void(unsigned char* msg32, unsigned char* sig73,
                                                           unsigned char* pub33)>& fill,
                      uint8_t* result);
    // n block headers: fill(in140, sols, lenok) writes each header's 140-byte Equihash input
    // (CEquihashInput || nNonce), its solution (EquihashSolutionBytes bytes) and whether the
    // solution had that length into the lane's pinned staging; the device builds the BLAKE2b
    // base states and verifies. result[i] = 1 iff header i's solution is valid.
    void EquihashHeaders(unsigned N, unsigned K, size_t n,
                         const std::function<void(uint8_t* in140, uint8_t* sols, uint8_t* lenok)>& fill,
                         uint8_t* result);
    // The whole of CheckBlockHeader for n post-fork headers from the same `fill`: status[i] =
    // HeaderStatus bits, hashes = n x 32 bytes (zero where HDR_HASH_VALID is clear), one D2H copy
    // for both. firstPrev32, when given, receives header 0's hashPrevBlock (a caller that splits
    // a message over lanes links the shards with it). (N, K) as EquihashPowCheckBatch.
    void CheckHeaders(unsigned N, unsigned K, size_t n,
                      const std::function<void(uint8_t* in140, uint8_t* sols, uint8_t* lenok)>& fill,
                      const unsigned char powLimitLE[32], uint8_t* status, unsigned char* hashes,
                      unsigned char* firstPrev32 = nullptr);
    // Same contract as EquihashVerifyBatch for n (state, solution) pairs; a solution of the
    // wrong length is rejected.
    void Equihash(unsigned N, unsigned K, const EhBaseState* states, const std::vector<unsigned char>* const* sols,
                  size_t n, uint8_t* result);
    // Equihash plus why[i] = EhVerifyReason bits of item i (EquihashVerifyReasons).
    void EquihashReasons(unsigned N, unsigned K, const EhBaseState* states,
                         const std::vector<unsigned char>* const* sols, size_t n, uint8_t* result, uint8_t* why);
    // Batches and items this lane has run (service statistics).
    uint64_t Batches() const;
    uint64_t Items() const;
    // header hashes CheckHeaders has returned (HDR_HASH_VALID set)
    uint64_t HeaderHashes() const;
    // time spent in the callers' fills (host) and in copies + kernels + the wait (device)
    uint64_t FillMicros() const;
    uint64_t DeviceMicros() const;
    struct Impl;

private:
    std::unique_ptr<Impl> impl;
};

} // namespace gpu
} // namespace bcp
