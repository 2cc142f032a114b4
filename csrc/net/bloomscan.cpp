#include "net/bloomscan.h"

#include "crypto/common.h"
#include "kernels/gpu_api.h"
#include "script/script.h"
#include "util/util.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>

namespace bcp {

namespace {

// The pushes CScript::GetOp would return, without the copies: fn(data, size) for each non-empty
// one, stopping where GetOp fails (a push that runs past the script's end).
template <typename F> void ForEachPush(const CScript& script, F&& fn) {
    const unsigned char* pc = script.data();
    const unsigned char* const end = pc + script.size();
    while (pc < end) {
        const unsigned opcode = *pc++;
        if (opcode > OP_PUSHDATA4) continue;
        size_t nSize = 0;
        if (opcode < OP_PUSHDATA1) {
            nSize = opcode;
        } else if (opcode == OP_PUSHDATA1) {
            if (end - pc < 1) return;
            nSize = *pc++;
        } else if (opcode == OP_PUSHDATA2) {
            if (end - pc < 2) return;
            nSize = ReadLE16(pc);
            pc += 2;
        } else {
            if (end - pc < 4) return;
            nSize = ReadLE32(pc);
            pc += 4;
        }
        if ((size_t)(end - pc) < nSize) return;
        if (nSize) fn(pc, nSize);
        pc += nSize;
    }
}

// fn(kind, index, data, size) for each element of tx in IsRelevantAndUpdate's order
template <typename F> void ForEachElement(const CTransaction& tx, F&& fn) {
    fn(BLOOM_EL_TXID, 0u, tx.GetHash().begin(), (size_t)32);
    for (unsigned i = 0; i < tx.vout.size(); i++)
        ForEachPush(tx.vout[i].scriptPubKey, [&](const unsigned char* p, size_t n) { fn(BLOOM_EL_OUT_PUSH, i, p, n); });
    for (unsigned i = 0; i < tx.vin.size(); i++) {
        unsigned char op[36];
        memcpy(op, tx.vin[i].prevout.hash.begin(), 32);
        WriteLE32(op + 32, tx.vin[i].prevout.n);
        fn(BLOOM_EL_PREVOUT, i, op, sizeof(op));
        ForEachPush(tx.vin[i].scriptSig, [&](const unsigned char* p, size_t n) { fn(BLOOM_EL_IN_PUSH, i, p, n); });
    }
}

// The element table of one list: where each transaction's elements start, what each is, and
// (offset, length) into one blob. offs/lens/blob point into pinned staging or into `own`.
struct ElementTable {
    std::vector<uint32_t> first;  // first[t] .. first[t + 1]: the elements of transaction t
    std::vector<uint32_t> byteAt; // the same for blob bytes
    std::vector<uint8_t> kind;
    uint32_t* offs = nullptr;
    uint32_t* lens = nullptr;
    unsigned char* blob = nullptr;
    std::vector<uint32_t> ownIdx;
    std::vector<unsigned char> ownBlob;
    size_t Elements() const { return first.back(); }
    size_t Bytes() const { return byteAt.back(); }
};

WorkerPool& ScanPool() {
    static WorkerPool pool(std::max(1, std::min(8, GetNumCores())));
    return pool;
}

template <typename F> void ForEachTx(size_t n, F&& fn) {
    if (n >= 512) ScanPool().ParallelFor(n, fn, 64);
    else for (size_t t = 0; t < n; t++) fn(t);
}

// pass 1: sizes per transaction and their prefix sums
void CountElements(const std::vector<CTransactionRef>& txs, ElementTable& E) {
    const size_t n = txs.size();
    E.first.assign(n + 1, 0);
    E.byteAt.assign(n + 1, 0);
    ForEachTx(n, [&](size_t t) {
        uint32_t cnt = 0, bytes = 0; // a transaction is far below 4 GiB
        ForEachElement(*txs[t], [&](uint8_t, unsigned, const unsigned char*, size_t len) {
            cnt++;
            bytes += (uint32_t)len;
        });
        E.first[t + 1] = cnt;
        E.byteAt[t + 1] = bytes;
    });
    uint64_t e = 0, b = 0;
    for (size_t t = 1; t <= n; t++) {
        e += E.first[t];
        b += E.byteAt[t];
        if (e > 0xFFFFFFFFu || b > 0xFFFFFFFFu) throw std::length_error("bloom scan: the list's elements exceed 4 GiB");
        E.first[t] = (uint32_t)e;
        E.byteAt[t] = (uint32_t)b;
    }
}

// pass 2: every transaction writes its own part of the table
void FillElements(const std::vector<CTransactionRef>& txs, ElementTable& E) {
    E.kind.resize(E.Elements());
    ForEachTx(txs.size(), [&](size_t t) {
        uint32_t e = E.first[t], at = E.byteAt[t];
        ForEachElement(*txs[t], [&](uint8_t kind, unsigned, const unsigned char* p, size_t len) {
            E.kind[e] = kind;
            E.offs[e] = at;
            E.lens[e] = (uint32_t)len;
            memcpy(E.blob + at, p, len);
            e++;
            at += (uint32_t)len;
        });
    });
}

void UseOwnStorage(ElementTable& E) {
    E.ownIdx.resize(2 * E.Elements());
    E.ownBlob.resize(E.Bytes());
    E.offs = E.ownIdx.data();
    E.lens = E.offs + E.Elements();
    E.blob = E.ownBlob.data();
}

std::atomic<size_t> g_threshold{0};
std::atomic<bool> g_enabled{true};
std::atomic<int> g_consecutiveFailures{0};
std::atomic<uint64_t> g_gpuScans{0}, g_gpuElements{0}, g_rounds{0}, g_cpuReruns{0}, g_cpuScans{0}, g_gpuFailures{0};

// one device table, one scan on the device at a time
std::mutex g_tableMutex;
std::unique_ptr<gpu::BloomElementTable> g_table;

bool DevicePathOpen() {
    return g_consecutiveFailures.load() < 3 && (GpuFaultInjection() || gpu::GpuAvailable());
}

} // namespace

void SetGpuBloomThreshold(size_t n) { g_threshold = n; }
size_t GetGpuBloomThreshold() { return g_threshold.load(); }
void SetGpuBloomEnabled(bool on) { g_enabled = on; }
bool GpuBloomScanWanted(size_t n) {
    const size_t th = g_threshold.load();
    return th != 0 && n >= th && g_enabled.load() && DevicePathOpen();
}
BloomScanStats GetBloomScanStats() {
    BloomScanStats s;
    s.gpu_scans = g_gpuScans;
    s.gpu_elements = g_gpuElements;
    s.rounds = g_rounds;
    s.cpu_reruns = g_cpuReruns;
    s.cpu_scans = g_cpuScans;
    s.gpu_failures = g_gpuFailures;
    return s;
}
void ResetBloomScanFailures() { g_consecutiveFailures = 0; }

std::vector<BloomElement> BloomExtractElements(const std::vector<CTransactionRef>& txs) {
    std::vector<BloomElement> out;
    for (size_t t = 0; t < txs.size(); t++)
        ForEachElement(*txs[t], [&](uint8_t kind, unsigned index, const unsigned char* p, size_t len) {
            out.push_back({(uint32_t)t, kind, index, std::vector<unsigned char>(p, p + len)});
        });
    return out;
}

std::vector<bool> BloomScanTransactions(const std::vector<CTransactionRef>& txs, CBloomFilter& filter, bool allowGpu,
                                        BloomScanInfo* info) {
    const size_t ntx = txs.size();
    std::vector<bool> out(ntx, false);
    BloomScanInfo I;
    size_t t = 0; // transactions [0, t) have their verdict
    auto done = [&]() -> std::vector<bool>& {
        for (; t < ntx; t++) out[t] = filter.IsRelevantAndUpdate(*txs[t]);
        g_rounds += I.rounds;
        g_cpuReruns += I.cpuReruns;
        if (I.usedGpu) {
            g_gpuScans++;
            g_gpuElements += I.elements;
        } else {
            g_cpuScans++;
        }
        if (info) *info = I;
        return out;
    };
    if (!ntx) return done();
    // what the loop answers without a single hash
    if (filter.IsFull()) {
        out.assign(ntx, true);
        t = ntx;
        return done();
    }
    if (filter.IsEmpty() || filter.Data().empty()) {
        t = ntx;
        return done();
    }
    // contains() is true of everything without hash functions, and a filter past the protocol's
    // limits is not one the kernel takes: the loop itself
    if (filter.HashFuncs() == 0 || !filter.IsWithinSizeConstraints()) return done();

    ElementTable E;
    CountElements(txs, E);
    I.elements = E.Elements();
    bool device = allowGpu && DevicePathOpen();
    std::unique_lock<std::mutex> tableLock;
    auto deviceFailed = [&](const std::exception& e) {
        const int f = ++g_consecutiveFailures;
        g_gpuFailures++;
        LogPrintf("GPU bloom scan failed (%s); finishing %zu of %zu transactions on the CPU%s\n", e.what(), ntx - t, ntx,
                  f >= 3 ? " (GPU path now disabled)" : "");
    };
    if (device) {
        try {
            if (GpuFaultInjection()) throw std::runtime_error("injected GPU bloom-scan fault");
            tableLock = std::unique_lock<std::mutex>(g_tableMutex);
            if (!g_table) g_table.reset(new gpu::BloomElementTable());
            g_table->Stage(E.Elements(), E.Bytes(), &E.offs, &E.lens, &E.blob);
            FillElements(txs, E);
            g_table->Commit();
        } catch (const std::exception& e) {
            deviceFailed(e);
            return done();
        }
    } else {
        UseOwnStorage(E);
        FillElements(txs, E);
    }

    const std::vector<unsigned char>& vData = filter.Data();
    const uint32_t nBits = (uint32_t)vData.size() * 8;
    std::vector<uint8_t> flags(E.Elements());
    while (t < ntx && I.rounds < 8) {
        // flags of the elements of transactions t.. against the filter as it is now; it only
        // gains bits, so a set flag stays true whatever is inserted later
        const size_t e0 = E.first[t];
        if (device) {
            try {
                g_table->Match(vData.data(), (uint32_t)vData.size(), filter.HashFuncs(), filter.Tweak(), e0, flags.data() + e0);
                I.usedGpu = true;
                g_consecutiveFailures = 0;
            } catch (const std::exception& e) {
                deviceFailed(e);
                return done();
            }
        } else {
            for (size_t e = e0; e < E.Elements(); e++) {
                uint8_t ok = 1;
                for (unsigned h = 0; h < filter.HashFuncs() && ok; h++) {
                    const uint32_t bit = MurmurHash3(h * 0xFBA4C795 + filter.Tweak(), E.blob + E.offs[e], E.lens[e]) % nBits;
                    ok = (vData[bit >> 3] >> (bit & 7)) & 1;
                }
                flags[e] = ok;
            }
        }
        I.rounds++;
        bool changed = false;
        for (; t < ntx && !changed; t++) {
            bool any = false, outPush = false;
            for (size_t e = E.first[t]; e < E.first[t + 1]; e++) {
                if (flags[e] != 1) continue;
                any = true;
                outPush |= E.kind[e] == BLOOM_EL_OUT_PUSH;
            }
            // Without a matching output push the transaction inserts nothing, and since the
            // filter has not changed since the pass its flags are exact.
            if (!outPush) {
                out[t] = any;
                continue;
            }
            const uint64_t before = filter.BitsFlipped();
            out[t] = filter.IsRelevantAndUpdate(*txs[t]);
            I.cpuReruns++;
            changed = filter.BitsFlipped() != before; // later flags may be stale: a new pass
        }
    }
    return done(); // past the last round the loop takes what is left
}

} // namespace bcp
