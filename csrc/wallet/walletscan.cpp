#include "wallet/walletscan.h"

#include "crypto/common.h"
#include "kernels/gpu_api.h"
#include "util/util.h"
#include "wallet/wallet.h"
#include "wallet/walletmatch.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>

namespace bcp {

// What of the wallet the table was built from: the sizes of its sets. A scan appends what it adds
// itself and takes the new sizes; any other difference (a key imported, a transaction sent) means
// the table is rebuilt. Removals keep a stale member, which costs a CPU rerun at most, except
// where a removal and an addition could cancel out: those sites call InvalidateScanCache.
struct WalletScanCache {
    WalletMatchTable table;
    size_t nKeys = 0, nScripts = 0, nWatch = 0, nWalletTx = 0, nSpends = 0;
    uint64_t id = 0; // distinguishes caches for the device copy
};

struct WalletScanAccess {
    static void Sizes(const CWallet& w, WalletScanCache& c) {
        std::lock_guard<CCriticalSection> lk(w.cs_KeyStore);
        c.nKeys = w.mapKeys.size() + w.mapCryptedKeys.size();
        c.nScripts = w.mapScripts.size();
        c.nWatch = w.setWatchOnly.size();
        c.nWalletTx = w.mapWallet.size();
        c.nSpends = w.mapTxSpends.size();
    }
    static bool Fresh(const CWallet& w, const WalletScanCache& c) {
        WalletScanCache now;
        Sizes(w, now);
        return now.nKeys == c.nKeys && now.nScripts == c.nScripts && now.nWatch == c.nWatch && now.nWalletTx == c.nWalletTx &&
               now.nSpends == c.nSpends;
    }
    static void Build(const CWallet& w, WalletScanCache& c) {
        static std::atomic<uint64_t> nextId{1};
        c.table = WalletMatchTable();
        c.id = nextId++;
        Sizes(w, c);
        c.table.Reserve(c.nKeys + c.nScripts + c.nWatch + c.nWalletTx + c.nSpends);
        std::lock_guard<CCriticalSection> lk(w.cs_KeyStore);
        for (const auto& kv : w.mapKeys) c.table.Insert(wm::TAG_K, kv.first.begin(), 20);
        for (const auto& kv : w.mapCryptedKeys) c.table.Insert(wm::TAG_K, kv.first.begin(), 20);
        for (const auto& kv : w.mapScripts) c.table.Insert(wm::TAG_K, kv.first.begin(), 20);
        for (const CScript& s : w.setWatchOnly) c.table.Insert(wm::TAG_W, s.data(), s.size());
        for (const auto& kv : w.mapWallet) c.table.Insert(wm::TAG_T, kv.first.begin(), 32);
        unsigned char op[36];
        for (const auto& kv : w.mapTxSpends) {
            memcpy(op, kv.first.hash.begin(), 32);
            WriteLE32(op + 32, kv.first.n);
            c.table.Insert(wm::TAG_S, op, 36);
        }
    }
    static WalletScanCache& Cache(CWallet& w) {
        if (!w.scanCache || !Fresh(w, *w.scanCache)) {
            w.scanCache = std::make_shared<WalletScanCache>();
            Build(w, *w.scanCache);
        }
        return *w.scanCache;
    }
    static size_t Spends(const CWallet& w) { return w.mapTxSpends.size(); }
};

void CWallet::InvalidateScanCache() {
    WalletLock l(*this);
    scanCache.reset();
}

// A transaction sent or received between scans keeps the table current instead of making the
// next scan rebuild it: the txid joins T, the inputs S, and the sizes the table stands for move
// by exactly that much, so any other change still shows.
void CWallet::NoteScanCacheAdded(const CTransaction& tx) {
    if (!scanCache) return;
    WalletScanCache& c = *scanCache;
    c.table.Insert(wm::TAG_T, tx.GetHash().begin(), 32);
    c.nWalletTx++;
    if (tx.IsCoinBase()) return;
    for (const CTxIn& in : tx.vin) {
        unsigned char op[36];
        memcpy(op, in.prevout.hash.begin(), 32);
        WriteLE32(op + 32, in.prevout.n);
        c.table.Insert(wm::TAG_S, op, 36);
        c.nSpends++;
    }
}

namespace {

// fn(kind, data, size) for each item of tx: the txid, every prevout, every scriptPubKey of at
// most 10,000 bytes. Returns false when a longer script was left out.
template <typename F> bool ForEachItem(const CTransaction& tx, F&& fn) {
    bool all = true;
    fn((uint8_t)wm::ITEM_TXID, tx.GetHash().begin(), (size_t)32);
    for (const CTxIn& in : tx.vin) {
        unsigned char op[36];
        memcpy(op, in.prevout.hash.begin(), 32);
        WriteLE32(op + 32, in.prevout.n);
        fn((uint8_t)wm::ITEM_INPUT, op, sizeof(op));
    }
    for (const CTxOut& o : tx.vout) {
        if (o.scriptPubKey.size() > wm::WM_MAX_SCRIPT) {
            all = false;
            continue;
        }
        fn((uint8_t)wm::ITEM_OUTPUT, o.scriptPubKey.data(), o.scriptPubKey.size());
    }
    return all;
}

struct ItemTable {
    std::vector<uint32_t> first;  // first[t] .. first[t + 1]: the items of transaction t
    std::vector<uint32_t> byteAt; // the same for blob bytes
    std::vector<uint8_t> force;   // the transaction has a script the device was not given
    uint8_t* kinds = nullptr;
    uint32_t* offs = nullptr;
    uint32_t* lens = nullptr;
    unsigned char* blob = nullptr;
    std::vector<uint32_t> ownIdx;
    std::vector<unsigned char> ownBytes;
    size_t Items() const { return first.back(); }
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

void CountItems(const std::vector<CTransactionRef>& txs, ItemTable& E) {
    const size_t n = txs.size();
    E.first.assign(n + 1, 0);
    E.byteAt.assign(n + 1, 0);
    E.force.assign(n, 0);
    ForEachTx(n, [&](size_t t) {
        uint32_t cnt = 0, bytes = 0; // a transaction is far below 4 GiB
        const bool all = ForEachItem(*txs[t], [&](uint8_t, const unsigned char*, size_t len) {
            cnt++;
            bytes += (uint32_t)len;
        });
        E.first[t + 1] = cnt;
        E.byteAt[t + 1] = bytes;
        E.force[t] = !all;
    });
    uint64_t e = 0, b = 0;
    for (size_t t = 1; t <= n; t++) {
        e += E.first[t];
        b += E.byteAt[t];
        if (e > 0xFFFFFFFFu || b > 0xFFFFFFFFu) throw std::length_error("wallet scan: the list's items exceed 4 GiB");
        E.first[t] = (uint32_t)e;
        E.byteAt[t] = (uint32_t)b;
    }
}

// every transaction writes its own part of the table
void FillItems(const std::vector<CTransactionRef>& txs, ItemTable& E) {
    ForEachTx(txs.size(), [&](size_t t) {
        uint32_t e = E.first[t], at = E.byteAt[t];
        ForEachItem(*txs[t], [&](uint8_t kind, const unsigned char* p, size_t len) {
            E.kinds[e] = kind;
            E.offs[e] = at;
            E.lens[e] = (uint32_t)len;
            memcpy(E.blob + at, p, len);
            e++;
            at += (uint32_t)len;
        });
    });
}

void UseOwnStorage(ItemTable& E) {
    E.ownIdx.resize(2 * E.Items());
    E.ownBytes.resize(E.Items() + E.Bytes());
    E.offs = E.ownIdx.data();
    E.lens = E.offs + E.Items();
    E.kinds = E.ownBytes.data();
    E.blob = E.kinds + E.Items();
}

gpu::WalletMatchTableDesc DescOf(const WalletMatchTable& t) {
    return gpu::WalletMatchTableDesc{t.Data(), t.Slots(), t.K0(), t.K1(), t.HasWatch()};
}

constexpr size_t MAX_DEVICE_PASSES = 16;

std::atomic<size_t> g_threshold{DEFAULT_GPU_WALLET_SCAN_THRESHOLD};
std::atomic<bool> g_enabled{true};
std::atomic<int> g_consecutiveFailures{0};
std::atomic<uint64_t> g_gpuScans{0}, g_items{0}, g_passes{0}, g_cpuReruns{0}, g_cpuScans{0}, g_gpuFailures{0};

// one set of device items and tables, one scan on the device at a time
std::mutex g_itemsMutex;
std::unique_ptr<gpu::WalletMatchItems> g_items_dev;
uint64_t g_residentCache = 0, g_residentLayout = 0; // whose table is table 0 on the device

bool DevicePathOpen() { return g_consecutiveFailures.load() < 3 && (GpuFaultInjection() || gpu::GpuAvailable()); }

} // namespace

void SetGpuWalletScanThreshold(size_t n) { g_threshold = n; }
size_t GetGpuWalletScanThreshold() { return g_threshold.load(); }
void SetGpuWalletScanEnabled(bool on) { g_enabled = on; }
bool GpuWalletScanWanted(size_t n) {
    const size_t th = g_threshold.load();
    return th != 0 && n >= th && g_enabled.load() && DevicePathOpen();
}
WalletScanStats GetWalletScanStats() {
    WalletScanStats s;
    s.wallet_scans = g_gpuScans;
    s.items = g_items;
    s.passes = g_passes;
    s.cpu_reruns = g_cpuReruns;
    s.cpu_scans = g_cpuScans;
    s.gpu_failures = g_gpuFailures;
    return s;
}
void ResetWalletScanFailures() { g_consecutiveFailures = 0; }

std::vector<bool> WalletScanTransactions(CWallet& wallet, const std::vector<CTransactionRef>& txs,
                                         const CBlockIndex* pindex, bool fUpdate, bool allowGpu, WalletScanInfo* info) {
    const size_t ntx = txs.size();
    std::vector<bool> out(ntx, false);
    WalletScanInfo I;
    WalletLock lock(wallet);
    size_t t = 0; // transactions [0, t) have their verdict
    auto done = [&]() -> std::vector<bool>& {
        for (; t < ntx; t++) out[t] = wallet.AddToWalletIfInvolvingMe(txs[t], pindex, (int)t, fUpdate);
        g_passes += I.passes;
        g_cpuReruns += I.cpuReruns;
        if (I.usedGpu) {
            g_gpuScans++;
            g_items += I.items;
        } else {
            g_cpuScans++;
        }
        if (info) *info = I;
        return out;
    };
    if (!ntx) return done();

    const int64_t tStart = GetTimeMicros();
    WalletScanCache& cache = WalletScanAccess::Cache(wallet);
    WalletMatchTable& table = cache.table;
    ItemTable E;
    CountItems(txs, E);
    I.items = E.Items();
    bool device = allowGpu && DevicePathOpen();
    std::unique_lock<std::mutex> itemsLock;
    auto deviceFailed = [&](const std::exception& e) {
        const int f = ++g_consecutiveFailures;
        g_gpuFailures++;
        g_residentCache = 0;
        LogPrintf("GPU wallet scan failed (%s); finishing %zu of %zu transactions on the CPU%s\n", e.what(), ntx - t, ntx,
                  f >= 3 ? " (GPU path now disabled)" : "");
    };
    if (device) {
        try {
            if (GpuFaultInjection()) throw std::runtime_error("injected GPU wallet-scan fault");
            itemsLock = std::unique_lock<std::mutex>(g_itemsMutex);
            if (!g_items_dev) g_items_dev.reset(new gpu::WalletMatchItems());
            g_items_dev->Stage(E.Items(), E.Bytes(), &E.kinds, &E.offs, &E.lens, &E.blob);
            FillItems(txs, E);
            g_items_dev->Commit();
            // the wallet's table: as it is on the device, patched, or whole
            const std::vector<uint32_t> dirty = table.TakeDirty();
            if (g_residentCache == cache.id && g_residentLayout == table.Layout()) {
                if (!dirty.empty()) g_items_dev->PatchTable(0, dirty.data(), dirty.size(), DescOf(table));
            } else {
                g_items_dev->SetTable(0, DescOf(table));
                g_residentCache = cache.id;
                g_residentLayout = table.Layout();
            }
        } catch (const std::exception& e) {
            deviceFailed(e);
            return done();
        }
    } else {
        UseOwnStorage(E);
        FillItems(txs, E);
    }

    I.extractMicros = GetTimeMicros() - tStart;
    std::vector<uint8_t> flags(E.Items(), 0), pass(E.Items());
    // the transactions a walk step added, for the next pass
    std::unique_ptr<WalletMatchTable> delta;
    // past the device passes: the exact additions
    std::set<uint256> lateTx;
    std::set<COutPoint> lateSpent;
    bool late = false;
    auto flagged = [&](size_t i) {
        if (E.force[i]) return true;
        for (size_t e = E.first[i]; e < E.first[i + 1]; e++)
            if (flags[e]) return true; // NOT_READ too: what was not matched is judged by the wallet
        if (late) {
            const CTransaction& tx = *txs[i];
            if (lateTx.count(tx.GetHash())) return true;
            for (const CTxIn& in : tx.vin)
                if (lateSpent.count(in.prevout) || lateTx.count(in.prevout.hash)) return true;
        }
        return false;
    };
    while (t < ntx) {
        // flags of the items of transactions t.. : the first pass against the wallet's table, a
        // later one against what the last walk step added. Flags only gain bits.
        const size_t e0 = E.first[t];
        const size_t cnt = E.Items() - e0;
        const bool first = I.passes == 0;
        const WalletMatchTable& against = first ? table : *delta;
        const uint32_t kindMask = first ? wm::KIND_MASK_ALL : wm::KIND_MASK_COINS;
        const int64_t tPass = GetTimeMicros();
        if (device) {
            try {
                if (!first) g_items_dev->SetTable(1, DescOf(against));
                g_items_dev->Match(first ? 0 : 1, e0, kindMask, pass.data() + e0);
                I.usedGpu = true;
                g_consecutiveFailures = 0;
            } catch (const std::exception& e) {
                deviceFailed(e);
                return done();
            }
        } else {
            WalletMatchCpu(against, kindMask, E.kinds + e0, E.blob, E.Bytes(), E.offs + e0, E.lens + e0, cnt, pass.data() + e0);
        }
        for (size_t e = e0; e < E.Items(); e++) flags[e] |= pass[e];
        I.passes++;
        const int64_t tWalk = GetTimeMicros();
        I.matchMicros += tWalk - tPass;
        bool again = false;
        for (; t < ntx && !again; t++) {
            if (!flagged(t)) continue; // a no-op of AddToWalletIfInvolvingMe: see the header
            const size_t nTx = wallet.mapWallet.size(), nSp = WalletScanAccess::Spends(wallet);
            out[t] = wallet.AddToWalletIfInvolvingMe(txs[t], pindex, (int)t, fUpdate);
            I.cpuReruns++;
            if (wallet.mapWallet.size() == nTx && WalletScanAccess::Spends(wallet) == nSp) continue;
            // added: its txid joins T, its inputs S (AddToSpends leaves a coinbase's out)
            const CTransaction& tx = *txs[t];
            const bool deviceNext = I.passes < MAX_DEVICE_PASSES && t + 1 < ntx;
            if (deviceNext) delta.reset(new WalletMatchTable(table.K0(), table.K1()));
            else late = true;
            auto add = [&](wm::Tag tag, const unsigned char* p, size_t len) {
                table.Insert(tag, p, len);
                if (deviceNext) delta->Insert(tag, p, len);
            };
            add(wm::TAG_T, tx.GetHash().begin(), 32);
            if (!deviceNext) lateTx.insert(tx.GetHash());
            if (!tx.IsCoinBase())
                for (const CTxIn& in : tx.vin) {
                    unsigned char op[36];
                    memcpy(op, in.prevout.hash.begin(), 32);
                    WriteLE32(op + 32, in.prevout.n);
                    add(wm::TAG_S, op, 36);
                    if (!deviceNext) lateSpent.insert(in.prevout);
                }
            again = deviceNext;
        }
        I.walkMicros += GetTimeMicros() - tWalk;
    }
    WalletScanAccess::Sizes(wallet, cache); // the table now holds what the walk added
    return done();
}

} // namespace bcp
