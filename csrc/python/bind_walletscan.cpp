// Python bindings for wallet matching: the HASH160 and match kernels
// (csrc/kernels/wallet_match.hip), the match table and the CPU twin (csrc/wallet/walletmatch.h),
// and the exact scan of a transaction list (csrc/wallet/walletscan.h).
#include "consensus/chain.h"
#include "crypto/common.h"
#include "kernels/gpu_api.h"
#include "primitives/serialize.h"
#include "python/bind.h"
#include "util/util.h"
#include "wallet/wallet.h"
#include "wallet/walletmatch.h"
#include "wallet/walletscan.h"

#include <algorithm>

namespace bcp {
namespace py {

namespace {
struct Packed {
    std::vector<uint8_t> kinds;
    std::vector<unsigned char> blob;
    std::vector<uint32_t> offs, lens;
};
Packed PackBytes(const std::vector<pyb::bytes>& v) {
    Packed p;
    for (const pyb::bytes& e : v) {
        const std::string s = e;
        p.offs.push_back((uint32_t)p.blob.size());
        p.lens.push_back((uint32_t)s.size());
        p.blob.insert(p.blob.end(), s.begin(), s.end());
    }
    return p;
}
// items: (kind, bytes) pairs
Packed PackItems(const std::vector<std::pair<int, pyb::bytes>>& items) {
    Packed p;
    for (const auto& it : items) {
        const std::string s = it.second;
        p.kinds.push_back((uint8_t)it.first);
        p.offs.push_back((uint32_t)p.blob.size());
        p.lens.push_back((uint32_t)s.size());
        p.blob.insert(p.blob.end(), s.begin(), s.end());
    }
    return p;
}
std::vector<pyb::bytes> BytesList(const pyb::dict& d, const char* key) {
    if (!d.contains(key)) return {};
    return d[key].cast<std::vector<pyb::bytes>>();
}
// table_desc = {salt: 16 bytes (optional: random), keys: [20 bytes], watch: [script], txids: [32
// bytes], spent: [36 bytes]}
WalletMatchTable BuildTable(const pyb::dict& d) {
    WalletMatchTable t;
    if (d.contains("salt")) {
        const std::vector<unsigned char> salt = to_vec(d["salt"].cast<pyb::bytes>());
        if (salt.size() != 16) throw std::invalid_argument("wallet match table: salt of 16 bytes expected");
        t = WalletMatchTable(wm::LoadLE64(salt.data()), wm::LoadLE64(salt.data() + 8));
    }
    auto addAll = [&](const char* key, wm::Tag tag, size_t size) {
        for (const pyb::bytes& b : BytesList(d, key)) {
            const std::vector<unsigned char> v = to_vec(b);
            if (size && v.size() != size) throw std::invalid_argument(std::string("wallet match table: bad member size in ") + key);
            t.Insert(tag, v.data(), v.size());
        }
    };
    addAll("keys", wm::TAG_K, 20);
    addAll("watch", wm::TAG_W, 0);
    addAll("txids", wm::TAG_T, 32);
    addAll("spent", wm::TAG_S, 36);
    return t;
}
gpu::WalletMatchTableDesc DescOf(const WalletMatchTable& t) {
    return gpu::WalletMatchTableDesc{t.Data(), t.Slots(), t.K0(), t.K1(), t.HasWatch()};
}
std::vector<CTransactionRef> DecodeTxs(const std::vector<pyb::bytes>& raw) {
    std::vector<CTransactionRef> txs;
    for (const pyb::bytes& b : raw) {
        const std::vector<unsigned char> v = to_vec(b);
        SpanReader r(v.data(), v.size(), SER_NETWORK, PROTOCOL_VERSION);
        CMutableTransaction mtx;
        r >> mtx;
        txs.push_back(std::make_shared<const CTransaction>(mtx));
    }
    return txs;
}
// wallet_desc = {pubkeys, scripts, watch, wallet_txs} into a memory-only wallet
void FillWallet(CWallet& w, const pyb::dict& d) {
    CKey dummy; // IsMine asks HaveKey only: any secret stands in for the one behind a public key
    dummy.MakeNewKey(true);
    for (const pyb::bytes& b : BytesList(d, "pubkeys")) {
        const std::vector<unsigned char> v = to_vec(b);
        w.LoadKey(dummy, CPubKey(v.begin(), v.end()));
    }
    for (const pyb::bytes& b : BytesList(d, "scripts")) {
        const std::vector<unsigned char> v = to_vec(b);
        w.AddCScript(CScript(v.begin(), v.end()));
    }
    for (const pyb::bytes& b : BytesList(d, "watch")) {
        const std::vector<unsigned char> v = to_vec(b);
        w.AddWatchOnly(CScript(v.begin(), v.end()));
    }
    for (const CTransactionRef& tx : DecodeTxs(BytesList(d, "wallet_txs"))) w.AddToWallet(CWalletTx(&w, tx), false);
}
// (verdicts, wallet transactions as txid || hashBlock || nIndex, spent outpoints) after a scan
struct WalletScanAccessPy {
    static pyb::tuple State(const std::vector<bool>& verdicts, CWallet& w, const std::vector<CTransactionRef>& txs) {
        pyb::list v;
        for (bool b : verdicts) v.append(b);
        std::vector<std::string> wtxs, spent;
        WalletLock l(w);
        for (const auto& kv : w.mapWallet) {
            std::string s((const char*)kv.first.begin(), 32);
            s.append((const char*)kv.second.hashBlock.begin(), 32);
            unsigned char idx[4];
            WriteLE32(idx, (uint32_t)kv.second.nIndex);
            s.append((const char*)idx, 4);
            wtxs.push_back(s);
        }
        // every entry of mapTxSpends: outpoint || spending txid
        for (const auto& kv : w.TxSpends()) {
            std::string s((const char*)kv.first.hash.begin(), 32);
            unsigned char n[4];
            WriteLE32(n, kv.first.n);
            s.append((const char*)n, 4);
            s.append((const char*)kv.second.begin(), 32);
            spent.push_back(s);
        }
        std::sort(wtxs.begin(), wtxs.end());
        std::sort(spent.begin(), spent.end());
        pyb::list lw, ls;
        for (const std::string& s : wtxs) lw.append(pyb::bytes(s));
        for (const std::string& s : spent) ls.append(pyb::bytes(s));
        return pyb::make_tuple(v, lw, ls);
    }
};
const uint256 kScanBlockHash = uint256S("00000000000000000000000000000000000000000000000000000000000b10c0");
} // namespace

void bind_walletscan(pyb::module_& m) {
    m.attr("WM_HIT_K") = (int)wm::HIT_K;
    m.attr("WM_NOT_READ") = (int)wm::NOT_READ;
    m.attr("WM_HIT_W") = (int)wm::HIT_W;
    m.attr("WM_HIT_T") = (int)wm::HIT_T;
    m.attr("WM_HIT_S") = (int)wm::HIT_S;
    m.attr("WM_ITEM_TXID") = (int)wm::ITEM_TXID;
    m.attr("WM_ITEM_INPUT") = (int)wm::ITEM_INPUT;
    m.attr("WM_ITEM_OUTPUT") = (int)wm::ITEM_OUTPUT;
    m.attr("WM_MAX_PROBE") = (int)wm::WM_MAX_PROBE;
    m.attr("WM_LDS_MAX_BYTES") = (int)wm::WM_LDS_MAX_BYTES;
    m.def(
        "hash160_gpu",
        [](const std::vector<pyb::bytes>& messages, int device) {
            const Packed p = PackBytes(messages);
            std::vector<unsigned char> out;
            {
                pyb::gil_scoped_release rel;
                out = gpu::Hash160Batch(p.blob.data(), p.blob.size(), p.offs.data(), p.lens.data(), p.offs.size(), device);
            }
            std::vector<pyb::bytes> r;
            for (size_t i = 0; i < p.offs.size(); ++i) r.push_back(to_bytes(out.data() + 20 * i, 20));
            return r;
        },
        pyb::arg("messages"), pyb::arg("device") = -1);
    m.def(
        "hash160_device",
        [](uintptr_t blob, size_t blob_bytes, uintptr_t offs, uintptr_t lens, uintptr_t out, uintptr_t status, size_t n,
           int device, uintptr_t stream) {
            gpu::Hash160Device(reinterpret_cast<const void*>(blob), blob_bytes, reinterpret_cast<const void*>(offs),
                               reinterpret_cast<const void*>(lens), reinterpret_cast<void*>(out),
                               reinterpret_cast<void*>(status), n, device, stream);
        },
        pyb::arg("blob_ptr"), pyb::arg("blob_bytes"), pyb::arg("offs_ptr"), pyb::arg("lens_ptr"), pyb::arg("out_ptr"),
        pyb::arg("status_ptr"), pyb::arg("n"), pyb::arg("device"), pyb::arg("stream"));
    // RIPEMD160 of a 32-byte message by the code the device runs (kernels/wallet_match.h)
    m.def("wallet_match_ripemd160_32", [](const pyb::bytes& digest) {
        const std::vector<unsigned char> v = to_vec(digest);
        if (v.size() != 32) throw std::invalid_argument("32 bytes expected");
        uint32_t d[8], o[5];
        for (int i = 0; i < 8; ++i) d[i] = wm::LoadLE32(v.data() + 4 * i);
        wm::Ripemd160Of32(d, o);
        unsigned char out[20];
        for (int i = 0; i < 5; ++i) WriteLE32(out + 4 * i, o[i]);
        return to_bytes(out, 20);
    });
    m.def(
        "wallet_fingerprint",
        [](const pyb::bytes& salt, const pyb::bytes& data) {
            const std::vector<unsigned char> s = to_vec(salt), v = to_vec(data);
            if (s.size() != 16) throw std::invalid_argument("salt of 16 bytes expected");
            return wm::Fingerprint(wm::LoadLE64(s.data()), wm::LoadLE64(s.data() + 8), v.data(), (uint32_t)v.size());
        },
        pyb::arg("salt"), pyb::arg("data"));
    // the table of a description: its slots (little-endian uint64), salt words and counts
    m.def("wallet_match_table", [](const pyb::dict& table_desc) {
        const WalletMatchTable t = BuildTable(table_desc);
        pyb::dict d;
        d["slots"] = to_bytes(reinterpret_cast<const unsigned char*>(t.Data()), (size_t)t.Slots() * 8);
        d["n_slots"] = t.Slots();
        d["k0"] = t.K0();
        d["k1"] = t.K1();
        d["has_watch"] = t.HasWatch();
        d["entries"] = t.Entries();
        return d;
    });
    m.def(
        "wallet_match_gpu",
        [](const pyb::dict& table_desc, const std::vector<std::pair<int, pyb::bytes>>& items, int device) {
            const WalletMatchTable t = BuildTable(table_desc);
            const Packed p = PackItems(items);
            std::vector<uint8_t> flags;
            {
                pyb::gil_scoped_release rel;
                gpu::WalletMatchBatch(DescOf(t), p.kinds.data(), p.blob.data(), p.blob.size(), p.offs.data(), p.lens.data(),
                                      p.offs.size(), flags, device);
            }
            return std::vector<int>(flags.begin(), flags.end());
        },
        pyb::arg("table_desc"), pyb::arg("items"), pyb::arg("device") = -1);
    m.def(
        "wallet_match_cpu",
        [](const pyb::dict& table_desc, const std::vector<std::pair<int, pyb::bytes>>& items, uint32_t kind_mask) {
            const WalletMatchTable t = BuildTable(table_desc);
            const Packed p = PackItems(items);
            std::vector<uint8_t> flags(p.offs.size());
            WalletMatchCpu(t, kind_mask, p.kinds.data(), p.blob.data(), p.blob.size(), p.offs.data(), p.lens.data(),
                           p.offs.size(), flags.data());
            return std::vector<int>(flags.begin(), flags.end());
        },
        pyb::arg("table_desc"), pyb::arg("items"), pyb::arg("kind_mask") = (uint32_t)wm::KIND_MASK_ALL);
    // the twin over packed arrays as the device entry point takes them (items may reach past the blob)
    m.def(
        "wallet_match_cpu_packed",
        [](const pyb::dict& table_desc, const pyb::bytes& kinds, const pyb::bytes& blob, const std::vector<uint32_t>& offs,
           const std::vector<uint32_t>& lens, uint32_t kind_mask) {
            const WalletMatchTable t = BuildTable(table_desc);
            const std::vector<unsigned char> k = to_vec(kinds), b = to_vec(blob);
            if (k.size() != offs.size() || lens.size() != offs.size()) throw std::invalid_argument("kinds, offs, lens differ in length");
            std::vector<uint8_t> flags(offs.size());
            WalletMatchCpu(t, kind_mask, k.data(), b.data(), b.size(), offs.data(), lens.data(), offs.size(), flags.data());
            return std::vector<int>(flags.begin(), flags.end());
        },
        pyb::arg("table_desc"), pyb::arg("kinds"), pyb::arg("blob"), pyb::arg("offs"), pyb::arg("lens"),
        pyb::arg("kind_mask") = (uint32_t)wm::KIND_MASK_ALL);
    m.def(
        "wallet_match_device",
        [](uintptr_t slots, uint32_t n_slots, uint64_t k0, uint64_t k1, bool has_watch, uint32_t kind_mask, uintptr_t kinds,
           uintptr_t blob, size_t blob_bytes, uintptr_t offs, uintptr_t lens, uintptr_t flags, size_t n, int device,
           uintptr_t stream) {
            gpu::WalletMatchDevice(reinterpret_cast<const void*>(slots), n_slots, k0, k1, has_watch, kind_mask,
                                   reinterpret_cast<const void*>(kinds), reinterpret_cast<const void*>(blob), blob_bytes,
                                   reinterpret_cast<const void*>(offs), reinterpret_cast<const void*>(lens),
                                   reinterpret_cast<void*>(flags), n, device, stream);
        },
        pyb::arg("slots_ptr"), pyb::arg("n_slots"), pyb::arg("k0"), pyb::arg("k1"), pyb::arg("has_watch"),
        pyb::arg("kind_mask"), pyb::arg("kinds_ptr"), pyb::arg("blob_ptr"), pyb::arg("blob_bytes"), pyb::arg("offs_ptr"),
        pyb::arg("lens_ptr"), pyb::arg("flags_ptr"), pyb::arg("n"), pyb::arg("device"), pyb::arg("stream"));
    // (verdicts, wallet transactions, spent outpoints, info) of WalletScanTransactions over a
    // memory-only wallet made from wallet_desc, the list taken as the block kScanBlockHash.
    // use_gpu without a device is an error (unless the node's fault injection stands in for one).
    m.def(
        "wallet_scan",
        [](const std::vector<pyb::bytes>& raw_txs, const pyb::dict& wallet_desc, bool use_gpu, bool f_update) {
            const std::vector<CTransactionRef> txs = DecodeTxs(raw_txs);
            if (use_gpu && !GpuFaultInjection() && !gpu::GpuAvailable())
                throw std::runtime_error("wallet_scan: use_gpu without a HIP device");
            CWallet w{"walletscan", "", true};
            FillWallet(w, wallet_desc);
            CBlockIndex index;
            index.phashBlock = &kScanBlockHash;
            WalletScanInfo info;
            std::vector<bool> v;
            {
                pyb::gil_scoped_release rel;
                v = WalletScanTransactions(w, txs, &index, f_update, use_gpu, &info);
            }
            pyb::dict d;
            d["items"] = info.items;
            d["passes"] = info.passes;
            d["cpu_reruns"] = info.cpuReruns;
            d["used_gpu"] = info.usedGpu;
            const pyb::tuple st = WalletScanAccessPy::State(v, w, txs);
            return pyb::make_tuple(st[0], st[1], st[2], d);
        },
        pyb::arg("raw_txs"), pyb::arg("wallet_desc"), pyb::arg("use_gpu"), pyb::arg("f_update") = true);
    m.def(
        "wallet_scan_reference",
        [](const std::vector<pyb::bytes>& raw_txs, const pyb::dict& wallet_desc, bool f_update) {
            const std::vector<CTransactionRef> txs = DecodeTxs(raw_txs);
            CWallet w{"walletscan", "", true};
            FillWallet(w, wallet_desc);
            CBlockIndex index;
            index.phashBlock = &kScanBlockHash;
            std::vector<bool> v;
            for (size_t i = 0; i < txs.size(); i++) v.push_back(w.AddToWalletIfInvolvingMe(txs[i], &index, (int)i, f_update));
            return WalletScanAccessPy::State(v, w, txs);
        },
        pyb::arg("raw_txs"), pyb::arg("wallet_desc"), pyb::arg("f_update") = true);
    m.def("wallet_scan_stats", []() {
        const WalletScanStats s = GetWalletScanStats();
        pyb::dict d;
        d["wallet_scans"] = s.wallet_scans;
        d["items"] = s.items;
        d["passes"] = s.passes;
        d["cpu_reruns"] = s.cpu_reruns;
        d["cpu_scans"] = s.cpu_scans;
        d["gpu_failures"] = s.gpu_failures;
        d["threshold"] = GetGpuWalletScanThreshold();
        return d;
    });
    m.def("wallet_scan_reset_failures", &ResetWalletScanFailures);
}

} // namespace py
} // namespace bcp
