// Python bindings for BIP37 filter matching: the membership kernel (csrc/kernels/relay.hip), its
// CPU oracles, and the exact scan of a transaction list (csrc/net/bloomscan.h).
#include "consensus/merkleblock.h"
#include "kernels/gpu_api.h"
#include "net/bloomscan.h"
#include "primitives/serialize.h"
#include "python/bind.h"
#include "util/util.h"

namespace bcp {
namespace py {

namespace {
struct PackedElements {
    std::vector<unsigned char> blob;
    std::vector<uint32_t> offs, lens;
};
PackedElements Pack(const std::vector<pyb::bytes>& elements) {
    PackedElements p;
    for (const pyb::bytes& e : elements) {
        const std::string s = e;
        p.offs.push_back((uint32_t)p.blob.size());
        p.lens.push_back((uint32_t)s.size());
        p.blob.insert(p.blob.end(), s.begin(), s.end());
    }
    return p;
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
// a filterload payload, brought to the state net processing keeps it in
CBloomFilter DecodeFilter(const pyb::bytes& ser) {
    const std::vector<unsigned char> v = to_vec(ser);
    SpanReader r(v.data(), v.size(), SER_NETWORK, PROTOCOL_VERSION);
    CBloomFilter f;
    r >> f;
    f.UpdateEmptyFull();
    return f;
}
pyb::list Verdicts(const std::vector<bool>& v) {
    pyb::list l;
    for (bool b : v) l.append(b);
    return l;
}
} // namespace

void bind_bloom(pyb::module_& m) {
    m.def(
        "murmur3",
        [](uint32_t seed, const pyb::bytes& data) {
            const std::string s = data;
            return MurmurHash3(seed, reinterpret_cast<const unsigned char*>(s.data()), s.size());
        },
        pyb::arg("seed"), pyb::arg("data"));
    // CBloomFilter::contains of a filter that is neither flagged full nor empty, from its parts
    m.def(
        "bloom_contains_cpu",
        [](const pyb::bytes& filter, uint32_t n_hash, uint32_t tweak, const std::vector<pyb::bytes>& elements) {
            const std::vector<unsigned char> f = to_vec(filter);
            if (f.empty()) throw std::invalid_argument("bloom_contains_cpu: empty filter");
            const uint32_t nBits = (uint32_t)f.size() * 8;
            std::vector<int> out;
            for (const pyb::bytes& e : elements) {
                const std::string s = e;
                bool ok = true;
                for (uint32_t h = 0; h < n_hash && ok; h++) {
                    const uint32_t bit =
                        MurmurHash3(h * 0xFBA4C795 + tweak, reinterpret_cast<const unsigned char*>(s.data()), s.size()) % nBits;
                    ok = (f[bit >> 3] >> (bit & 7)) & 1;
                }
                out.push_back(ok);
            }
            return out;
        },
        pyb::arg("filter"), pyb::arg("n_hash"), pyb::arg("tweak"), pyb::arg("elements"));
    m.def(
        "bloom_match_gpu",
        [](const pyb::bytes& filter, uint32_t n_hash, uint32_t tweak, const std::vector<pyb::bytes>& elements, int device) {
            const std::vector<unsigned char> f = to_vec(filter);
            const PackedElements p = Pack(elements);
            std::vector<uint8_t> match;
            {
                pyb::gil_scoped_release rel;
                gpu::BloomMatchBatch(f.data(), (uint32_t)std::min<size_t>(f.size(), 0xFFFFFFFFu), n_hash, tweak, p.blob.data(),
                                     p.blob.size(), p.offs.data(), p.lens.data(), p.offs.size(), match, device);
            }
            return std::vector<int>(match.begin(), match.end());
        },
        pyb::arg("filter"), pyb::arg("n_hash"), pyb::arg("tweak"), pyb::arg("elements"), pyb::arg("device") = -1);
    m.def(
        "bloom_match_device",
        [](uintptr_t filter, uint32_t filter_bytes, uint32_t n_hash, uint32_t tweak, uintptr_t blob, size_t blob_bytes,
           uintptr_t offs, uintptr_t lens, uintptr_t match, size_t n, int device, uintptr_t stream) {
            gpu::BloomMatchDevice(reinterpret_cast<const void*>(filter), filter_bytes, n_hash, tweak,
                                  reinterpret_cast<const void*>(blob), blob_bytes, reinterpret_cast<const void*>(offs),
                                  reinterpret_cast<const void*>(lens), reinterpret_cast<void*>(match), n, device, stream);
        },
        pyb::arg("filter_ptr"), pyb::arg("filter_bytes"), pyb::arg("n_hash"), pyb::arg("tweak"), pyb::arg("blob_ptr"),
        pyb::arg("blob_bytes"), pyb::arg("offs_ptr"), pyb::arg("lens_ptr"), pyb::arg("match_ptr"), pyb::arg("n"),
        pyb::arg("device"), pyb::arg("stream"));
    // (verdicts, the filter's payload afterwards, info) of BloomScanTransactions. use_gpu without a
    // device is an error (unless the node's fault injection stands in for one).
    m.def(
        "bloom_scan",
        [](const std::vector<pyb::bytes>& raw_txs, const pyb::bytes& filter_ser, bool use_gpu) {
            const std::vector<CTransactionRef> txs = DecodeTxs(raw_txs);
            CBloomFilter f = DecodeFilter(filter_ser);
            if (use_gpu && !GpuFaultInjection() && !gpu::GpuAvailable())
                throw std::runtime_error("bloom_scan: use_gpu without a HIP device");
            BloomScanInfo info;
            std::vector<bool> v;
            {
                pyb::gil_scoped_release rel;
                v = BloomScanTransactions(txs, f, use_gpu, &info);
            }
            pyb::dict d;
            d["elements"] = info.elements;
            d["rounds"] = info.rounds;
            d["cpu_reruns"] = info.cpuReruns;
            d["used_gpu"] = info.usedGpu;
            return pyb::make_tuple(Verdicts(v), to_bytes(SerializeToBytes(f)), d);
        },
        pyb::arg("raw_txs"), pyb::arg("filter_ser"), pyb::arg("use_gpu"));
    m.def(
        "bloom_scan_reference",
        [](const std::vector<pyb::bytes>& raw_txs, const pyb::bytes& filter_ser) {
            const std::vector<CTransactionRef> txs = DecodeTxs(raw_txs);
            CBloomFilter f = DecodeFilter(filter_ser);
            std::vector<bool> v;
            for (const CTransactionRef& tx : txs) v.push_back(f.IsRelevantAndUpdate(*tx));
            return pyb::make_tuple(Verdicts(v), to_bytes(SerializeToBytes(f)));
        },
        pyb::arg("raw_txs"), pyb::arg("filter_ser"));
    m.def("bloom_scan_stats", []() {
        const BloomScanStats s = GetBloomScanStats();
        pyb::dict d;
        d["gpu_scans"] = s.gpu_scans;
        d["gpu_elements"] = s.gpu_elements;
        d["rounds"] = s.rounds;
        d["cpu_reruns"] = s.cpu_reruns;
        d["cpu_scans"] = s.cpu_scans;
        d["gpu_failures"] = s.gpu_failures;
        d["threshold"] = GetGpuBloomThreshold();
        return d;
    });
    m.def("bloom_scan_reset_failures", &ResetBloomScanFailures);
}

} // namespace py
} // namespace bcp
