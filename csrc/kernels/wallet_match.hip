// Wallet matching for CDNA4: which transactions of a block can concern the wallet at all.
//   K11 hash160_kernel: RIPEMD160(SHA256(m)) of a batch of byte strings of 0..520 bytes, one lane
//       per message (CHash160, reference src/hash.h:46-80).
//   K12 wallet_match_kernel: one lane per item (a txid, a prevout, a scriptPubKey) against the
//       wallet's match table (kernels/wallet_match.h): exact-set membership by salted 64-bit
//       fingerprints, for csrc/wallet/walletscan.cpp.
// The item code is kernels/wallet_match.h, compiled here for the device and in
// csrc/wallet/walletmatch.cpp for the host, so both give the same flags.
//
// Public-key pushes are hashed in place, by the lane that walks the script, not compacted into a
// second hash160_kernel pass. Read from the gfx950 ISA of this file: with HASH160 inlined into the
// walk wallet_match_kernel takes 91 VGPRs (5 waves per SIMD), no AGPRs and no scratch, against 63
// VGPRs for hash160_kernel alone, so inlining spills nothing and in-place hashing costs the other
// lanes of a wave only the wait for the lanes that met a key: three compressions per compressed
// key. A second pass would add a compaction (atomics and a second list of offsets), a launch and
// a dependent flag merge to every scan, to save that wait in the waves that hold a P2PK or
// bare-multisig output, which are rare in blocks after 2012. The kernel is 20-50 us of a scan
// that takes 0.5 ms end to end on a 21k-transaction block (profiles/wallet_scan.md).
#include <hip/hip_runtime.h>

#include "kernels/gpu_api.h"
#include "kernels/hip_util.h"
#include "kernels/relay_ctx.h"
#include "kernels/sha256_device.h"
#include "kernels/wallet_match.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>

namespace bcpk {

using namespace bcp::wm;

constexpr uint32_t HASH160_MAX_BYTES = 520; // MAX_SCRIPT_ELEMENT_SIZE

// SHA-256 of len bytes at any byte offset: every block's sixteen words are built in registers
// from byte loads that stay inside the message; s = the digest as big-endian words.
__device__ __forceinline__ void sha256_bytes(const uint8_t* p, uint32_t len, uint32_t s[8]) {
    const uint32_t nblk = (len + 9 + 63) >> 6;
    sha256_init(s);
    for (uint32_t b = 0; b < nblk; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t at = b * 64 + 4 * j;
            uint32_t v = 0;
            if (at + 4 <= len) {
                const uint8_t* q = p + at;
                v = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
            } else if (at <= len) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t idx = at + k;
                    const uint32_t byte = idx < len ? p[idx] : (idx == len ? 0x80u : 0u);
                    v |= byte << (24 - 8 * k);
                }
            }
            w[j] = v;
        }
        if (b == nblk - 1) w[15] = len << 3; // w[14], the length's high word, is already 0
        sha256_transform(s, w);
    }
}

// id = RIPEMD160(SHA256(p[0..len))) as five little-endian words
__device__ __forceinline__ void hash160_words(const uint8_t* p, uint32_t len, uint32_t id[5]) {
    uint32_t s[8], d[8];
    sha256_bytes(p, len, s);
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = bswap32d(s[i]);
    Ripemd160Of32(d, id);
}

// out[20 * i ..] = HASH160(blob[offs[i] .. offs[i] + lens[i])). A message longer than 520 bytes or
// one that reaches past the blob is not read: its 20 bytes are zero and status[i] = 2 (else 1).
__global__ __launch_bounds__(256) void hash160_kernel(const uint8_t* __restrict__ blob, uint64_t blobBytes,
                                                      const uint32_t* __restrict__ offs,
                                                      const uint32_t* __restrict__ lens, uint8_t* __restrict__ out,
                                                      uint8_t* __restrict__ status, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t off = offs[i], len = lens[i];
    uint32_t id[5] = {0, 0, 0, 0, 0};
    const bool ok = len <= HASH160_MAX_BYTES && off <= blobBytes && len <= blobBytes - off;
    if (ok) hash160_words(blob + off, len, id);
    uint8_t* o = out + 20 * i;
#pragma unroll
    for (int w = 0; w < 5; ++w) {
        o[4 * w] = (uint8_t)id[w];
        o[4 * w + 1] = (uint8_t)(id[w] >> 8);
        o[4 * w + 2] = (uint8_t)(id[w] >> 16);
        o[4 * w + 3] = (uint8_t)(id[w] >> 24);
    }
    status[i] = ok ? 1 : 2;
}

struct DeviceHash160 {
    __device__ __forceinline__ void operator()(const uint8_t* p, uint32_t len, uint32_t id[5]) const {
        hash160_words(p, len, id);
    }
};

// flags[i] = MatchItem(table, item i), NOT_READ for an item that reaches past the blob. LDS: the
// table is copied to dynamic LDS (nSlots * 8 bytes) by every block, else read from device memory.
template <bool LDS>
__global__ __launch_bounds__(256) void wallet_match_kernel(const uint64_t* __restrict__ slots, uint32_t nSlots,
                                                           uint64_t k0, uint64_t k1, uint32_t hasWatch,
                                                           uint32_t kindMask, const uint8_t* __restrict__ kinds,
                                                           const uint8_t* __restrict__ blob, uint64_t blobBytes,
                                                           const uint32_t* __restrict__ offs,
                                                           const uint32_t* __restrict__ lens,
                                                           uint8_t* __restrict__ flags, size_t n) {
    extern __shared__ uint64_t s_slots[];
    TableView t;
    t.mask = nSlots - 1;
    t.k0 = k0;
    t.k1 = k1;
    t.hasWatch = hasWatch;
    if (LDS) {
        for (uint32_t w = threadIdx.x; w < nSlots; w += blockDim.x) s_slots[w] = slots[w];
        __syncthreads();
        t.slots = s_slots;
    } else {
        t.slots = slots;
    }
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t off = offs[i], len = lens[i];
        uint8_t f = NOT_READ;
        if (off <= blobBytes && len <= blobBytes - off) f = MatchItem(t, kindMask, kinds[i], blob + off, len, DeviceHash160());
        flags[i] = f;
    }
}

} // namespace bcpk

namespace bcp {
namespace gpu {

namespace {
void CheckTable(const WalletMatchTableDesc& t) {
    if (!t.slots) throw std::invalid_argument("wallet match: no table");
    if (t.nSlots < wm::WM_MIN_SLOTS || t.nSlots > (1u << 28) || (t.nSlots & (t.nSlots - 1)))
        throw std::invalid_argument("wallet match: slot count is not a power of two in 8..2^28");
}
void LaunchWalletMatch(hipStream_t s, const uint64_t* d_slots, uint32_t nSlots, uint64_t k0, uint64_t k1, bool hasWatch,
                       uint32_t kindMask, const uint8_t* d_kinds, const unsigned char* d_blob, uint64_t blobBytes,
                       const uint32_t* d_offs, const uint32_t* d_lens, unsigned char* d_flags, size_t n) {
    const size_t tableBytes = (size_t)nSlots * 8;
    if (tableBytes <= wm::WM_LDS_MAX_BYTES) {
        // every block copies the table first (at most 32 slots per lane)
        const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 1024);
        hipLaunchKernelGGL(bcpk::wallet_match_kernel<true>, dim3(blocks), dim3(256), tableBytes, s, d_slots, nSlots, k0, k1,
                           hasWatch ? 1u : 0u, kindMask, d_kinds, d_blob, blobBytes, d_offs, d_lens, d_flags, n);
    } else {
        const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(bcpk::wallet_match_kernel<false>, dim3(blocks), dim3(256), 0, s, d_slots, nSlots, k0, k1,
                           hasWatch ? 1u : 0u, kindMask, d_kinds, d_blob, blobBytes, d_offs, d_lens, d_flags, n);
    }
    BCP_HIP_CHECK(hipGetLastError());
}
void LaunchHash160(hipStream_t s, const unsigned char* d_blob, uint64_t blobBytes, const uint32_t* d_offs,
                   const uint32_t* d_lens, unsigned char* d_out, unsigned char* d_status, size_t n) {
    hipLaunchKernelGGL(bcpk::hash160_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_blob, blobBytes, d_offs,
                       d_lens, d_out, d_status, n);
    BCP_HIP_CHECK(hipGetLastError());
}
size_t Align8(size_t x) { return (x + 7) & ~(size_t)7; }
} // namespace

// ------------------------------------------------------------------ HASH160
std::vector<unsigned char> Hash160Batch(const unsigned char* blob, size_t blobBytes, const uint32_t* offs,
                                        const uint32_t* lens, size_t n, int device) {
    std::vector<unsigned char> out(n * 20);
    if (!n) return out;
    if (blobBytes > 0xFFFFFFFFu) throw std::invalid_argument("hash160: more than 4 GiB of messages");
    for (size_t i = 0; i < n; ++i) {
        if (lens[i] > bcpk::HASH160_MAX_BYTES) throw std::invalid_argument("hash160: message longer than 520 bytes");
        if (offs[i] > blobBytes || lens[i] > blobBytes - offs[i]) throw std::invalid_argument("hash160: message reaches past the blob");
    }
    device = UseDevice(device);
    RelayCtx& c = Ctx(device);
    auto l = Lock(c);
    const size_t inBytes = n * 8 + blobBytes, outBytes = n * 21;
    unsigned char* h_in = c.st.Host(0, inBytes + 1);
    unsigned char* d_in = c.st.Dev(0, inBytes + 1);
    unsigned char* h_out = c.st.Host(1, outBytes);
    unsigned char* d_out = c.st.Dev(1, outBytes);
    memcpy(h_in, offs, n * 4);
    memcpy(h_in + n * 4, lens, n * 4);
    if (blobBytes) memcpy(h_in + n * 8, blob, blobBytes);
    try {
        BCP_HIP_CHECK(hipMemcpyAsync(d_in, h_in, inBytes, hipMemcpyHostToDevice, c.s));
        LaunchHash160(c.s, d_in + n * 8, blobBytes, reinterpret_cast<const uint32_t*>(d_in),
                      reinterpret_cast<const uint32_t*>(d_in) + n, d_out, d_out + n * 20, n);
        BCP_HIP_CHECK(hipMemcpyAsync(h_out, d_out, outBytes, hipMemcpyDeviceToHost, c.s));
        BCP_HIP_CHECK(hipStreamSynchronize(c.s));
    } catch (...) {
        (void)hipStreamSynchronize(c.s); // nothing may still read the pinned staging
        throw;
    }
    for (size_t i = 0; i < n; ++i)
        if (h_out[n * 20 + i] != 1) throw std::runtime_error("hash160: the kernel did not read a checked message");
    memcpy(out.data(), h_out, n * 20);
    return out;
}

void Hash160Device(const void* blob, size_t blobBytes, const void* offs, const void* lens, void* out20, void* status,
                   size_t n, int device, uintptr_t stream) {
    if (!n) return;
    if (reinterpret_cast<uintptr_t>(offs) % 4 || reinterpret_cast<uintptr_t>(lens) % 4)
        throw std::invalid_argument("Hash160Device: offsets or lengths not 4-byte aligned");
    DeviceScope ds(device);
    LaunchHash160(reinterpret_cast<hipStream_t>(stream), static_cast<const unsigned char*>(blob), blobBytes,
                  static_cast<const uint32_t*>(offs), static_cast<const uint32_t*>(lens),
                  static_cast<unsigned char*>(out20), static_cast<unsigned char*>(status), n);
}

// ------------------------------------------------------------------ wallet match
struct WalletMatchItems::Impl {
    int device = 0;
    HostBuf<unsigned char> host;
    DevBuf<unsigned char> dev;
    size_t n = 0, blobBytes = 0;
    bool committed = false, resident = false;
    size_t Bytes() const { return n * 9 + blobBytes; }
    struct Table {
        HostBuf<uint64_t> host;
        DevBuf<uint64_t> dev;
        uint32_t nSlots = 0;
        uint64_t k0 = 0, k1 = 0;
        bool hasWatch = false;
        bool set = false, resident = false;
        std::vector<uint32_t> patches; // slots changed since the upload
    } tab[2];
};

WalletMatchItems::WalletMatchItems(int device) : impl(new Impl) { impl->device = UseDevice(device); }
WalletMatchItems::~WalletMatchItems() {}
int WalletMatchItems::Device() const { return impl->device; }
size_t WalletMatchItems::Size() const { return impl->committed ? impl->n : 0; }

void WalletMatchItems::Stage(size_t n, size_t blobBytes, uint8_t** kinds, uint32_t** offs, uint32_t** lens,
                             unsigned char** blob) {
    if (n > 0xFFFFFFFFu || blobBytes > 0xFFFFFFFFu) throw std::invalid_argument("wallet match items: more than 2^32 items or bytes");
    Impl& t = *impl;
    t.committed = t.resident = false;
    t.n = n;
    t.blobBytes = blobBytes;
    UseDevice(t.device);
    // every copy out of this buffer is waited for by the Match that issued it
    if (t.host.n < t.Bytes() + 1) t.host.alloc(t.Bytes() + t.Bytes() / 2 + 1);
    *offs = reinterpret_cast<uint32_t*>(t.host.p);
    *lens = *offs + n;
    *kinds = reinterpret_cast<uint8_t*>(*lens + n);
    *blob = *kinds + n;
}

void WalletMatchItems::Commit() {
    Impl& t = *impl;
    const uint32_t* offs = reinterpret_cast<const uint32_t*>(t.host.p);
    const uint32_t* lens = offs + t.n;
    const uint8_t* kinds = reinterpret_cast<const uint8_t*>(lens + t.n);
    for (size_t i = 0; i < t.n; ++i) {
        if (kinds[i] > wm::ITEM_OUTPUT) throw std::invalid_argument("wallet match items: unknown item kind");
        if (offs[i] > t.blobBytes || lens[i] > t.blobBytes - offs[i])
            throw std::invalid_argument("wallet match items: item reaches past the blob");
    }
    t.committed = true;
}

void WalletMatchItems::SetTable(int which, const WalletMatchTableDesc& d) {
    if (which < 0 || which > 1) throw std::invalid_argument("wallet match items: table 0 or 1");
    CheckTable(d);
    Impl::Table& T = impl->tab[which];
    UseDevice(impl->device);
    if (T.host.n < d.nSlots) T.host.alloc(d.nSlots);
    memcpy(T.host.p, d.slots, (size_t)d.nSlots * 8);
    T.nSlots = d.nSlots;
    T.k0 = d.k0;
    T.k1 = d.k1;
    T.hasWatch = d.hasWatch;
    T.set = true;
    T.resident = false;
    T.patches.clear();
}

void WalletMatchItems::PatchTable(int which, const uint32_t* idx, size_t n, const WalletMatchTableDesc& d) {
    if (which < 0 || which > 1) throw std::invalid_argument("wallet match items: table 0 or 1");
    CheckTable(d);
    Impl::Table& T = impl->tab[which];
    if (!T.set || T.nSlots != d.nSlots || T.k0 != d.k0 || T.k1 != d.k1)
        throw std::logic_error("wallet match items: PatchTable of another table");
    for (size_t i = 0; i < n; ++i) {
        if (idx[i] >= d.nSlots) throw std::invalid_argument("wallet match items: patched slot out of range");
        T.host.p[idx[i]] = d.slots[idx[i]];
    }
    T.hasWatch = d.hasWatch;
    if (!T.resident) return; // the whole table is still to be uploaded
    T.patches.insert(T.patches.end(), idx, idx + n);
    if (T.patches.size() > 64) { // cheaper as one copy
        T.patches.clear();
        T.resident = false;
    }
}

void WalletMatchItems::Match(int which, size_t first, uint32_t kindMask, uint8_t* flags) {
    if (which < 0 || which > 1) throw std::invalid_argument("wallet match items: table 0 or 1");
    Impl& t = *impl;
    Impl::Table& T = t.tab[which];
    if (!t.committed) throw std::logic_error("wallet match items: Match before Commit");
    if (!T.set) throw std::logic_error("wallet match items: Match before SetTable");
    if (first > t.n) throw std::invalid_argument("wallet match items: first item out of range");
    const size_t cnt = t.n - first;
    if (!cnt) return;
    UseDevice(t.device);
    RelayCtx& c = Ctx(t.device);
    auto l = Lock(c);
    if (t.dev.n < t.Bytes() + 1) {
        t.dev.alloc(t.Bytes() + t.Bytes() / 2 + 1);
        t.resident = false;
    }
    if (T.dev.n < T.nSlots) {
        T.dev.alloc(T.nSlots);
        T.resident = false;
    }
    unsigned char* h_out = c.st.Host(1, cnt);
    unsigned char* d_out = c.st.Dev(1, cnt);
    try {
        if (!t.resident) BCP_HIP_CHECK(hipMemcpyAsync(t.dev.p, t.host.p, t.Bytes(), hipMemcpyHostToDevice, c.s));
        if (!T.resident) {
            BCP_HIP_CHECK(hipMemcpyAsync(T.dev.p, T.host.p, (size_t)T.nSlots * 8, hipMemcpyHostToDevice, c.s));
        } else {
            for (uint32_t s : T.patches)
                BCP_HIP_CHECK(hipMemcpyAsync(T.dev.p + s, T.host.p + s, 8, hipMemcpyHostToDevice, c.s));
        }
        const uint32_t* d_offs = reinterpret_cast<const uint32_t*>(t.dev.p);
        const uint32_t* d_lens = d_offs + t.n;
        const uint8_t* d_kinds = reinterpret_cast<const uint8_t*>(d_lens + t.n);
        const unsigned char* d_blob = d_kinds + t.n;
        LaunchWalletMatch(c.s, T.dev.p, T.nSlots, T.k0, T.k1, T.hasWatch, kindMask, d_kinds + first, d_blob, t.blobBytes,
                          d_offs + first, d_lens + first, d_out, cnt);
        BCP_HIP_CHECK(hipMemcpyAsync(h_out, d_out, cnt, hipMemcpyDeviceToHost, c.s));
        BCP_HIP_CHECK(hipStreamSynchronize(c.s));
    } catch (...) {
        (void)hipStreamSynchronize(c.s); // nothing may still read the pinned staging
        t.resident = T.resident = false;
        T.patches.clear();
        throw;
    }
    t.resident = T.resident = true;
    T.patches.clear();
    memcpy(flags, h_out, cnt);
}

void WalletMatchBatch(const WalletMatchTableDesc& table, const uint8_t* kinds, const unsigned char* blob, size_t blobBytes,
                      const uint32_t* offs, const uint32_t* lens, size_t n, std::vector<uint8_t>& flags, int device) {
    CheckTable(table);
    flags.assign(n, 0);
    device = UseDevice(device);
    static std::mutex tm[64];
    static std::unique_ptr<WalletMatchItems> items[64];
    Ctx(device); // range check
    std::lock_guard<std::mutex> lt(tm[device]);
    if (!items[device]) items[device].reset(new WalletMatchItems(device));
    WalletMatchItems& t = *items[device];
    uint8_t* sk;
    uint32_t *so, *sl;
    unsigned char* sb;
    t.Stage(n, blobBytes, &sk, &so, &sl, &sb);
    if (n) {
        memcpy(sk, kinds, n);
        memcpy(so, offs, n * 4);
        memcpy(sl, lens, n * 4);
    }
    if (blobBytes) memcpy(sb, blob, blobBytes);
    t.Commit();
    t.SetTable(0, table);
    t.Match(0, 0, wm::KIND_MASK_ALL, flags.data());
}

void WalletMatchDevice(const void* slots, uint32_t nSlots, uint64_t k0, uint64_t k1, bool hasWatch, uint32_t kindMask,
                       const void* kinds, const void* blob, size_t blobBytes, const void* offs, const void* lens,
                       void* flags, size_t n, int device, uintptr_t stream) {
    WalletMatchTableDesc d{static_cast<const uint64_t*>(slots), nSlots, k0, k1, hasWatch};
    CheckTable(d);
    if (!n) return;
    if (reinterpret_cast<uintptr_t>(slots) % 8) throw std::invalid_argument("WalletMatchDevice: table not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(offs) % 4 || reinterpret_cast<uintptr_t>(lens) % 4)
        throw std::invalid_argument("WalletMatchDevice: offsets or lengths not 4-byte aligned");
    DeviceScope ds(device);
    LaunchWalletMatch(reinterpret_cast<hipStream_t>(stream), d.slots, nSlots, k0, k1, hasWatch, kindMask,
                      static_cast<const uint8_t*>(kinds), static_cast<const unsigned char*>(blob), blobBytes,
                      static_cast<const uint32_t*>(offs), static_cast<const uint32_t*>(lens),
                      static_cast<unsigned char*>(flags), n);
}

} // namespace gpu
} // namespace bcp
