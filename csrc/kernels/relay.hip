// Relay-path batch kernels for CDNA4:
//   K9  BIP152 short transaction ids (SipHash-2-4 of a txid, 48 bits): the mempool side of
//       compact-block reconstruction, reference src/blockencodings.cpp:37-42 and
//       PartiallyDownloadedBlock::InitData (:67-178), SipHashUint256 src/hash.cpp:181-300;
//   K10 BIP37 bloom-filter membership of a batch of byte strings (MurmurHash3 x86_32, up to 50
//       probes of a filter of up to 36,000 bytes): CBloomFilter::contains, reference
//       src/bloom.cpp:82-91 and src/hash.cpp:14-73, for the filtered-block and mempool replies.
// One lane per item; 64-bit SipHash words stay in VGPR pairs (v_lshl_add_u64 adds,
// v_alignbit rotates). The bloom kernel keeps the filter in LDS and an element's words, already
// through the seed-independent half of the Murmur block step, in VGPRs across the probes.
#include <hip/hip_runtime.h>

#include "kernels/gpu_api.h"
#include "kernels/hip_util.h"
#include "kernels/relay_ctx.h"
#include "kernels/siphash.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>

namespace bcpk {

__global__ __launch_bounds__(256) void shortid_kernel(uint64_t k0, uint64_t k1, const uint4* __restrict__ txids,
                                                      uint64_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 a = txids[2 * i], b = txids[2 * i + 1];
    const uint64_t d[4] = {((uint64_t)a.y << 32) | a.x, ((uint64_t)a.w << 32) | a.z, ((uint64_t)b.y << 32) | b.x,
                           ((uint64_t)b.w << 32) | b.z};
    bcp::sip::Sip s;
    s.Init(k0, k1);
#pragma unroll
    for (int w = 0; w < 4; ++w) s.Word(d[w]);
    s.Word(32ULL << 56); // message length 32 bytes, no tail bytes
    out[i] = s.Final() & 0xffffffffffffULL;
}

// ------------------------------------------------------------------ K10 bloom membership
constexpr uint32_t BLOOM_MAX_BYTES = 36000; // CBloomFilter::MAX_BLOOM_FILTER_SIZE
constexpr uint32_t BLOOM_MAX_FUNCS = 50;    // CBloomFilter::MAX_HASH_FUNCS
constexpr int BLOOM_REG_WORDS = 20;         // element words kept in VGPRs (80 bytes: a DER signature)

__device__ __forceinline__ uint32_t rotl32d(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
// The part of a Murmur block step that does not depend on the running hash.
__device__ __forceinline__ uint32_t murmur_premix(uint32_t k) {
    k *= 0xcc9e2d51u;
    k = rotl32d(k, 15);
    return k * 0x1b873593u;
}
__device__ __forceinline__ uint32_t murmur_step(uint32_t h, uint32_t k) {
    h ^= k;
    h = rotl32d(h, 13);
    return h * 5 + 0xe6546b64u;
}
// Elements sit at any byte offset of the blob: byte loads, never past the element's last byte.
__device__ __forceinline__ uint32_t load_le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// match[i] = 1 iff every one of the nHashFuncs probes of element i finds its bit set
// (MurmurHash3(h * 0xFBA4C795 + nTweak, element) % (filterBytes * 8)), 0 iff one does not, and
// 2 for an element that is empty or reaches past the blob (nothing of it is read). Dynamic LDS:
// filterBytes rounded up to a multiple of 4.
__global__ __launch_bounds__(256) void bloom_match_kernel(const uint8_t* __restrict__ filter, uint32_t filterBytes,
                                                          uint32_t nHashFuncs, uint32_t nTweak,
                                                          const uint8_t* __restrict__ blob, uint64_t blobBytes,
                                                          const uint32_t* __restrict__ offs,
                                                          const uint32_t* __restrict__ lens, uint8_t* __restrict__ match,
                                                          size_t n) {
    extern __shared__ uint32_t s_filter[];
    uint8_t* sf = reinterpret_cast<uint8_t*>(s_filter);
    if ((reinterpret_cast<uintptr_t>(filter) & 3) == 0) {
        const uint32_t words = filterBytes >> 2;
        const uint32_t* fw = reinterpret_cast<const uint32_t*>(filter);
        for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) s_filter[w] = fw[w];
        for (uint32_t b = (words << 2) + threadIdx.x; b < filterBytes; b += blockDim.x) sf[b] = filter[b];
    } else {
        for (uint32_t b = threadIdx.x; b < filterBytes; b += blockDim.x) sf[b] = filter[b];
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t off = offs[i], len = lens[i];
    if (len == 0 || off > blobBytes || len > blobBytes - off) {
        match[i] = 2;
        return;
    }
    const uint8_t* p = blob + off;
    const uint32_t nblocks = len >> 2;
    uint32_t k[BLOOM_REG_WORDS];
#pragma unroll
    for (int w = 0; w < BLOOM_REG_WORDS; ++w) k[w] = (uint32_t)w < nblocks ? murmur_premix(load_le32(p + 4 * w)) : 0;
    const uint8_t* tail = p + 4 * (size_t)nblocks;
    uint32_t kt = 0;
    if ((len & 3) >= 3) kt ^= (uint32_t)tail[2] << 16;
    if ((len & 3) >= 2) kt ^= (uint32_t)tail[1] << 8;
    if ((len & 3) >= 1) kt ^= tail[0];
    kt = murmur_premix(kt); // zero stays zero: no tail, no change to the hash
    const uint32_t nbits = filterBytes * 8;
    uint8_t ok = 1;
    for (uint32_t f = 0; f < nHashFuncs; ++f) {
        uint32_t h = f * 0xFBA4C795u + nTweak;
#pragma unroll
        for (int w = 0; w < BLOOM_REG_WORDS; ++w) h = (uint32_t)w < nblocks ? murmur_step(h, k[w]) : h;
        for (uint32_t w = BLOOM_REG_WORDS; w < nblocks; ++w) h = murmur_step(h, murmur_premix(load_le32(p + 4 * (size_t)w)));
        h ^= kt;
        h ^= len;
        h ^= h >> 16;
        h *= 0x85ebca6bu;
        h ^= h >> 13;
        h *= 0xc2b2ae35u;
        h ^= h >> 16;
        const uint32_t bit = h % nbits;
        if (!((sf[bit >> 3] >> (bit & 7)) & 1)) { // this lane is done; the others go on
            ok = 0;
            break;
        }
    }
    match[i] = ok;
}

} // namespace bcpk

namespace bcp {
namespace gpu {

std::vector<uint64_t> ShortTxIdBatch(uint64_t k0, uint64_t k1, const unsigned char* txids32, size_t n, int device) {
    std::vector<uint64_t> out(n);
    if (!n) return out;
    device = UseDevice(device);
    RelayCtx& c = Ctx(device);
    auto l = Lock(c);
    unsigned char* h_in = c.st.Host(0, n * 32);
    unsigned char* h_out = c.st.Host(1, n * 8);
    unsigned char* d_in = c.st.Dev(0, n * 32);
    unsigned char* d_out = c.st.Dev(1, n * 8);
    memcpy(h_in, txids32, n * 32);
    BCP_HIP_CHECK(hipMemcpyAsync(d_in, h_in, n * 32, hipMemcpyHostToDevice, c.s));
    hipLaunchKernelGGL(bcpk::shortid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.s, k0, k1,
                       reinterpret_cast<const uint4*>(d_in), reinterpret_cast<uint64_t*>(d_out), n);
    BCP_HIP_CHECK(hipGetLastError());
    BCP_HIP_CHECK(hipMemcpyAsync(h_out, d_out, n * 8, hipMemcpyDeviceToHost, c.s));
    BCP_HIP_CHECK(hipStreamSynchronize(c.s));
    memcpy(out.data(), h_out, n * 8);
    return out;
}

// ------------------------------------------------------------------ bloom membership
namespace {
void CheckBloomParams(uint32_t filterBytes, uint32_t nHashFuncs) {
    if (filterBytes == 0) throw std::invalid_argument("bloom match: empty filter");
    if (filterBytes > bcpk::BLOOM_MAX_BYTES) throw std::invalid_argument("bloom match: filter larger than 36000 bytes");
    if (nHashFuncs == 0 || nHashFuncs > bcpk::BLOOM_MAX_FUNCS)
        throw std::invalid_argument("bloom match: hash function count outside 1..50");
}
void LaunchBloomMatch(hipStream_t s, const unsigned char* d_filter, uint32_t filterBytes, uint32_t nHashFuncs,
                      uint32_t nTweak, const unsigned char* d_blob, uint64_t blobBytes, const uint32_t* d_offs,
                      const uint32_t* d_lens, unsigned char* d_match, size_t n) {
    hipLaunchKernelGGL(bcpk::bloom_match_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), (filterBytes + 3) & ~3u, s,
                       d_filter, filterBytes, nHashFuncs, nTweak, d_blob, blobBytes, d_offs, d_lens, d_match, n);
    BCP_HIP_CHECK(hipGetLastError());
}
// Start of the table proper in a BloomElementTable's buffers: the filter's bytes go in front of
// it, so a first match uploads filter and table in one copy and a later one the filter alone.
constexpr size_t BLOOM_TABLE_AT = (bcpk::BLOOM_MAX_BYTES + 63) & ~(size_t)63;
} // namespace

struct BloomElementTable::Impl {
    int device = 0;
    HostBuf<unsigned char> host;
    DevBuf<unsigned char> dev;
    size_t n = 0, blobBytes = 0;
    bool committed = false; // the staged table passed its checks
    bool resident = false;  // and is on the device
    size_t Bytes() const { return BLOOM_TABLE_AT + n * 8 + blobBytes; }
};

BloomElementTable::BloomElementTable(int device) : impl(new Impl) { impl->device = UseDevice(device); }
BloomElementTable::~BloomElementTable() {}
int BloomElementTable::Device() const { return impl->device; }
size_t BloomElementTable::Size() const { return impl->committed ? impl->n : 0; }

void BloomElementTable::Stage(size_t n, size_t blobBytes, uint32_t** offs, uint32_t** lens, unsigned char** blob) {
    if (n > 0xFFFFFFFFu || blobBytes > 0xFFFFFFFFu) throw std::invalid_argument("bloom element table: more than 2^32 elements or bytes");
    Impl& t = *impl;
    t.committed = t.resident = false;
    t.n = n;
    t.blobBytes = blobBytes;
    UseDevice(t.device);
    // every copy out of this buffer is waited for by the Match that issued it
    if (t.host.n < t.Bytes()) t.host.alloc(t.Bytes() + t.Bytes() / 2);
    *offs = reinterpret_cast<uint32_t*>(t.host.p + BLOOM_TABLE_AT);
    *lens = *offs + n;
    *blob = reinterpret_cast<unsigned char*>(*lens + n);
}

void BloomElementTable::Commit() {
    Impl& t = *impl;
    const uint32_t* offs = reinterpret_cast<const uint32_t*>(t.host.p + BLOOM_TABLE_AT);
    const uint32_t* lens = offs + t.n;
    for (size_t i = 0; i < t.n; ++i) {
        if (lens[i] == 0) throw std::invalid_argument("bloom element table: empty element");
        if (offs[i] > t.blobBytes || lens[i] > t.blobBytes - offs[i])
            throw std::invalid_argument("bloom element table: element reaches past the blob");
    }
    t.committed = true;
}

void BloomElementTable::Match(const unsigned char* filter, uint32_t filterBytes, uint32_t nHashFuncs, uint32_t nTweak,
                              size_t first, uint8_t* match) {
    CheckBloomParams(filterBytes, nHashFuncs);
    Impl& t = *impl;
    if (!t.committed) throw std::logic_error("bloom element table: Match before Commit");
    if (first > t.n) throw std::invalid_argument("bloom element table: first element out of range");
    const size_t cnt = t.n - first;
    if (!cnt) return;
    UseDevice(t.device);
    RelayCtx& c = Ctx(t.device);
    auto l = Lock(c);
    if (t.dev.n < t.Bytes()) {
        t.dev.alloc(t.Bytes() + t.Bytes() / 2);
        t.resident = false;
    }
    unsigned char* h_out = c.st.Host(1, cnt);
    unsigned char* d_out = c.st.Dev(1, cnt);
    memcpy(t.host.p, filter, filterBytes);
    BCP_HIP_CHECK(hipMemcpyAsync(t.dev.p, t.host.p, t.resident ? (size_t)filterBytes : t.Bytes(), hipMemcpyHostToDevice, c.s));
    const uint32_t* d_offs = reinterpret_cast<const uint32_t*>(t.dev.p + BLOOM_TABLE_AT);
    const uint32_t* d_lens = d_offs + t.n;
    const unsigned char* d_blob = reinterpret_cast<const unsigned char*>(d_lens + t.n);
    try {
        LaunchBloomMatch(c.s, t.dev.p, filterBytes, nHashFuncs, nTweak, d_blob, t.blobBytes, d_offs + first, d_lens + first,
                         d_out, cnt);
        BCP_HIP_CHECK(hipMemcpyAsync(h_out, d_out, cnt, hipMemcpyDeviceToHost, c.s));
        BCP_HIP_CHECK(hipStreamSynchronize(c.s));
    } catch (...) {
        (void)hipStreamSynchronize(c.s); // nothing may still read the pinned staging
        throw;
    }
    t.resident = true;
    memcpy(match, h_out, cnt);
}

void BloomMatchBatch(const unsigned char* filter, uint32_t filterBytes, uint32_t nHashFuncs, uint32_t nTweak,
                     const unsigned char* blob, size_t blobBytes, const uint32_t* offs, const uint32_t* lens, size_t n,
                     std::vector<uint8_t>& match, int device) {
    CheckBloomParams(filterBytes, nHashFuncs);
    match.assign(n, 0);
    device = UseDevice(device);
    // one table per device for this entry point, its own lock around stage + match
    static std::mutex tm[64];
    static std::unique_ptr<BloomElementTable> tables[64];
    Ctx(device); // range check
    std::lock_guard<std::mutex> lt(tm[device]);
    if (!tables[device]) tables[device].reset(new BloomElementTable(device));
    BloomElementTable& t = *tables[device];
    uint32_t *so, *sl;
    unsigned char* sb;
    t.Stage(n, blobBytes, &so, &sl, &sb);
    if (n) {
        memcpy(so, offs, n * 4);
        memcpy(sl, lens, n * 4);
    }
    if (blobBytes) memcpy(sb, blob, blobBytes);
    t.Commit();
    t.Match(filter, filterBytes, nHashFuncs, nTweak, 0, match.data());
}

void BloomMatchDevice(const void* filter, uint32_t filterBytes, uint32_t nHashFuncs, uint32_t nTweak, const void* blob,
                      size_t blobBytes, const void* offs, const void* lens, void* match, size_t n, int device,
                      uintptr_t stream) {
    CheckBloomParams(filterBytes, nHashFuncs);
    if (!n) return;
    if (reinterpret_cast<uintptr_t>(offs) % 4 || reinterpret_cast<uintptr_t>(lens) % 4)
        throw std::invalid_argument("BloomMatchDevice: offsets or lengths not 4-byte aligned");
    DeviceScope ds(device);
    LaunchBloomMatch(reinterpret_cast<hipStream_t>(stream), static_cast<const unsigned char*>(filter), filterBytes,
                     nHashFuncs, nTweak, static_cast<const unsigned char*>(blob), blobBytes,
                     static_cast<const uint32_t*>(offs), static_cast<const uint32_t*>(lens),
                     static_cast<unsigned char*>(match), n);
}

void ShortTxIdsDevice(uint64_t k0, uint64_t k1, const void* txids32, void* out64, size_t n, int device,
                      uintptr_t stream) {
    if (!n) return;
    if (reinterpret_cast<uintptr_t>(txids32) % 16) throw std::invalid_argument("ShortTxIdsDevice: txids not 16-byte aligned");
    DeviceScope ds(device);
    hipLaunchKernelGGL(bcpk::shortid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), k0, k1, static_cast<const uint4*>(txids32),
                       static_cast<uint64_t*>(out64), n);
    BCP_HIP_CHECK(hipGetLastError());
}

} // namespace gpu
} // namespace bcp
