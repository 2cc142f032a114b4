// Equihash solver for CDNA4 (gfx950) — the GPU replacement for the reference's
// CPU BasicSolve/OptimisedSolve (reference src/crypto/equihash.cpp:332-722,
// called from generateBlocks src/rpc/mining.cpp:161-199).
//
// Design: a bucket-sorted Wagner solver with parent pointers and contiguous buckets.
//
//  * Rows are bucketed on the top BB bits of the current digit (NB = 2^BB buckets, ~INIT/NB rows
//    each). (200,9) runs BB = 9: 512 buckets of ~4096 rows, one 1024-thread round workgroup per
//    CU (145 KiB of LDS). 1024 buckets of ~2048 rows with two 512-thread workgroups (<= 80 KiB
//    each) per CU measured slower (the phases are latency-bound per lane, and the producer runs
//    are 4x shorter), profiles/equihash_r4.md.
//    Every stage keeps each bucket CONTIGUOUS in its own area of AREA row slots.
//  * Every kernel works "one workgroup per bucket". A producer workgroup counting-sorts its
//    output rows by destination bucket in LDS, then claims one run per destination with ONE
//    device-scope atomicAdd on that bucket's fill counter (issued as soon as the histogram is
//    known so its latency hides behind the scan and scatter), and writes its rows into the
//    claimed runs. The consumer round then reads its bucket as one contiguous block (16-byte
//    loads, straight into LDS): no run tables, slot maps or per-row gather maps.
//  * Collisions on the remaining RB = DB-BB bits of the digit (the key) are found by grouping the
//    bucket's rows by key and listing the pairs of every group. The commit takes each row's rank
//    in its key group with a returning LDS atomic. A sorted round ((200,9) rounds 1-2, (48,5),
//    every final round) then scans the key counts and places the row ids in key order; a slot
//    round (EhCfg::ks: (200,9) rounds 3-8, (96,5)) needs no order: the commit writes the row's id
//    into slot `rank` of its key's 8 slots, a row later reads all its partners with one 16-byte
//    LDS load, and the few rows of rank >= 8 (about one per bucket) go through an overflow list.
//    That takes the key scan, the placement pass and three of ten barriers out of the bucket
//    iteration (profiles/equihash_r10.md). Each output
//    row keeps a parent triple (producing bucket, LDS row i, LDS row j; in its slot or, see Memory
//    layout, in the producing bucket's tables), so nothing ever carries
//    index lists: the parents of a stage-s row are the stage-(s-1) slots bucket*AREA + i and
//    bucket*AREA + j.
//  * Depth-1 duplicate pruning (pairs whose rows share a parent are dropped) wherever the parent
//    words fit in the round's LDS budget.
//  * Final round: pairs equal on all remaining bits are candidates; eh_expand walks the K levels
//    of parent triples, canonicalises subtree order (reference IsValidSolution ordering rule)
//    and rejects repeated indices (LDS bitonic sort).
//  * Block scans use DPP row shifts/broadcasts inside a wave and one LDS word per wave
//    across waves: two barriers per scan, no ds_bpermute traffic.
//  * Generation (VALU-bound, HBM idle) is hidden inside the collision rounds (memory- and
//    LDS-bound, VALU mostly idle). A launch is split into nonce groups; the stand-alone kernel
//    generates group 0 only, and the round workgroups of rounds 1..K-1 of every group give GW
//    of their waves to the generation of the next group (eh_carry_gen): nonce n's buckets hash
//    the chunks of nonce n + group size. Both kinds of wave meet at the round's own workgroup
//    barriers, the same number on either path; nothing waits across workgroups. The dispatcher
//    would not co-schedule separate generation and round kernels on a CU (profiles/equihash_r5.md);
//    inside one workgroup the placement is given. profiles/equihash_r7.md has the measurements.
// Memory layout and kernel geometry: equihash_layout.h (checked on the CPU by csrc/test/equihash_layout_tests.cpp).
#include <hip/hip_runtime.h>

#include "crypto/hashes.h"
#include "kernels/blake2b_device.h"
#include "kernels/equihash_layout.h"
#include "kernels/equihash_pow.h"
#include "kernels/gpu_api.h"
#include "kernels/hip_util.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <utility>

// Build options: numeric tuning values only (each either the measured default or covered by the GPU
// tests; the options that shape the layout are in equihash_layout.h). Variants whose A/B is over are
// not kept as switches: those measured and rejected in rounds 3-5 are at git tag solver-r5-knobs
// (profiles/equihash_r4.md, profiles/equihash_r5.md); the unmapped work order (XCD_MAP=0, 16-23%
// slower in rounds 1-4), the unrolled slot listing (SLOT_LIST=0, profiles/equihash_r10.md), the
// all-sorted rounds (KEY_SLOTS=0) and the slots with parent words everywhere (TABLE_PARENTS=0,
// profiles/equihash_r8.md) were last buildable at commit 3ff18da.
#ifndef BCP_EH_SLOT_RB // generation waves of a carrying slot round: the BLAKE2b round at which the slice of the
#define BCP_EH_SLOT_RB 5 //   commit interval stops, and (BCP_EH_SLOT_RD) the slice of the pair-listing interval
#endif
#ifndef BCP_EH_SLOT_RD
#define BCP_EH_SLOT_RD 10
#endif
#ifndef BCP_EH_GROUPS_DEFAULT // nonce groups of a solver by its batch size (BCP_EH_GROUPS overrides at run time):
#define BCP_EH_GROUPS_DEFAULT(batch) ((batch) >= 48 ? (batch) / 24 : 1) // groups of 24 nonces; measured at 96 (profiles/equihash_r7.md)
#endif

namespace bcpk {

constexpr uint32_t OOB = 0x80000000u; // buffer offset past every descriptor's range: access dropped
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint32_t u3v __attribute__((ext_vector_type(3)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ wave / block scans
// DPP controls (GFX9 encoding): row_shr:n = 0x110|n, row_bcast:15 = 0x142, row_bcast:31 = 0x143,
// wave_shr:1 = 0x138. Lanes whose source is outside the row / disabled keep `old` (= 0, the
// identity of both + and max over unsigned values). All lanes of the wave must be active.
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ uint32_t dpp0(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWMASK, 0xf, false);
}
// Inclusive wave-wide sum (MAX = false) or max (MAX = true).
template <bool MAX> __device__ __forceinline__ uint32_t wave_incl(uint32_t x) {
    auto op = [](uint32_t a, uint32_t b) -> uint32_t { return MAX ? (a > b ? a : b) : a + b; };
    x = op(x, dpp0<0x111>(x));
    x = op(x, dpp0<0x112>(x));
    x = op(x, dpp0<0x114>(x));
    x = op(x, dpp0<0x118>(x));
    x = op(x, dpp0<0x142, 0xa>(x));
    x = op(x, dpp0<0x143, 0xc>(x));
    return x;
}

// Block-wide exclusive sum over n (<= MAXPER*NT) values: src[i] -> dst[i] (src may be dst);
// thread t owns `per` consecutive entries. Wave totals go through `wsum` (>= NT/64 entries);
// every wave combines them itself, so the scan costs two barriers (the second makes dst
// visible and frees wsum). Returns the total; `mine` (optional) receives the exclusive prefix of
// the thread's first entry.
template <int NT, int MAXPER = 4, class TS = uint32_t, class TD = TS>
__device__ uint32_t block_exscan(const TS* src, TD* dst, int n, uint32_t* wsum, uint32_t* mine = nullptr) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per = (n + NT - 1) / NT;
    uint32_t local[MAXPER];
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < MAXPER; ++q) {
        const int i = tid * per + q;
        local[q] = (q < per && i < n) ? (uint32_t)src[i] : 0u;
        s += local[q];
    }
    const uint32_t x = wave_incl<false>(s);
    if (NW > 1) {
        if (lane == 63) wsum[wid] = x;
        __syncthreads();
    }
    const uint32_t wt = (NW > 1 && lane < NW) ? wsum[lane] : 0u;
    const uint32_t ws = wave_incl<false>(wt);
    const uint32_t before = NW > 1 ? __builtin_amdgcn_readlane(ws, wid) - __builtin_amdgcn_readlane(wt, wid) : 0u;
    const uint32_t total = NW > 1 ? __builtin_amdgcn_readlane(ws, NW - 1) : __builtin_amdgcn_readlane(x, 63);
    uint32_t base = before + x - s;
    if (mine) *mine = base;
#pragma unroll
    for (int q = 0; q < MAXPER; ++q) {
        const int i = tid * per + q;
        if (q < per && i < n) dst[i] = (TD)base;
        base += local[q];
    }
    __syncthreads();
    return total;
}
template <int NT, int MAXPER = 4, class T = uint32_t>
__device__ uint32_t block_exscan(T* v, int n, uint32_t* wsum) {
    return block_exscan<NT, MAXPER, T, T>(v, v, n, wsum);
}

// Inclusive prefix maximum in place (entries u32 or u16); two barriers.
template <int NT, int MAXPER = 4, class T = uint32_t>
__device__ void block_maxscan(T* v, int n, uint32_t* wsum) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per = (n + NT - 1) / NT;
    uint32_t local[MAXPER];
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < MAXPER; ++q) {
        const int i = tid * per + q;
        local[q] = (q < per && i < n) ? (uint32_t)v[i] : 0u;
        s = max(s, local[q]);
    }
    const uint32_t x = wave_incl<true>(s);
    const uint32_t excl = dpp0<0x138>(x); // wave_shr:1 -> lane l sees lane l-1 (lane 0: 0)
    if (NW > 1) {
        if (lane == 63) wsum[wid] = x;
        __syncthreads();
    }
    const uint32_t wt = (NW > 1 && lane < NW) ? wsum[lane] : 0u;
    const uint32_t ws = wave_incl<true>(wt);
    const uint32_t before = (NW > 1 && wid > 0) ? __builtin_amdgcn_readlane(ws, wid - 1) : 0u;
    uint32_t run = max(before, excl);
#pragma unroll
    for (int q = 0; q < MAXPER; ++q) {
        const int i = tid * per + q;
        run = max(run, local[q]);
        if (q < per && i < n) v[i] = (T)run;
    }
    __syncthreads();
}

// Row I/O of W dwords at a dword-aligned byte offset through a buffer descriptor: one
// 16-byte access plus a remainder (dword-aligned 16-byte buffer accesses are legal on gfx950).
template <int W> __device__ __forceinline__ void row_store(__amdgpu_buffer_rsrc_t rs, uint32_t off, const uint32_t* v) {
    if constexpr (W >= 4) {
        const u4v x = {v[0], v[1], v[2], v[3]};
        __builtin_amdgcn_raw_buffer_store_b128(x, rs, off, 0, 0);
        row_store<W - 4>(rs, off + 16, v + 4);
    } else if constexpr (W == 3) {
        const u3v x = {v[0], v[1], v[2]};
        __builtin_amdgcn_raw_buffer_store_b96(x, rs, off, 0, 0);
    } else if constexpr (W == 2) {
        const u2v x = {v[0], v[1]};
        __builtin_amdgcn_raw_buffer_store_b64(x, rs, off, 0, 0);
    } else if constexpr (W == 1) {
        __builtin_amdgcn_raw_buffer_store_b32(v[0], rs, off, 0, 0);
    }
}

template <int W> __device__ __forceinline__ void row_load(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t* v) {
    if constexpr (W >= 4) {
        const u4v x = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        row_load<W - 4>(rs, off + 16, v + 4);
    } else if constexpr (W == 3) {
        const u3v x = __builtin_amdgcn_raw_buffer_load_b96(rs, off, 0, 0);
        v[0] = x.x, v[1] = x.y, v[2] = x.z;
    } else if constexpr (W == 2) {
        const u2v x = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
        v[0] = x.x, v[1] = x.y;
    } else if constexpr (W == 1) {
        v[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
    }
}

// x = LDS row i XOR LDS row j (rows of WI words): 8-byte LDS reads when rows are 8-byte aligned
// (even WI). Rows are random here, so every read is bank-conflict bound; a ds_read_b64 spreads its
// lanes over 64 banks where a ds_read2_b32 pays two 32-bank conflict rounds.
template <int WI> __device__ __forceinline__ void lds_row_xor(const uint32_t* rows, uint32_t i, uint32_t j, uint32_t* x) {
    if constexpr (WI % 2 == 0) {
        const u2v* r2 = reinterpret_cast<const u2v*>(rows);
#pragma unroll
        for (int w = 0; w < WI / 2; ++w) {
            const u2v a = r2[i * (WI / 2) + w], b = r2[j * (WI / 2) + w];
            x[2 * w] = a.x ^ b.x;
            x[2 * w + 1] = a.y ^ b.y;
        }
    } else {
#pragma unroll
        for (int w = 0; w < WI; ++w) x[w] = rows[i * WI + w] ^ rows[j * WI + w];
    }
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// XCD-aware work mapping. Workgroups are dispatched round-robin over the 8 XCDs (workgroup b
// on XCD b % 8), and each XCD has its own L2. A producer writes runs into every destination
// bucket of its nonce; a 128-byte line at a run boundary is shared by two producers. With all
// workgroups of a nonce on the same XCD those partial lines merge in one L2 before they are
// written back (non-temporal stores, which skip the L2 merge, measured 2x slower).
constexpr int NXCD = 8;
// it-th bucket of workgroup b among nbk = NB * nonces buckets (grid G); -1 when done.
template <int NB> __device__ __forceinline__ int xcd_bucket(int b, int it, int G, int nbk) {
    const int nonces = nbk / NB;
    if (G % NXCD || nonces % NXCD) { // (grids and batches that are no multiple of 8: plain striding)
        const int bk = b + it * G;
        return bk < nbk ? bk : -1;
    }
    const int x = b % NXCD, j = b / NXCD + it * (G / NXCD);
    if (j >= NB * (nonces / NXCD)) return -1;
    return (x + NXCD * (j / NB)) * NB + j % NB;
}

// ------------------------------------------------------------------ stage 0
// The tail of register generation (eh_gen_reg, eh_carry_gen): the row whose rank word is rk
// ((rank in this workgroup's run << 16) | bucket) goes to run position base_d + rank of its bucket
// in the stage-0 array (rs) and its leaf index li to LEAF (rl). A row that is not `live` or lies
// past the first round's capacity is stored at the out-of-range offset: the store stream is fixed.
template <class C>
__device__ __forceinline__ void eh_gen_store(__amdgpu_buffer_rsrc_t rs, __amdgpu_buffer_rsrc_t rl, uint32_t rk, uint32_t base_d,
                                             bool live, uint32_t li, const uint32_t* row) {
    constexpr int SW0 = C::sw(0);
    const uint32_t d = rk & 0xffff;
    const uint32_t pos = base_d + (rk >> 16);
    const uint32_t slot = d * C::AREA + pos;
    const bool ok = live && pos < (uint32_t)C::cap(1);
    row_store<C::words(0)>(rs, ok ? slot * (SW0 * 4) : OOB, row);
    __builtin_amdgcn_raw_buffer_store_b32(li, rl, ok ? slot * 4 : OOB, 0, 0);
}

// Generation workgroup gw of a nonce hashes rows [gw*RPW, (gw+1)*RPW), counting-sorts them by
// bucket in LDS, claims one run per destination bucket (device-scope atomicAdd on the stage-0
// fill counters CTR0[nonce][NB]) and writes every row into its run; the leaf index of each
// slot goes to LEAF.
template <class C, bool HDR>
__global__ __launch_bounds__(C::NTG) void eh_gen(const EhBaseState* __restrict__ states, uint32_t* __restrict__ R,
                                                 uint32_t* __restrict__ LEAF, uint32_t* __restrict__ CTR0) {
    constexpr int W0 = C::words(0);
    constexpr int SW = (C::N + 31) / 32 + 1;
    constexpr int NTG = C::NTG;
    constexpr uint32_t OCAP = C::cap(1);
    __shared__ uint32_t rows[C::RPW * W0];
    __shared__ uint16_t dst[C::RPW];
    __shared__ uint16_t perm[C::RPW];
    __shared__ uint32_t hist[C::NB], cur[C::NB], base[C::NB];
    __shared__ uint32_t wsum[NTG / 64 + 1];
    const int gw = blockIdx.x % C::GENWG;
    const int nonce = blockIdx.x / C::GENWG;
    const int tid = threadIdx.x;
    const EhBaseState& bs = states[nonce];
    for (int i = tid; i < C::NB; i += NTG) hist[i] = 0;
    __syncthreads();
    const uint32_t r0 = (uint32_t)gw * C::RPW, r1 = r0 + C::RPW;
    const uint32_t g0 = r0 / C::IPH, g1 = (r1 + C::IPH - 1) / C::IPH;
    for (uint32_t g = g0 + tid; g < g1; g += NTG) {
        uint64_t h[8];
        if constexpr (HDR) eh_hash_g_hdr(bs, g, h);
        else eh_hash_g(bs, g, h);
#pragma unroll
        for (int s = 0; s < C::IPH; ++s) {
            const uint32_t idx = g * C::IPH + s;
            if (idx < r0 || idx >= r1) continue;
            uint32_t S[SW];
#pragma unroll
            for (int w = 0; w < SW; ++w) {
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int k = 4 * w + t;
                    v = (v << 8) | ((k < C::NBYTES) ? digest_byte(h, s * C::NBYTES + k) : 0u);
                }
                S[w] = v;
            }
            const uint32_t li = idx - r0;
            const uint32_t d = S[0] >> (32 - C::BB);
#pragma unroll
            for (int w = 0; w < W0; ++w) rows[li * W0 + w] = (S[w] << C::BB) | (S[w + 1] >> (32 - C::BB));
            dst[li] = (uint16_t)d;
            atomicAdd(&hist[d], 1u);
        }
    }
    __syncthreads();
    // claim the runs; the returned bases are used only after the scan and the scatter
    uint32_t myb = 0, start = 0;
    if (tid < C::NB && hist[tid]) myb = atomicAdd(&CTR0[(size_t)nonce * C::NB + tid], hist[tid]);
    block_exscan<NTG>(hist, cur, C::NB, wsum, &start); // cur = run offsets inside this workgroup's sorted order
    for (int li = tid; li < C::RPW; li += NTG) perm[atomicAdd(&cur[dst[li]], 1u)] = (uint16_t)li;
    if (tid < C::NB) base[tid] = myb - start; // sorted position t of bucket d -> run position base[d] + t
    __syncthreads();
    constexpr int SW0 = C::sw(0);
    const auto rs = buf_rsrc(R + (size_t)nonce * C::ROWS * SW0, (uint32_t)(C::ROWS * SW0 * 4));
    uint32_t* leaf = LEAF + (size_t)nonce * C::ROWS;
    for (int t = tid; t < C::RPW; t += NTG) {
        const uint32_t li = perm[t], d = dst[li];
        const uint32_t pos = base[d] + (uint32_t)t;
        if (pos < OCAP) {
            uint32_t o[W0];
#pragma unroll
            for (int w = 0; w < W0; ++w) o[w] = rows[li * W0 + w];
            const uint32_t slot = d * C::AREA + pos;
            row_store<SW0>(rs, slot * (SW0 * 4), o);
            leaf[slot] = r0 + li;
        }
    }
}

// Register-resident generation for configs whose rows split evenly over hashes (IPH | RPW):
// every thread keeps the HPT*IPH rows it hashed in VGPRs, takes its rank inside this
// workgroup's run of each row's bucket with an LDS atomicAdd (returning), and after the
// run claims writes the rows straight from registers. LDS holds only the two NB-entry
// tables, so several workgroups share a CU and one's hashing (VALU) overlaps another's
// claim and scatter (memory) — the LDS-sorted eh_gen above holds a whole CU with its 118 KB
// row buffer and runs those phases back to back.
template <class C, bool HDR, int NTG, int HPT>
__global__ __launch_bounds__(NTG) __attribute__((amdgpu_waves_per_eu(1))) void eh_gen_reg(const EhBaseState* __restrict__ states, uint32_t* __restrict__ R,
                                                  uint32_t* __restrict__ LEAF, uint32_t* __restrict__ CTR0, int items) {
    using G = GenReg<C, NTG, HPT>;
    static_assert(G::OK, "register generation geometry");
    constexpr int W0 = C::words(0);
    constexpr int SW = (C::N + 31) / 32 + 1;
    __shared__ uint32_t hist[C::NB], base[C::NB];
    __shared__ uint64_t r0p[HDR ? 16 : 1]; // the nonce's g-independent round-0 prefix
    const int tid = threadIdx.x;
    // work item b = (nonce, gw); a persistent grid (gridDim.x < items, a multiple of 8) keeps every
    // item of a workgroup on that workgroup's XCD
    for (int b = blockIdx.x; b < items; b += gridDim.x) {
    int gw = b % G::GWG;
    int nonce = b / G::GWG;
    if ((items / G::GWG) % NXCD == 0 && gridDim.x % NXCD == 0) { // nonce n's workgroups on XCD n % 8
        const int x = b % NXCD, j = b / NXCD;
        gw = j % G::GWG;
        nonce = x + NXCD * (j / G::GWG);
    }
    if (b != (int)blockIdx.x) __syncthreads(); // the previous item's scatter has read base[]
    const EhBaseState& bs = states[nonce];
    for (int i = tid; i < C::NB; i += NTG) hist[i] = 0;
    if constexpr (HDR) {
        if (tid == 0) {
            uint64_t P[16];
            eh_hdr_round0_uniform(bs, P);
#pragma unroll
            for (int i = 0; i < 16; ++i) r0p[i] = P[i];
        }
    }
    __syncthreads();
    const uint32_t r0 = (uint32_t)gw * G::RPW;
    const uint32_t g0 = r0 / C::IPH;
    uint32_t rw[G::RPT][W0];
    uint32_t rk[G::RPT]; // (rank within this workgroup's run << 16) | bucket
#pragma unroll
    for (int hh = 0; hh < HPT; ++hh) {
        const uint32_t g = g0 + hh * NTG + tid;
        uint64_t h[8];
        if constexpr (HDR) {
            uint64_t P[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) P[i] = r0p[i];
            eh_hash_g_hdr_from(P, bs, g, h);
        } else {
            eh_hash_g(bs, g, h);
        }
#pragma unroll
        for (int s = 0; s < C::IPH; ++s) {
            uint32_t S[SW];
#pragma unroll
            for (int w = 0; w < SW; ++w) {
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int k = 4 * w + t;
                    v = (v << 8) | ((k < C::NBYTES) ? digest_byte(h, s * C::NBYTES + k) : 0u);
                }
                S[w] = v;
            }
            const int q = hh * C::IPH + s;
            const uint32_t d = S[0] >> (32 - C::BB);
#pragma unroll
            for (int w = 0; w < W0; ++w) rw[q][w] = (S[w] << C::BB) | (S[w + 1] >> (32 - C::BB));
            rk[q] = (atomicAdd(&hist[d], 1u) << 16) | d;
        }
    }
    __syncthreads();
    // claim one run per destination bucket
    for (int b = tid; b < C::NB; b += NTG) {
        const uint32_t c = hist[b];
        base[b] = c ? atomicAdd(&CTR0[(size_t)nonce * C::NB + b], c) : 0u;
    }
    __syncthreads();
    constexpr int SW0 = C::sw(0);
    const auto rs = buf_rsrc(R + (size_t)nonce * C::ROWS * SW0, (uint32_t)(C::ROWS * SW0 * 4));
    const auto rl = buf_rsrc(LEAF + (size_t)nonce * C::ROWS, (uint32_t)(C::ROWS * 4));
#pragma unroll
    for (int q = 0; q < G::RPT; ++q) {
        const uint32_t d = rk[q] & 0xffff;
        const uint32_t g = g0 + (q / C::IPH) * NTG + tid;
        const uint32_t li = g * C::IPH + (q % C::IPH); // leaf index
        eh_gen_store<C>(rs, rl, rk[q], base[d], true, li, rw[q]);
    }
    }
}

// ------------------------------------------------------------------ stages 1..K
// Diagnostic builds (STAMP) record s_memtime at each phase boundary (thread 0, after the
// barrier) into `stamps` — never used by the production instantiation.
#define EH_STAMP(k)                                                                                  \
    do {                                                                                             \
        if constexpr (STAMP) {                                                                       \
            if (threadIdx.x == 0) stamps[(size_t)bk * 16 + (k)] = __builtin_amdgcn_s_memtime();        \
        }                                                                                            \
    } while (0)

// What a carrying round needs of the next group (all pointers already at that group's first nonce).
struct EhCarry {
    const EhBaseState* states;
    uint32_t* R0;
    uint32_t* LEAF;
    uint32_t* CTR0;
    int nonces; // partner nonces that exist (the last group may be smaller)
};

// Workgroup barrier k of a carrying round's bucket iteration. The round waves and the generation
// waves run different code between the SAME number of barriers: each path executes eh_bar<1, NBAR> ..
// eh_bar<NBAR, NBAR> exactly once per bucket, in order, and one prologue barrier before the loop.
// NBAR = eh_bars(slot round).n (equihash_layout.h) on either path: 10 in a sorted round, 7 in a
// slot round. No barrier depends on data. The two barriers inside block_exscan are written out at
// its call sites as EH_BAR_SCAN(k, NBAR) (a check only; block_exscan executes them).
constexpr int EH_SCAN_BARS = 2; // block_exscan with more than one wave
template <int K, int NBAR> __device__ __forceinline__ void eh_bar() {
    static_assert(K >= 1 && K <= NBAR, "barrier outside the bucket iteration's count");
    __syncthreads();
}
#define EH_BAR_SCAN(k, nbar) static_assert((k) >= 1 && (k) + EH_SCAN_BARS - 1 <= (nbar), "scan barriers")

// The generation waves of a carrying round (threads C::RNT.. of the workgroup). They walk the
// same buckets as the round waves (the same xcd_bucket sequence, so the same trip count) and in
// bucket (nonce n, d) generate chunk (STAGE-1)*NB + d of the next group's nonce n: what eh_gen_reg
// does for a workgroup's rows, cut into slices between the round's barriers. The slices follow
// the length of the round waves' intervals (profiles/equihash_r6.md, per-bucket cycles), so that
// the generation waves are not the last to reach a barrier (barrier numbers of a sorted round) —
//   before barrier 1 (commit), 4 (key placement), 5 (pair listing), 6 (pair filter): BLAKE2b
//   rounds; nothing inside the round's two block scans (barriers 2, 3 and 7, 8 are a few hundred
//   cycles apart); before 5 also one lane's round-0 prefix when the next bucket is another nonce's;
//   before 6 also digest -> rows and the LDS histogram (each row's rank in this chunk's run of
//   its bucket);
//   before 7: one atomicAdd per non-empty destination claims the run on CTR0 (the returns are
//   read two barriers later, so their latency is not waited for at a barrier);
//   before 8: the histogram is cleared for the next chunk;
//   before 9: run bases to LDS;
//   before 10 (emit, the round's longest interval): the rows and their leaf indices go to the
//   claimed runs, then the NEXT bucket's hashes start (the state words stay in registers).
// A slot round (EhCfg::ks) has no key scan and no key placement: its barriers 2..7 are the sorted
// round's 5..10, the slices keep their intervals, and the BLAKE2b round of the key-placement
// interval runs in the pair-listing interval (BCP_EH_SLOT_RB .. BCP_EH_SLOT_RD).
// A bucket whose partner nonce does not exist or whose chunk lies past the nonce's last hash
// only keeps the barriers.
template <class C, int STAGE>
__device__ __forceinline__ void eh_carry_gen(const EhCarry& cy, int nbk, uint32_t* ghist, uint32_t* gbase, uint64_t* gr0p) {
    using GC = GenCarry<C>;
    constexpr int W0 = C::words(0);
    constexpr int SW = (C::N + 31) / 32 + 1;
    constexpr int SW0 = C::sw(0);
    constexpr int GT = GC::GT, HB = GC::HB;
    const int gtid = (int)threadIdx.x - C::RNT;
    const int grid = gridDim.x;
    // chunk of bucket b, or -1 when there is nothing to generate (uniform)
    auto chunk_of = [&](int b) -> int {
        const int nonce = b / C::NB, c = (STAGE - 1) * C::NB + b % C::NB;
        return (nonce < cy.nonces && (long long)c * GC::CH < GC::NHASH) ? c : -1;
    };
    auto prefix = [&](int b) { // the round-0 prefix of bucket b's partner nonce
        if (gtid == 0 && b / C::NB < cy.nonces) {
            uint64_t P[16];
            eh_hdr_round0_uniform(cy.states[b / C::NB], P);
#pragma unroll
            for (int i = 0; i < 16; ++i) gr0p[i] = P[i];
        }
    };
    // BLAKE2b round at which each slice stops (round 0 belongs to begin())
    // in the round's emit / commit / key placement / pair listing interval; the pair filter
    // interval takes the rest (the schedules measured are in profiles/equihash_r7.md)
    using G = EhRoundGeom<C, STAGE, true>; // the round these waves are part of
    constexpr bool SLOT = G::SLOT;
    constexpr EhBars BAR = G::BAR;
    constexpr int NBAR = G::NBAR;
    constexpr int RA = 3, RB = SLOT ? BCP_EH_SLOT_RB : 5, RC = SLOT ? RB : 6, RD = SLOT ? BCP_EH_SLOT_RD : 10;
    static_assert(RA <= RB && RB <= RC && RC <= RD && RD <= 12, "BLAKE2b slices in order");
    EhHdrHash hs[HB];
    // start the hashes of bucket b's chunk: begin() and rounds 1..RA-1
    auto start = [&](int b) {
        const int c = chunk_of(b);
        if (c < 0) return;
        const EhBaseState& bs = cy.states[b / C::NB];
        uint64_t P[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) P[i] = gr0p[i];
#pragma unroll
        for (int hh = 0; hh < HB; ++hh) {
            hs[hh].begin(P, bs, (uint32_t)c * GC::CH + (uint32_t)(hh * GT + gtid));
            hs[hh].template rounds<1, RA>(bs);
        }
    };
    int it = 0;
    int bk = xcd_bucket<C::NB>(blockIdx.x, 0, grid, nbk); // >= 0: the caller returned otherwise
    for (int i = gtid; i < C::NB; i += GT) ghist[i] = 0;
    prefix(bk);
    __syncthreads(); // the prologue barrier
    start(bk);
    for (;;) {
        const int nonce = bk / C::NB;
        const int chunk = chunk_of(bk);
        const bool act = chunk >= 0; // uniform
        const EhBaseState& bs = cy.states[act ? nonce : 0];
        const int bn = xcd_bucket<C::NB>(blockIdx.x, it + 1, grid, nbk);
        const bool more = bn >= 0; // uniform, the round waves' loop-exit test
        const uint32_t g0 = (uint32_t)chunk * GC::CH + (uint32_t)gtid;
        uint32_t rw[GC::RPT][W0];
        uint32_t rk[GC::RPT]; // (rank within this chunk's run << 16) | bucket; NIL: no such row
        uint32_t myb[GC::BPT];
        if (act) {
#pragma unroll
            for (int hh = 0; hh < HB; ++hh) hs[hh].template rounds<RA, RB>(bs);
        }
        eh_bar<1, NBAR>();
        if constexpr (!SLOT) {
            eh_bar<2, NBAR>(); // (the round waves are inside their key scan: two short intervals)
            eh_bar<3, NBAR>();
            if (act) {
#pragma unroll
                for (int hh = 0; hh < HB; ++hh) hs[hh].template rounds<RB, RC>(bs);
            }
            eh_bar<4, NBAR>();
        }
        if (act) {
#pragma unroll
            for (int hh = 0; hh < HB; ++hh) hs[hh].template rounds<RC, RD>(bs);
        }
        // the next bucket's prefix, when its nonce is another one: gr0p is read only in start()
        // (before the last barrier of the previous bucket; next after the pair-sort barrier of this one)
        if (more && bn / C::NB != nonce) prefix(bn);
        eh_bar<BAR.list, NBAR>();
        if (act) {
#pragma unroll
            for (int hh = 0; hh < HB; ++hh) {
                hs[hh].template rounds<RD, 12>(bs);
                uint64_t h[8];
                hs[hh].finish(bs, h);
                const uint32_t g = g0 + hh * GT;
#pragma unroll
                for (int s = 0; s < C::IPH; ++s) {
                    uint32_t S[SW];
#pragma unroll
                    for (int w = 0; w < SW; ++w) {
                        uint32_t v = 0;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int k = 4 * w + t;
                            v = (v << 8) | ((k < C::NBYTES) ? digest_byte(h, s * C::NBYTES + k) : 0u);
                        }
                        S[w] = v;
                    }
                    const int q = hh * C::IPH + s;
                    const uint32_t d = S[0] >> (32 - C::BB);
#pragma unroll
                    for (int w = 0; w < W0; ++w) rw[q][w] = (S[w] << C::BB) | (S[w + 1] >> (32 - C::BB));
                    rk[q] = NIL;
                    if (g * C::IPH + s < (uint32_t)C::INIT) rk[q] = (atomicAdd(&ghist[d], 1u) << 16) | d;
                }
            }
        }
        eh_bar<BAR.filter, NBAR>();
        if (act) {
#pragma unroll
            for (int k = 0; k < GC::BPT; ++k) {
                const int b = gtid + k * GT;
                const uint32_t c = b < C::NB ? ghist[b] : 0u;
                myb[k] = 0;
                if (c) myb[k] = atomicAdd(&cy.CTR0[(size_t)nonce * C::NB + b], c);
            }
        }
        eh_bar<BAR.scan, NBAR>();
        if (act)
            for (int i = gtid; i < C::NB; i += GT) ghist[i] = 0;
        eh_bar<BAR.scan + 1, NBAR>();
        if (act) {
#pragma unroll
            for (int k = 0; k < GC::BPT; ++k) {
                const int b = gtid + k * GT;
                if (b < C::NB) gbase[b] = myb[k];
            }
        }
        eh_bar<BAR.sort, NBAR>();
        if (act) {
            const auto rs = buf_rsrc(cy.R0 + (size_t)nonce * C::ROWS * SW0, (uint32_t)(C::ROWS * SW0 * 4));
            const auto rl = buf_rsrc(cy.LEAF + (size_t)nonce * C::ROWS, (uint32_t)(C::ROWS * 4));
#pragma unroll
            for (int q = 0; q < GC::RPT; ++q) {
                const uint32_t d = rk[q] & 0xffff;
                const uint32_t li = (g0 + (q / C::IPH) * GT) * C::IPH + (q % C::IPH); // leaf index
                eh_gen_store<C>(rs, rl, rk[q], gbase[d < (uint32_t)C::NB ? d : 0], rk[q] != NIL, li, rw[q]);
            }
        }
        if (more) start(bn); // the round waves' emit is their longest interval
        eh_bar<NBAR, NBAR>();
        if (!more) break;
        bk = bn;
        ++it;
    }
}

// STAGE < K: collision round producing stage-STAGE rows. STAGE == K: final round.
// Bucket bk = nonce*NB + d holds the stage STAGE-1 rows whose top digit bits are d (area d of
// that stage, CTRin[bk] rows).
//
// The kernel is PERSISTENT and software-pipelined: one workgroup per CU walks buckets
// blockIdx.x, +gridDim.x, ... While it collides bucket b out of LDS, the rows of its next
// bucket are in flight into VGPRs (lane-flat row loads of the contiguous area, issued in slices
// across the phases; plain loads are not drained by a bare barrier). Per bucket:
//   A. commit: prefetched rows (VGPRs) -> LDS rows (+ parent words when pruning), counting each
//      row's RB-bit key with a returning LDS atomic (its rank in the key group);
//      issue the first slice of the next bucket's loads;
//      a slot round also files the row's id in slot `rank` of its key (ranks >= 8: overflow list);
//   D1. sorted round only. Key scan: every committed row learns its sorted position;
//   D2. pair list by per-wave compaction (one barrier; a sorted round walks the key group in
//       sorted order, a slot round reads the key's slots), then the pair filter (identical
//       subtrees; depth-1 pruning where the round prunes) and the destination histogram;
//   D3. one atomicAdd per destination bucket claims this bucket's runs there; counting sort of
//       the pairs by destination;
//   D4. one-lane-per-row emit (XOR, shift one digit, 16-byte stores) into the claimed runs,
//       plus the parent word(s), or (table parents) the bucket in the row's padding and the pair
//       word into the bucket's pair table.
// The final round (STAGE == K) sorts its one-word rows by key and lists the candidates: pairs
// equal on all remaining bits.
// Input rows whose slots carry compact parents keep the parent-bucket bits in their padding in
// LDS (the prune check reads them); every comparison and the emit XOR mask them out (RMI).
// pdrop holds 2K + 2 counters per nonce. pdrop[STAGE]: pairs lost to a full pair list or to the 14-partner cap of a row in a large key
// group (duplicate subtrees); pdrop[K + STAGE]: stage-(STAGE-1) rows past the
// round's capacity (offered to a bucket but never read), counted for every nonce. Slot rounds
// also count the rows sent to the overflow list and the most of them in one bucket (EhCfg::PDW).
// Workgroup barriers per bucket: 10 in a sorted round, 7 in a slot round (eh_bars).
//
// CARRY (collision rounds of a configuration with GW > 0): the last GW waves of the workgroup are
// generation waves. The first C::RNT threads run the round exactly as described above (every
// per-workgroup size below is taken from that thread count); the generation waves run
// eh_carry_gen between the same workgroup barriers.
//
// The phases that come out of the kernel without costing registers are the function templates
// below: the prefetch issue (identical code), the key sort, the final round's candidate search and
// the sorted round's listing (sorted and final rounds change slightly, within the register bounds;
// the slot rounds stay byte-identical). G is the round's EhRoundGeom (equihash_layout.h). The
// commit, the slot listing, the pair filter, the run claim, the pair sort and the emit stay inline
// in eh_round: each of them as a function cost SGPR spills or more than two VGPRs in some round
// (profiles/equihash_r11.md has the per-phase table), and so does sharing eh_shares_parent or
// opaque_tid with the lambdas of the same name in eh_round.

// (keep in step with the lambda of the same name in eh_round, which the inline phases use)
// A thread id the compiler cannot see through: keeps the per-lane index math of the
// prefetch/commit loops from being hoisted out of the persistent loop (live invariants
// would otherwise push the prefetched rows out to scratch).
__device__ __forceinline__ uint32_t opaque_tid() {
    const int tid = threadIdx.x;
    uint32_t t;
    asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(tid));
    return t;
}

// rows i and j share a parent (depth-1 duplicate): equal producing bucket and a common LDS row
// (keep in step with the shares_parent lambda in eh_round, which the inline pair filter uses)
template <class G>
__device__ __forceinline__ bool eh_shares_parent(const typename G::Rows& rows, const typename G::Psig& psig, const typename G::Pdw& pdw, uint32_t i,
                                                 uint32_t j) {
    using C = typename G::Cfg;
    constexpr int WI = G::WI;
    const uint32_t a = psig[i], b = psig[j];
    const uint32_t ai = a & C::IMASK, bi = b & C::IMASK;
    const bool hit = (ai & 0xffff) == (bi & 0xffff) || (ai & 0xffff) == (bi >> 16) ||
                     (ai >> 16) == (bi & 0xffff) || (ai >> 16) == (bi >> 16);
    if (!hit) return false;
    if constexpr (G::CPI)
        return ((a ^ b) & ~C::IMASK) == 0 && ((rows[i * WI + WI - 1] ^ rows[j * WI + WI - 1]) & G::RMI) == 0;
    else
        return pdw[i] == pdw[j];
}

// Prefetch issue: the loads of rows [u0, u1) per lane of bucket pf_bk (pf_n rows) into nr. Reads
// Rin; no barrier on either side (the loads stay in flight across barriers until the commit).
// Every vector-memory instruction of the loop body is issued unconditionally (lanes with nothing
// to move use an out-of-range buffer offset, which the descriptor's range check drops), so the
// compiler can count the outstanding operations and wait for the prefetched words with a precise
// vmcnt(N) instead of vmcnt(0): a vmcnt(0) at the commit would wait for the acks of the previous
// bucket's emit stores as well.
template <class G>
__device__ __forceinline__ void eh_prefetch(const uint32_t* Rin, int pf_bk, uint32_t pf_n, int u0, int u1,
                                            uint32_t (&nr)[G::RPL][G::LWI]) {
    using C = typename G::Cfg;
    const int nonce = pf_bk / C::NB, d = pf_bk % C::NB;
    const auto rs = buf_rsrc(Rin + ((size_t)nonce * C::ROWS + (size_t)d * C::AREA) * G::SWI, G::CAP * G::SWI * 4);
    const uint32_t ot = opaque_tid();
#pragma unroll
    for (int u = 0; u < G::RPL; ++u) {
        if (u < u0 || u >= u1) continue;
        const uint32_t r = ot + u * G::NT;
        row_load<G::LWI>(rs, r < pf_n ? r * (G::SWI * 4) : OOB, nr[u]);
    }
}

// D1. key sort of a sorted round, between barriers 1 and 4 (the scan runs barriers 2 and 3).
// Collision round: the commit counted the keys; scan bend to group starts and place each row by
// its rank: sidx = row ids grouped by key, krank = the row's sorted position, kpairs = the number of
// later positions in its key group (its pairs, capped at 14; the excess counts as pair drops).
// Final round: count, scan, then place (sidx as above, bend[key] = end of the key's group).
template <class G>
__device__ __forceinline__ void eh_key_sort(const typename G::Rows& rows, uint32_t* bend, uint16_t* sidx, typename G::Wsum& wsum,
                                            uint32_t* pdrop, int nonce, uint32_t n, uint32_t (&krank)[G::FINAL ? 1 : G::RPL],
                                            uint32_t (&kpairs)[G::FINAL ? 1 : G::RPL]) {
    using C = typename G::Cfg;
    constexpr int NT = G::NT;
    const int tid = threadIdx.x;
    if constexpr (!G::FINAL) {
        EH_BAR_SCAN(2, G::NBAR); // barriers 2, 3
        block_exscan<NT, (C::NRESTS + NT - 1) / NT>(bend, C::NRESTS, wsum);
        const uint32_t ot = opaque_tid();
#pragma unroll
        for (int u = 0; u < G::RPL; ++u) {
            const uint32_t r = ot + u * NT;
            kpairs[u] = 0;
            if (r < n) {
                const uint32_t key = krank[u] >> 16;
                const uint32_t pos = bend[key] + (krank[u] & 0xffff);
                const uint32_t e = key + 1 < (uint32_t)C::NRESTS ? bend[key + 1] : n;
                sidx[pos] = (uint16_t)r;
                krank[u] = pos;
                kpairs[u] = min(e - pos - 1, 14u);
                if (e - pos - 1 > 14u) atomicAdd(&pdrop[nonce * C::PDW + G::STAGE], e - pos - 1 - 14u); // capped pairs (rare) count as pair-list drops
            }
        }
    } else {
        auto key_of = [&](uint32_t i) -> uint32_t { return rows[i * G::WI] >> (32 - C::RB); };
        for (uint32_t i = tid; i < n; i += NT) atomicAdd(&bend[key_of(i)], 1u);
        __syncthreads();
        block_exscan<NT, (C::NRESTS + NT - 1) / NT>(bend, C::NRESTS, wsum);
        for (uint32_t i = tid; i < n; i += NT) sidx[atomicAdd(&bend[key_of(i)], 1u)] = (uint16_t)i;
    }
}

// D2, final round: the candidate search, after barrier 4, before the last barrier. Reads rows,
// sidx, bend (psig, pdw); writes ncand and cand. Candidates are pairs equal on ALL remaining bits:
// each sorted position scans the rest of its key group (a few rows). No pair list, so a bucket's
// pair count is not capped (a capped list here silently lost solutions).
template <class G>
__device__ __forceinline__ void eh_final_candidates(const typename G::Rows& rows, const typename G::Psig& psig, const typename G::Pdw& pdw,
                                                    const uint16_t* sidx, const uint32_t* bend, uint32_t* ncand, uint64_t* cand,
                                                    int nonce, int d, uint32_t n) {
    using C = typename G::Cfg;
    static_assert(G::WI == 1, "final-round rows are one word");
    const int tid = threadIdx.x;
    for (uint32_t p = tid; p < n; p += G::NT) {
        const uint32_t i = sidx[p], ri = rows[i], e = bend[ri >> (32 - C::RB)];
        for (uint32_t q = p + 1; q < e; ++q) {
            const uint32_t j = sidx[q];
            if ((rows[j] ^ ri) & ~G::RMI) continue;
            if constexpr (G::PRUNE) {
                if (eh_shares_parent<G>(rows, psig, pdw, i, j)) continue;
            }
            const uint32_t c = atomicAdd(&ncand[nonce], 1u);
            if (c < (uint32_t)C::MAXCAND) cand[(size_t)nonce * C::MAXCAND + c] = pack_tri(d, i, j);
        }
    }
}

// D2. pair list by per-wave compaction, before barrier BAR.list (after barrier 4 in a sorted round,
// 1 in a slot round). Each lane has counted the pairs of the rows it committed (kpairs, registers;
// cnt: the lane's other pairs), a DPP wave scan gives the lane's offset inside its wave, ONE LDS
// atomic per wave claims the wave's block of the list (npairs): returns the lane's first entry.
// The list holds MP*NT pairs (above the row capacity: capped pair lists lost ~9% of the
// solutions); identical subtrees and pairs that share a parent are dropped when the pairs are read
// back (eh_filter).
template <class G>
__device__ __forceinline__ uint32_t eh_list_claim(uint32_t cnt, const uint32_t (&kpairs)[G::RPL], uint32_t& npairs) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < G::RPL; ++u) cnt += kpairs[u];
    const uint32_t incl = wave_incl<false>(cnt);
    uint32_t wb = 0;
    if ((tid & 63) == 63) wb = atomicAdd(&npairs, incl);
    return __builtin_amdgcn_readlane(wb, 63) + incl - cnt;
}

// D2, sorted round. Reads sidx, krank and kpairs; writes plist and npairs. Sorted position p pairs
// with every later position of its key group: c_p = bend[key] - p - 1 pairs (capped at 14; a group
// of 16+ rows is ~1e-8 likely), the lane writes its (j << 16 | i) pairs into its part of the list.
template <class G>
__device__ __forceinline__ void eh_list_sorted(const uint16_t* sidx, uint32_t* plist, uint32_t& npairs,
                                               const uint32_t (&krank)[G::RPL], const uint32_t (&kpairs)[G::RPL]) {
    const int tid = threadIdx.x;
    uint32_t o = eh_list_claim<G>(0, kpairs, npairs);
#pragma unroll
    for (int u = 0; u < G::RPL; ++u) {
        if (!kpairs[u]) continue;
        const uint32_t p = krank[u];
        const uint32_t i = tid + u * G::NT;
        for (uint32_t q = p + 1; q <= p + kpairs[u]; ++q, ++o) {
            if (o >= (uint32_t)G::NPAIR) continue;
            plist[o] = ((uint32_t)sidx[q] << 16) | i;
        }
    }
}

// The kernel. EhRoundGeom gives the geometry; the local names below are the ones the inline phases use.
template <class C, int STAGE, bool STAMP, bool CARRY = false>
__global__ __launch_bounds__(C::NT) __attribute__((amdgpu_waves_per_eu(C::WGCU * C::NT / 256)))
void eh_round(const uint32_t* __restrict__ Rin, const uint32_t* __restrict__ CTRin, uint32_t* __restrict__ Rout,
              uint32_t* __restrict__ CTRout, uint32_t* __restrict__ Pout, uint32_t* __restrict__ Bout,
              uint32_t* __restrict__ ncand, uint64_t* __restrict__ cand, uint64_t* __restrict__ stamps,
              uint32_t* __restrict__ pdrop, int nbk, EhCarry carry) {
    using G = EhRoundGeom<C, STAGE, CARRY>;
    static_assert(!CARRY || !STAMP, "only plain collision rounds carry generation");
    constexpr bool FINAL = G::FINAL, PRUNE = G::PRUNE, SLOT = G::SLOT, TPO = G::TPO, CPI = G::CPI;
    constexpr int WI = G::WI, WO = G::WO, CAP = G::CAP, NT = G::NT, RPL = G::RPL, MP = G::MP, SWI = G::SWI, SWO = G::SWO;
    constexpr int PTW = G::PTW, SLI = G::SLI, BPT = G::BPT, LWI = G::LWI, OVL = G::OVL, PDW = C::PDW;
    constexpr uint32_t RMI = G::RMI, RMO = G::RMO, OCAP = G::OCAP;
    constexpr EhBars BAR = G::BAR;
    constexpr int NBAR = G::NBAR; // workgroup barriers per bucket (eh_carry_gen: the same constant)
    // key counting folded into the commit (collision rounds): bend holds counts after the commit
    // and group starts after the scan; spair then aliases the pair list, so bend survives the
    // emit and is cleared for the next bucket in D3
    constexpr bool FOLD = !FINAL;
    using HT = typename G::HT;
    __shared__ __attribute__((aligned(16))) typename G::Rows rows;
    __shared__ typename G::Psig psig;                          // the input rows' parent word (j << 16 | i, + d bits)
    __shared__ typename G::Pdw pdw;                            // two-word parents: the producing bucket
    __shared__ uint32_t npairs;                                // wave-compaction pair list fill
    __shared__ uint32_t novf;                                  // slot round: overflow list fill (rows offered to it); else unused
    __shared__ __attribute__((aligned(16))) uint8_t un[G::UN_BYTES];
    __shared__ typename G::Hist hist_, cur_;                   // H16: two 16-bit counters per word
    __shared__ typename G::Base base;
    __shared__ typename G::Wsum wsum;
    __shared__ uint32_t ghist[CARRY ? C::NB : 1], gbase[CARRY ? C::NB : 1]; // the generation waves' tables
    __shared__ uint64_t gr0p[CARRY ? 16 : 1];
    uint16_t* sidx = reinterpret_cast<uint16_t*>(un); // slot round: ktab[key][rank], the row ids of each key
    uint16_t* ktab = sidx;
    uint32_t* bend = reinterpret_cast<uint32_t*>(un + G::UN_BEND);
    uint32_t* ovl = reinterpret_cast<uint32_t*>(un + G::UN_OVL); // slot round only
    uint32_t* plist = reinterpret_cast<uint32_t*>(un + G::UN_PLIST);
    uint32_t* spair = FOLD ? plist : reinterpret_cast<uint32_t*>(un);
    const int tid = threadIdx.x;
    const int grid = gridDim.x;
    int it = 0;
    int bk = xcd_bucket<C::NB>(blockIdx.x, 0, grid, nbk);
    if (bk < 0) return; // uniform per workgroup
    if constexpr (CARRY) {
        // the role is wave-uniform: a scalar branch
        if (__builtin_amdgcn_readfirstlane(tid >> 6) >= NT / 64) {
            eh_carry_gen<C, STAGE>(carry, nbk, ghist, gbase, gr0p);
            return;
        }
    }

    // histogram entry b (count or running position) and its returning increment
    auto hget = [&](const uint32_t* h, int b) -> uint32_t {
        if constexpr (C::H16) return reinterpret_cast<const uint16_t*>(h)[b];
        else return h[b];
    };
    auto hinc = [&](uint32_t* h, uint32_t b) -> uint32_t {
        if constexpr (C::H16) {
            const uint32_t sh = (b & 1) * 16;
            return (atomicAdd(&h[b >> 1], 1u << sh) >> sh) & 0xffffu;
        } else {
            return atomicAdd(&h[b], 1u);
        }
    };
    // rows i and j share a parent (depth-1 duplicate): equal producing bucket and a common LDS row
    // (keep in step with eh_shares_parent above, which eh_final_candidates uses)
    auto shares_parent = [&](uint32_t i, uint32_t j) -> bool {
        const uint32_t a = psig[i], b = psig[j];
        const uint32_t ai = a & C::IMASK, bi = b & C::IMASK;
        const bool hit = (ai & 0xffff) == (bi & 0xffff) || (ai & 0xffff) == (bi >> 16) ||
                         (ai >> 16) == (bi & 0xffff) || (ai >> 16) == (bi >> 16);
        if (!hit) return false;
        if constexpr (CPI)
            return ((a ^ b) & ~C::IMASK) == 0 && ((rows[i * WI + WI - 1] ^ rows[j * WI + WI - 1]) & RMI) == 0;
        else
            return pdw[i] == pdw[j];
    };

    // a collision pair (LDS rows i, j) is kept unless the rows are identical or share a parent;
    // dest = its destination bucket
    auto pair_keep = [&](uint32_t i, uint32_t j, uint32_t& dest) -> bool {
        uint32_t x0 = rows[i * WI] ^ rows[j * WI];
        if constexpr (WI == 1) x0 &= ~RMI;
        // identical subtrees are dropped; word 0 differs in all but ~2^-21 of the pairs, so the
        // remaining words are read only when it matches. The branch is wave-uniform (every active
        // lane reads them when one lane's word 0 matches) and `keep` is assigned once. Written as
        // a per-lane `if (!keep) keep |= ...`, hipcc (ROCm 7.2.0, gfx950, this file's flags) compiled
        // the first unrolled filter instance of (200,9) rounds 3, 4, 6, 7, 8 so that every lane
        // on this path left pv = NIL while the kept ones still counted in hist_: about one pair per
        // nonce and round (destination bucket 0) was claimed but never emitted, its slot kept an
        // earlier batch's row, and a stale pair-table entry was emitted into another bucket.
        // 3 of 108,017 solutions were invalid that way; 0 of 270,706 with this form.
        bool keep = x0 != 0;
        if (__builtin_amdgcn_ballot_w64(!keep) != 0) {
            uint32_t acc = x0;
#pragma unroll
            for (int w = 1; w < WI; ++w) {
                uint32_t y = rows[i * WI + w] ^ rows[j * WI + w];
                if (w == WI - 1) y &= ~RMI;
                acc |= y;
            }
            keep = acc != 0;
        }
        if constexpr (PRUNE) {
            if (keep && shares_parent(i, j)) keep = false;
        }
        dest = (x0 >> (32 - C::DB)) & (C::NB - 1);
        return keep;
    };

    // (keep in step with the free opaque_tid() above, which the phase functions use)
    // A thread id the compiler cannot see through: keeps the per-lane index math of the
    // prefetch/commit loops from being hoisted out of the persistent loop (live invariants
    // would otherwise push the prefetched rows out to scratch).
    auto opaque_tid = [&]() -> uint32_t {
        uint32_t t;
        asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(tid));
        return t;
    };
    // (a round that does not prune loads only the row words of each slot)
    uint32_t nr[RPL][LWI];
    uint32_t krank[FOLD ? RPL : 1]; // FOLD: (key << 16) | rank in the key group of each committed row
    int pf_bk = bk;
    uint32_t pf_n = 0;
    // Issue prefetch rows [u0, u1) of bucket pf_bk. Every vector-memory instruction of the loop
    // body is issued unconditionally (lanes with nothing to move use an out-of-range buffer offset,
    // which the descriptor's range check drops), so the compiler can count the outstanding
    // operations and wait for the prefetched words with a precise vmcnt(N) instead of vmcnt(0): a
    // vmcnt(0) at the commit would wait for the acks of the previous bucket's emit stores as well.
    auto issue = [&](int u0, int u1) { eh_prefetch<G>(Rin, pf_bk, pf_n, u0, u1, nr); };

    // prologue: first bucket in flight, fill of the second known
    uint32_t fill = CTRin[bk]; // rows offered to the current bucket (more than CAP: the rest were dropped)
    uint32_t n = min(fill, (uint32_t)CAP);
    pf_n = n;
    issue(0, RPL);
    if constexpr (!FINAL) {
        // As many (dropped) stores as one emit issues: the compiler's wait counts at the loop head
        // take the minimum over the entry and back edges; with these, both edges see the prefetch
        // loads followed by MP emit store groups, so the commit waits for its loads only.
        const auto rs_out = buf_rsrc(Rout, 0);
        const uint32_t z[SWO] = {};
        if constexpr (TPO) { // D3's run-base stores come between the last prefetch slice and the emit
#pragma unroll
            for (int k = 0; k < BPT; ++k) __builtin_amdgcn_raw_buffer_store_b32(0u, rs_out, OOB + 256 * MP + 64 * k, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < MP; ++u) {
            row_store<SWO>(rs_out, OOB + 256 * u, z); // distinct offsets: identical stores would be merged
            if constexpr (TPO) __builtin_amdgcn_raw_buffer_store_b32(0u, rs_out, OOB + 256 * u + 128, 0, 0); // the unit's pair-table store
        }
    }
    if constexpr (FOLD) {
        for (int k = tid; k < C::NRESTS; k += NT) bend[k] = 0;
        if constexpr (SLOT) {
            if (tid == 0) novf = 0;
        }
        __syncthreads();
    }
    // slot round: overflow rows of this workgroup's buckets of the current nonce and the most in one
    // bucket (uniform), written to the nonce's counters when the nonce changes
    uint32_t ovf_sum = 0, ovf_max = 0;
    const int bk1 =xcd_bucket<C::NB>(blockIdx.x, 1, grid, nbk);
    uint32_t fill_next = bk1 >= 0 ? CTRin[bk1] : 0u;
    // Fill of bucket b (0 for b < 0). As a buffer load it is counted by vmcnt, which barriers do not
    // drain; a plain load of this uniform address would be a scalar load, counted with the LDS
    // operations in lgkmcnt, and the lgkmcnt(0) before the next barrier would wait for its
    // global-memory round trip. It is read (readfirstlane) one bucket later, after the commit has
    // waited for the prefetched rows that were issued around it.
    const auto ctr_rs = buf_rsrc(CTRin, (uint32_t)nbk * 4);
    auto fill_of = [&](int b) -> uint32_t {
        return __builtin_amdgcn_raw_buffer_load_b32(ctr_rs, b >= 0 ? (uint32_t)b * 4 : OOB, 0, 0);
    };

    for (;;) {
        const int nonce = bk / C::NB, d = bk % C::NB;
        EH_STAMP(0);
        if (tid == 0 && fill > (uint32_t)CAP) atomicAdd(&pdrop[nonce * PDW + C::K + STAGE], fill - CAP); // rare
        // A. commit the prefetched bucket (one row per lane per unit)
        {
            const uint32_t ot = opaque_tid();
#pragma unroll
            for (int u = 0; u < RPL; ++u) {
                const uint32_t r = ot + u * NT;
                if (r < n) {
                    if constexpr (WI % 2 == 0) {
#pragma unroll
                        for (int w = 0; w < WI; w += 2)
                            *reinterpret_cast<u2v*>(&rows[r * WI + w]) = u2v{nr[u][w], nr[u][w + 1]};
                    } else {
#pragma unroll
                        for (int w = 0; w < WI; ++w) rows[r * WI + w] = nr[u][w];
                    }
                    if constexpr (PRUNE) {
                        psig[r] = nr[u][WI];
                        if constexpr (!CPI) pdw[r] = (uint16_t)nr[u][WI + 1];
                    }
                    if constexpr (FOLD) {
                        const uint32_t key = nr[u][0] >> (32 - C::RB);
                        krank[u] = (key << 16) | atomicAdd(&bend[key], 1u);
                    }
                }
            }
            // Slot round: every unit's atomic is issued above; the stores that depend on the ranks
            // follow, so the commit pays one LDS round trip. A row of rank t < 8 files its id in
            // slot t of its key; a later one goes to the overflow list (bit 14 of krank), or, the
            // list full, stays off it (bit 15: it keeps its eight table partners).
            if constexpr (SLOT) {
#pragma unroll
                for (int u = 0; u < RPL; ++u) {
                    const uint32_t r = ot + u * NT;
                    if (r < n) {
                        const uint32_t key = krank[u] >> 16, t = krank[u] & 0xffff;
                        if (t < 8u) {
                            ktab[key * 8 + t] = (uint16_t)r;
                        } else {
                            const uint32_t o = atomicAdd(&novf, 1u);
                            if (o < (uint32_t)OVL) ovl[o] = (key << 16) | r;
                            krank[u] |= o < (uint32_t)OVL ? 0x4000u : 0x8000u;
                        }
                    }
                }
            }
        }
        if constexpr (!FINAL)
            for (int b = tid; b < C::HW; b += NT) hist_[b] = 0;
        if constexpr (!FOLD)
            for (int k = tid; k < C::NRESTS; k += NT) bend[k] = 0;
        if (tid == 0) npairs = 0;
        EH_STAMP(1);
        const int bn = xcd_bucket<C::NB>(blockIdx.x, it + 1, grid, nbk);
        const bool more = bn >= 0; // uniform
        const uint32_t fn = more ? (uint32_t)__builtin_amdgcn_readfirstlane(fill_next) : 0u;
        const uint32_t nn = min(fn, (uint32_t)CAP);
        pf_bk = more ? bn : bk;
        pf_n = nn;
        const int bn2 = xcd_bucket<C::NB>(blockIdx.x, it + 2, grid, nbk);
        issue(0, SLI); // nothing moves when !more (pf_n = 0), but the instruction count stays fixed
        fill_next = fill_of(bn2);
        eh_bar<1, NBAR>();
        EH_STAMP(2);

        // D1. key sort (eh_key_sort); a slot round has none
        uint32_t kpairs[FOLD ? RPL : 1];
        if constexpr (SLOT) {
            // the commit filed every row under its key. The phase reads as 0 cycles.
            if constexpr (STAMP) {
                if (threadIdx.x == 0) stamps[(size_t)bk * 16 + 3] = stamps[(size_t)bk * 16 + 2];
            }
            issue(SLI, 2 * SLI);
        } else {
            eh_key_sort<G>(rows, bend, sidx, wsum, pdrop, nonce, n, krank, kpairs);
            issue(SLI, 2 * SLI);
            eh_bar<4, NBAR>();
            EH_STAMP(3);
        }

        if constexpr (FINAL) {
            // D2, final round
            eh_final_candidates<G>(rows, psig, pdw, sidx, bend, ncand, cand, nonce, d, n);
            issue(2 * SLI, RPL);
        } else {
            // D2. pair list by per-wave compaction (eh_list_claim): one barrier. The sorted round's
            //     form is eh_list_sorted; the slot round's stays inline here (as a function it cost
            //     three VGPRs in (200,9) round 5, profiles/equihash_r11.md).
            if constexpr (SLOT) {
                // Slot round: a row of rank t in its key group pairs with the rows of smaller rank.
                // min(t, 8) of them are the first slots of ktab[key], one 16-byte LDS read, written
                // out by a short loop that selects the word in registers (eight predicated stores
                // lost 0.7% Sol/s, profiles/equihash_r10.md). A row on the overflow list (0.6 per
                // bucket) is listed by lane `ordinal`, not its own: all eight table rows, and the
                // list entries of its key with a smaller ordinal, at most 6 (the 14-partner cap).
                // Every unordered pair of a key group is so listed once, whatever order the atomics
                // took. Only when more than OVL rows were offered to the list (never seen) pairs
                // among overflow rows are lost; they are counted exactly: every overflow row adds
                // its t - 8, every list lane takes off the pairs it lists.
                uint32_t cnt = 0;
                uint32_t le = 0, lm = 0, ln = 0; // this lane's list entry, its partners on the list, its pairs
                const uint32_t nov = __builtin_amdgcn_readfirstlane(novf);
                const uint32_t NO = min(nov, (uint32_t)OVL);
                const bool full = nov > (uint32_t)OVL; // uniform
                ovf_sum += nov;
                ovf_max = max(ovf_max, nov);
#pragma unroll
                for (int u = 0; u < RPL; ++u) {
                    kpairs[u] = 0;
                    if (tid + u * NT < n) {
                        const uint32_t t = krank[u] & 0x3fffu, f = krank[u] & 0xc000u;
                        kpairs[u] = f == 0x4000u ? 0u : min(t, 8u);
                        if (full && f) atomicAdd(&pdrop[nonce * PDW + STAGE], t - 8u);
                    }
                }
                if ((uint32_t)tid < NO) {
                    le = ovl[tid];
                    uint32_t m = 0;
                    for (uint32_t q = 0; q < (uint32_t)tid; ++q) m += (ovl[q] >> 16) == (le >> 16) ? 1u : 0u;
                    lm = min(m, 6u);
                    if (full) {
                        if (lm) atomicSub(&pdrop[nonce * PDW + STAGE], lm);
                    } else if (m > 6u) {
                        atomicAdd(&pdrop[nonce * PDW + STAGE], m - 6u); // capped pairs (rare) count as pair-list drops
                    }
                    ln = 8u + lm;
                    cnt = ln;
                }
                // (the per-wave claim of eh_list_claim, deliberately written out: keep in step)
#pragma unroll
                for (int u = 0; u < RPL; ++u) cnt += kpairs[u];
                const uint32_t incl = wave_incl<false>(cnt);
                uint32_t wb = 0;
                if ((tid & 63) == 63) wb = atomicAdd(&npairs, incl);
                uint32_t o = __builtin_amdgcn_readlane(wb, 63) + incl - cnt;
                // the first c rows of `key`'s slots as partners of row i, at plist[o..]
                auto table_pairs = [&](uint32_t key, uint32_t c, uint32_t i) {
                    const u4v w = *reinterpret_cast<const u4v*>(&ktab[key * 8]);
                    const uint32_t room = o < (uint32_t)(MP * NT) ? (uint32_t)(MP * NT) - o : 0u;
                    const uint32_t ce = min(c, room);
                    for (uint32_t q = 0; q < ce; ++q) { // a short loop with a register select
                        const uint32_t ww = q < 4 ? (q < 2 ? w.x : w.y) : (q < 6 ? w.z : w.w);
                        plist[o + q] = ((q & 1) ? (ww & 0xffff0000u) : (ww << 16)) | i;
                    }
                    o += c;
                };
#pragma unroll
                for (int u = 0; u < RPL; ++u)
                    if (kpairs[u]) table_pairs(krank[u] >> 16, kpairs[u], tid + u * NT);
                if (ln) {
                    const uint32_t i = le & 0xffffu;
                    table_pairs(le >> 16, 8u, i);
                    for (uint32_t q = 0, k = 0; q < (uint32_t)tid && k < lm; ++q) {
                        const uint32_t e = ovl[q];
                        if ((e >> 16) != (le >> 16)) continue;
                        if (o < (uint32_t)(MP * NT)) plist[o] = (e << 16) | i;
                        ++o, ++k;
                    }
                }
            } else {
                eh_list_sorted<G>(sidx, plist, npairs, krank, kpairs);
            }
            eh_bar<BAR.list, NBAR>();
            EH_STAMP(7); // pair list complete (splits D2 into listing and filtering)
            const uint32_t P = npairs;
            const uint32_t Pc = min(P, (uint32_t)(MP * NT));
            if (tid == 0 && P > (uint32_t)(MP * NT)) atomicAdd(&pdrop[nonce * PDW + STAGE], P - MP * NT); // rare
            uint32_t pv[MP], pd[MP];
#pragma unroll
            for (int u = 0; u < MP; ++u) {
                const uint32_t k = tid + u * NT;
                pv[u] = NIL;
                pd[u] = 0;
                if (k < Pc) {
                    const uint32_t pr = plist[k];
                    const uint32_t i = pr & 0xffff, j = pr >> 16;
                    uint32_t dest;
                    if (pair_keep(i, j, dest)) {
                        pv[u] = (j << 16) | i;
                        pd[u] = dest; // destination bucket
                        hinc(hist_, pd[u]);
                    }
                }
            }
            // bend's last reads were before the barrier above; the next commit counts here
            for (int k = tid; k < C::NRESTS; k += NT) bend[k] = 0;
            if constexpr (SLOT) {
                if (tid == 0) novf = 0; // (read before the barrier above, like bend)
            }
            eh_bar<BAR.filter, NBAR>();
            EH_STAMP(4);
            // D3. claim this bucket's runs in the destination areas (device-scope atomics whose
            //     latency hides behind the scan and the scatter), then sort the pairs by
            //     destination: each pair takes the next LDS slot of its destination's run.
            //     Thread t owns destinations [t*BPT, t*BPT + BPT) (the scan's entry split).
            uint32_t myb[BPT];
#pragma unroll
            for (int k = 0; k < BPT; ++k) {
                const int b = tid * BPT + k;
                myb[k] = 0;
                if (b < C::NB) myb[k] = atomicAdd(&CTRout[(size_t)nonce * C::NB + b], hget(hist_, b)); // wave-uniform branch
            }
            issue(2 * SLI, RPL); // after the claim: waiting for its return then skips these loads
            uint32_t start = 0; // first LDS slot of the thread's first destination
            uint32_t np;
            EH_BAR_SCAN(BAR.scan, NBAR); // sorted round: barriers 7, 8; slot round: 4, 5
            if constexpr (C::H16)
                np = block_exscan<NT, BPT, uint16_t, uint16_t>(reinterpret_cast<const uint16_t*>(hist_),
                                                               reinterpret_cast<uint16_t*>(cur_), C::NB, wsum, &start);
            else
                np = block_exscan<NT, BPT>(hist_, cur_, C::NB, wsum, &start);
#pragma unroll
            for (int u = 0; u < MP; ++u)
                if (pv[u] != NIL) spair[hinc(cur_, pd[u])] = pv[u];
#pragma unroll
            for (int k = 0; k < BPT; ++k) { // LDS slot t of destination b -> run position base[b] + t
                const int b = tid * BPT + k;
                const uint32_t rb = myb[k] - start;
                if (b < C::NB) {
                    base[b] = (HT)rb;
                    start += hget(hist_, b);
                }
                if constexpr (TPO) { // the run base of (d, b) for eh_expand: consecutive lanes, consecutive words
                    const auto rs_b = buf_rsrc(Bout + ((size_t)nonce * C::NB + d) * C::NB, C::NB * 4);
                    __builtin_amdgcn_raw_buffer_store_b32(rb, rs_b, b < C::NB ? (uint32_t)b * 4 : OOB, 0, 0);
                }
            }
            eh_bar<BAR.sort, NBAR>();
            EH_STAMP(5);
            // D4. emit, one lane per output row in destination order: XOR, shift one digit,
            //     store into the claimed run (rows past the next round's capacity are dropped)
            const auto rs_out = buf_rsrc(Rout + (size_t)nonce * C::ROWS * SWO, (uint32_t)(C::ROWS * SWO * 4));
            const auto rs_p = buf_rsrc(Pout + (TPO ? ((size_t)nonce * C::NB + d) * PTW : 0), TPO ? PTW * 4 : 0);
#pragma unroll
            for (int u = 0; u < MP; ++u) { // fixed trip count, unconditional stores (see issue())
                const uint32_t t = tid + u * NT;
                const uint32_t pr = t < np ? spair[t] : 0u;
                const uint32_t i = pr & 0xffff, j = pr >> 16; // LDS rows = the parents' slots in the input area
                uint32_t x[WI + 1], o[WO];
                lds_row_xor<WI>(rows, i, j, x);
                x[WI - 1] &= ~RMI;
                x[WI] = 0;
                const uint32_t b = (x[0] >> (32 - C::DB)) & (C::NB - 1);
                const uint32_t pos = (HT)(base[b] + t);
                const bool ok = t < np && pos < OCAP;
                const uint32_t slot = b * C::AREA + pos;
#pragma unroll
                for (int w = 0; w < WO; ++w) o[w] = (x[w] << C::DB) | (x[w + 1] >> (32 - C::DB));
                uint32_t ov[SWO] = {};
#pragma unroll
                for (int w = 0; w < WO; ++w) ov[w] = o[w];
                if constexpr (TPO) {
                    ov[WO - 1] |= (uint32_t)d & RMO; // (d < NB: the whole bucket)
                } else if constexpr (C::cp(STAGE)) {
                    ov[WO - 1] |= (d >> C::DX) & RMO;
                    ov[WO] = cpack<C>(d, i, j);
                } else {
                    ov[WO] = (j << 16) | i;
                    ov[WO + 1] = d;
                }
                row_store<SWO>(rs_out, ok ? slot * (SWO * 4) : OOB, ov);
                // table parents: the pair word of ordinal t, lane after lane (t < MP * NT <= PTW)
                if constexpr (TPO) __builtin_amdgcn_raw_buffer_store_b32(pr, rs_p, t < np ? t * 4 : OOB, 0, 0);
            }
        }
        eh_bar<NBAR, NBAR>();
        EH_STAMP(6);
        if constexpr (SLOT) {
            if (!more || bn / C::NB != nonce) { // uniform: once per nonce and workgroup
                if (tid == 0 && ovf_sum) {
                    atomicAdd(&pdrop[nonce * PDW + 2 * C::K + 1 + STAGE], ovf_sum);
                    atomicMax(&pdrop[nonce * PDW + 3 * C::K + 1 + STAGE], ovf_max);
                }
                ovf_sum = ovf_max = 0;
            }
        }
        if (!more) break;
        bk = bn;
        ++it;
        fill = fn;
        n = nn;
    }
}


// ------------------------------------------------------------------ tree expansion
// The stage arrays (stage-s slot = row, parent word(s)) passed by value; LEAF: stage-0 leaf
// index per slot.
// p, b: the pair and run-base tables of the stages with table parents (EhCfg::tp).
struct EhStages {
    const uint32_t* r[16];
    const uint32_t* p[16];
    const uint32_t* b[16];
};
template <class C>
__global__ __launch_bounds__(C::L < 64 ? 64 : C::L) void eh_expand(const uint32_t* __restrict__ LEAF, EhStages st,
                                                                  const uint32_t* __restrict__ ncand,
                                                                  const uint64_t* __restrict__ cand,
                                                                  uint32_t* __restrict__ out_idx,
                                                                  uint32_t* __restrict__ out_valid,
                                                                  uint32_t* __restrict__ nout,
                                                                  uint32_t* __restrict__ out_list) {
    constexpr int L = C::L;
    __shared__ uint32_t buf[2][L];
    __shared__ uint64_t tri[L / 2 > 0 ? L / 2 : 1];
    __shared__ uint32_t dup;
    const uint32_t c = blockIdx.x % C::MAXCAND;
    const uint32_t nonce = blockIdx.x / C::MAXCAND;
    const uint32_t t = threadIdx.x;
    const uint32_t nc = min(ncand[nonce], (uint32_t)C::MAXCAND);
    if (c >= nc) return; // uniform per workgroup
    if (t == 0) {
        tri[0] = cand[(size_t)nonce * C::MAXCAND + c];
        dup = 0;
    }
    int cur = 0;
    // level s: 2^(K-s) triples of round s -> 2^(K-s+1) stage-(s-1) slots -> their triples. A
    // parent outside the slot arrays (never produced by a correct round) is clamped to slot 0
    // and the candidate is rejected, so no corrupt word can address past the stage arrays.
    for (int s = C::K; s >= 1; --s) {
        __syncthreads();
        const uint32_t cnt = 1u << (C::K - s);
        if (t < 2 * cnt) {
            const uint64_t tr = tri[t >> 1];
            const uint32_t dd = (uint32_t)(tr >> 32);
            const uint32_t r = (t & 1) ? (((uint32_t)tr >> 16) & 0xffff) : ((uint32_t)tr & 0xffff);
            const bool in = dd < (uint32_t)C::NB && r < (uint32_t)C::AREA;
            if (!in) dup = 1;
            buf[cur][t] = in ? dd * C::AREA + r : 0u;
        }
        __syncthreads();
        if (s > 1 && t < 2 * cnt) { // stage s-1 slot: row words, then the parent word(s)
            const uint32_t* q = st.r[s - 1] + ((size_t)nonce * C::ROWS + buf[cur][t]) * C::sw(s - 1) + C::words(s - 1);
            if (C::tp(s - 1)) {
                // table parents, three dependent reads: d from the row's padding, the slot's
                // ordinal in d's emit from the run base of (d, area), the pair word of that
                // ordinal. A d or an ordinal outside its table is clamped to entry 0 and the
                // candidate rejected; i and j are checked as LDS rows at the next level.
                const uint32_t area = buf[cur][t] / C::AREA, pos = buf[cur][t] % C::AREA;
                uint32_t d = q[-1] & C::tpmask(s - 1);
                if (d >= (uint32_t)C::NB) d = 0, dup = 1;
                const size_t db = (size_t)nonce * C::NB + d;
                uint32_t o = pos - st.b[s - 1][db * C::NB + area];
                if (o >= (uint32_t)C::ptab(s - 1)) o = 0, dup = 1;
                tri[t] = ((uint64_t)d << 32) | st.p[s - 1][db * C::ptab(s - 1) + o];
            } else if (C::cp(s - 1))
                tri[t] = ((uint64_t)cunpack_d<C>(q[0], q[-1]) << 32) | (q[0] & C::IMASK);
            else
                tri[t] = ((uint64_t)q[1] << 32) | q[0];
        }
    }
    __syncthreads();
    if (t < (uint32_t)L) buf[cur][t] = LEAF[(size_t)nonce * C::ROWS + buf[cur][t]];
    // Canonical order: at each level the subtree with the smaller first index goes left.
    for (int l = 0; l < C::K; ++l) {
        __syncthreads();
        if (t < (uint32_t)L) {
            const uint32_t w = 1u << l;
            const uint32_t j = t & ~(2 * w - 1);
            const bool swap = buf[cur][j + w] < buf[cur][j];
            const uint32_t pos = t - j;
            const uint32_t np = swap ? (pos < w ? pos + w : pos - w) : pos;
            buf[cur ^ 1][j + np] = buf[cur][t];
        }
        cur ^= 1;
    }
    __syncthreads();
    if (t < (uint32_t)L) out_idx[((size_t)nonce * C::MAXCAND + c) * L + t] = buf[cur][t];
    // Distinctness: bitonic sort a copy, then compare neighbours.
    const int o = cur ^ 1;
    if (t < (uint32_t)L) buf[o][t] = buf[cur][t];
    for (uint32_t k = 2; k <= (uint32_t)L; k <<= 1) {
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            __syncthreads();
            if (t < (uint32_t)L) {
                const uint32_t ixj = t ^ jj;
                if (ixj > t) {
                    const uint32_t a = buf[o][t], bb = buf[o][ixj];
                    const bool up = (t & k) == 0;
                    if ((a > bb) == up) {
                        buf[o][t] = bb;
                        buf[o][ixj] = a;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (t + 1 < (uint32_t)L && buf[o][t] == buf[o][t + 1]) atomicOr(&dup, 1u);
    __syncthreads();
    if (t == 0) out_valid[nonce * C::MAXCAND + c] = dup ? 0u : 1u;
    // Valid solutions are also appended to one compact list, (nonce, candidate, L indices) per
    // entry, so the host copies a few KB per nonce instead of MAXCAND * L words.
    if (dup) return; // uniform
    __shared__ uint32_t slot;
    if (t == 0) slot = atomicAdd(nout, 1u);
    __syncthreads();
    uint32_t* e = out_list + (size_t)slot * (L + 2);
    if (t == 0) {
        e[0] = nonce;
        e[1] = c;
    }
    if (t < (uint32_t)L) e[2 + t] = buf[cur][t];
}

} // namespace bcpk

namespace bcp {
namespace gpu {

static_assert(sizeof(EhBaseState) == sizeof(bcpk::EhBaseState), "EhBaseState mirror");

EhBaseState MakeEhBaseState(const CBlake2b& st_in) {
    CBlake2b st = st_in;
    Blake2bState& s = st.MutableState();
    if (s.buflen == 128) { // flush a full buffered block as non-final
        s.t[0] += 128;
        if (s.t[0] < 128) s.t[1]++;
        CBlake2b::Compress(s.h, s.buf, s.t[0], s.t[1], false);
        s.buflen = 0;
    }
    if (s.buflen + 4 > 128) throw std::runtime_error("MakeEhBaseState: g would straddle a block boundary");
    if (s.t[1] != 0) throw std::runtime_error("MakeEhBaseState: input too long");
    EhBaseState bs;
    memset(&bs, 0, sizeof(bs));
    memcpy(bs.h, s.h, sizeof(bs.h));
    unsigned char block[128] = {0};
    memcpy(block, s.buf, s.buflen);
    for (int i = 0; i < 16; ++i) memcpy(&bs.m[i], block + 8 * i, 8);
    bs.t0 = s.t[0] + s.buflen + 4;
    bs.g_byte = s.buflen;
    bs.outlen = s.outlen;
    return bs;
}

// Everything that depends on the configuration is a `template <class C>` member that reads the
// layout from C:: (equihash_layout.h); the public methods forward to them through dispatch_cfg.
struct EquihashGpuSolver::Impl {
    unsigned n, k;
    int batch, device;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_gen = nullptr, ev_rounds = nullptr; // this solver's last generation / rounds done (pipelining)
    DevBuf<bcpk::EhBaseState> d_states;
    DevBuf<uint32_t> d_ctr, d_leaf, d_ncand, d_idx, d_valid, d_pdrop, d_nout, d_out;
    DevBuf<uint64_t> d_cand;
    DevBuf<uint32_t> d_rst[16]; // merged layout: stage-s slot arrays (s = 0..K-1)
    DevBuf<uint32_t> d_ptab[16], d_btab[16]; // stages with table parents: pair tables [nonce][d][ptab], run bases [nonce][d][b]
    HostBuf<bcpk::EhBaseState> h_states;
    HostBuf<uint32_t> h_ncand, h_idx, h_ctr0, h_ctr_all, h_pdrop, h_nout, h_out;
    size_t outq = 0; // compact-list entries copied back with every batch (more: a second copy)
    int inflight = 0;
    // LaunchPow / CollectPow (kernels/equihash_pow.h); the buffers are allocated by the first LaunchPow
    DevBuf<uint32_t> d_in140, d_powctr, d_win; // inputs of the batch's nonces; winners + repeats counters; winner list
    HostBuf<uint32_t> h_powctr, h_win;
    bool pow_inflight = false; // the launch in flight is a LaunchPow
    EhPowJob pow_job;
    int ncu = 1;
    int groups = 1; // nonce groups of a launch (see launch()); 1: the whole batch is generated up front
    bool debug = false, stamp_mode = false;
    DevBuf<uint64_t> d_stamps;
    EhGpuStats stats;
    size_t bytes = 0;

    template <class C> void alloc() {
        d_states.alloc(batch);
        h_states.alloc(batch);
        static_assert(C::K <= 16, "stage arrays");
        for (int s = 0; s < C::K; ++s) d_rst[s].alloc((size_t)batch * C::ROWS * C::sw(s));
        for (int s = 0; s < C::K; ++s)
            if (C::tp(s)) {
                d_ptab[s].alloc((size_t)batch * C::NB * C::ptab(s));
                d_btab[s].alloc((size_t)batch * C::NB * C::NB);
            }
        d_ctr.alloc((size_t)C::K * batch * C::NB);
        d_leaf.alloc((size_t)batch * C::ROWS);
        d_ncand.alloc(batch);
        d_pdrop.alloc((size_t)batch * C::PDW); // per nonce (EhCfg::PDW): pair-list drops per round, row drops per stage, overflow rows
        h_pdrop.alloc((size_t)batch * C::PDW);
        d_cand.alloc((size_t)batch * C::MAXCAND);
        d_idx.alloc((size_t)batch * C::MAXCAND * C::L);
        d_valid.alloc((size_t)batch * C::MAXCAND);
        h_ncand.alloc(batch);
        d_nout.alloc(1);
        h_nout.alloc(1);
        d_out.alloc((size_t)batch * C::MAXCAND * (C::L + 2));
        h_out.alloc((size_t)batch * C::MAXCAND * (C::L + 2));
        outq = std::min<size_t>((size_t)batch * 4 + 16, (size_t)batch * C::MAXCAND);
        h_idx.alloc((size_t)C::MAXCAND * C::L);
        h_ctr0.alloc((size_t)C::K * C::NB);
        h_ctr_all.alloc((size_t)C::K * batch * C::NB);
        d_stamps.alloc((size_t)C::K * batch * C::NB * 16);
        bytes = d_leaf.n * 4 + d_ctr.n * 4 + d_idx.n * 4;
        for (int s = 0; s < C::K; ++s) bytes += (d_rst[s].n + d_ptab[s].n + d_btab[s].n) * 4;
    }

    // Persistent round kernels: as many workgroups as fit on the device at once.
    template <class C, int S, bool ST, bool CY> int round_grid(int nbk) {
        static int per_cu = -1;
        if (per_cu < 0) {
            int occ = 0;
            BCP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, bcpk::eh_round<C, S, ST, CY>, C::NT, 0));
            per_cu = std::max(occ, 1);
        }
        return std::min(nbk, ncu * per_cu);
    }
    // Kernel eh_round<C, S, STAMP, CARRY> over the group of `gn` nonces that starts at nonce `noff`.
    // CARRY: the round carries the generation of the next group's first `next` nonces.
    template <class C, int S, bool STAMP, bool CARRY> void launch_round_as(int noff, int gn, int next) {
        using G = bcpk::EhRoundGeom<C, S, CARRY>;
        constexpr bool OUT = !G::FINAL;       // the final round writes candidates, no stage
        constexpr int SO = OUT ? S : 0;       // the output stage
        constexpr bool TP = G::TPO;           // the output stage's parent tables
        constexpr size_t PDW = C::PDW;
        const size_t o = (size_t)noff;
        const uint32_t* rin = d_rst[S - 1].p + o * C::ROWS * G::SWI;
        uint32_t* rout = OUT ? d_rst[SO].p + o * C::ROWS * G::SWO : nullptr;
        const uint32_t* cin = d_ctr.p + ((size_t)(S - 1) * batch + o) * C::NB;
        uint32_t* cout = OUT ? d_ctr.p + ((size_t)S * batch + o) * C::NB : nullptr;
        uint32_t* pout = TP ? d_ptab[SO].p + o * C::NB * C::ptab(SO) : nullptr;
        uint32_t* bout = TP ? d_btab[SO].p + o * C::NB * C::NB : nullptr;
        uint64_t* st = STAMP ? d_stamps.p + ((size_t)(S - 1) * batch + o) * C::NB * 16 : nullptr;
        const int nbk = C::NB * gn;
        bcpk::EhCarry cy{};
        if constexpr (CARRY) {
            const size_t p = o + (size_t)gn; // the next group's first nonce
            cy.states = d_states.p + p;
            cy.R0 = d_rst[0].p + p * C::ROWS * C::sw(0);
            cy.LEAF = d_leaf.p + p * C::ROWS;
            cy.CTR0 = d_ctr.p + p * C::NB;
            cy.nonces = next;
        }
        hipLaunchKernelGGL((bcpk::eh_round<C, S, STAMP, CARRY>), dim3(round_grid<C, S, STAMP, CARRY>(nbk)), dim3(C::NT), 0,
                           stream, rin, cin, rout, cout, pout, bout, d_ncand.p + o, d_cand.p + o * C::MAXCAND, st,
                           d_pdrop.p + o * PDW, nbk, cy);
    }
    // Round S of a group. With next > 0 (and S < K) it carries the next group's generation; the
    // stamped diagnostic rounds never carry.
    template <class C, int S> void launch_round(int noff, int gn, int next) {
        if constexpr (C::GW > 0 && S < C::K) {
            if (next > 0 && !stamp_mode) {
                launch_round_as<C, S, false, true>(noff, gn, next);
                ++stats.carry_launches;
                return;
            }
        }
        if (stamp_mode) launch_round_as<C, S, true, false>(noff, gn, 0);
        else launch_round_as<C, S, false, false>(noff, gn, 0);
    }
    template <class C, int... S> void launch_rounds(int noff, int gn, int next, std::integer_sequence<int, S...>) {
        (launch_round<C, S + 1>(noff, gn, next), ...);
    }
    // The stand-alone generation of the first gen_n nonces: the register kernel where the
    // configuration's rows split evenly over its threads, else the LDS-sorted one.
    template <class C, bool HDR> void launch_gen(int gen_n) {
        using GR = bcpk::GenReg<C, C::GNT, C::GHPT>;
        if constexpr (GR::OK) {
            const int items = GR::GWG * gen_n;
            hipLaunchKernelGGL((bcpk::eh_gen_reg<C, HDR, C::GNT, C::GHPT>), dim3(items), dim3(C::GNT), 0, stream, d_states.p,
                               d_rst[0].p, d_leaf.p, d_ctr.p, items);
        } else
            hipLaunchKernelGGL((bcpk::eh_gen<C, HDR>), dim3(C::GENWG * gen_n), dim3(C::NTG), 0, stream, d_states.p,
                               d_rst[0].p, d_leaf.p, d_ctr.p);
    }
    // The tree expansion of `nonces` nonces. It walks the slot arrays and, for the stages with
    // table parents, their tables.
    template <class C> void launch_expand(size_t nonces) {
        constexpr int EB = C::L < 64 ? 64 : C::L;
        bcpk::EhStages stages{};
        for (int s = 0; s < C::K; ++s) stages.r[s] = d_rst[s].p, stages.p[s] = d_ptab[s].p, stages.b[s] = d_btab[s].p;
        hipLaunchKernelGGL((bcpk::eh_expand<C>), dim3(C::MAXCAND * nonces), dim3(EB), 0, stream, d_leaf.p, stages,
                           d_ncand.p, d_cand.p, d_idx.p, d_valid.p, d_nout.p, d_out.p);
    }

    template <class C> void alloc_pow() {
        using P = bcpk::PowCfg<C::N, C::K>;
        if (d_win.n) return;
        d_in140.alloc((size_t)batch * 35);
        d_powctr.alloc(2);
        h_powctr.alloc(2);
        d_win.alloc((size_t)batch * C::MAXCAND * P::WINW); // one entry per compact-list entry: no winner is lost
        h_win.alloc((size_t)batch * C::MAXCAND * P::WINW);
    }

    // Enqueue one batch. pow: the LaunchPow job (states built and winners filtered on the device) or
    // null; after: the solver whose batch this one is pipelined behind, or null.
    template <class C> void launch(size_t nstates, const bcpk::EhPowParams* pow, const Impl* after) {
        using P = bcpk::PowCfg<C::N, C::K>;
        if (pow) { // the states are built on the device
            BCP_HIP_CHECK(hipMemsetAsync(d_powctr.p, 0, 2 * sizeof(uint32_t), stream));
            hipLaunchKernelGGL((bcpk::eh_nonce_states<P>), dim3(((int)nstates + 63) / 64), dim3(64), 0, stream, *pow,
                               (int)nstates, d_in140.p, d_states.p);
        } else
            BCP_HIP_CHECK(hipMemcpyAsync(d_states.p, h_states.p, nstates * sizeof(bcpk::EhBaseState),
                                         hipMemcpyHostToDevice, stream));
        BCP_HIP_CHECK(hipMemsetAsync(d_ncand.p, 0, batch * sizeof(uint32_t), stream));
        BCP_HIP_CHECK(hipMemsetAsync(d_nout.p, 0, sizeof(uint32_t), stream));
        BCP_HIP_CHECK(hipMemsetAsync(d_pdrop.p, 0, d_pdrop.n * sizeof(uint32_t), stream));
        BCP_HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, d_ctr.n * sizeof(uint32_t), stream));
        if (debug) { // never-written slots and table entries read all-ones
            auto ones = [&](DevBuf<uint32_t>& b) {
                if (b.n) BCP_HIP_CHECK(hipMemsetAsync(b.p, 0xff, b.n * sizeof(uint32_t), stream));
            };
            ones(d_leaf);
            for (int s = 0; s < C::K; ++s) ones(d_rst[s]);
            for (int s = 0; s < C::K; ++s) ones(d_ptab[s]), ones(d_btab[s]);
        }
        BCP_HIP_CHECK(hipEventRecord(ev0, stream));
        // header-shaped inputs (140 B: g lands at byte 12 of the final block) take the
        // zero-message-word BLAKE2b specialisation
        bool hdr = true;
        for (size_t i = 0; i < nstates && !pow; ++i) {
            const bcpk::EhBaseState& st = h_states.p[i];
            hdr &= st.g_byte == 12;
            for (int w = 2; w < 16; ++w) hdr &= st.m[w] == 0;
        }
        // Nonce groups: the stand-alone kernel generates group 0 only, and rounds 1..K-1 of every
        // group carry the generation of the next one. One group is the whole batch generated up
        // front (inputs that are not header-shaped, configurations without generation waves and
        // the stamped diagnostic rounds always run that way).
        int gsz = (int)nstates;
        if (C::GW > 0 && hdr && !stamp_mode && groups > 1) {
            gsz = ((int)nstates + groups - 1) / groups;
            if (gsz >= bcpk::NXCD) gsz = (gsz + bcpk::NXCD - 1) / bcpk::NXCD * bcpk::NXCD; // keeps the XCD mapping
        }
        const int gen_n = std::min(gsz, (int)nstates); // nonces of the stand-alone generation
        if (after) BCP_HIP_CHECK(hipStreamWaitEvent(stream, after->ev_gen, 0)); // one generation at a time
        if (hdr) launch_gen<C, true>(gen_n);
        else launch_gen<C, false>(gen_n);
        BCP_HIP_CHECK(hipEventRecord(ev_gen, stream));
        if (after) BCP_HIP_CHECK(hipStreamWaitEvent(stream, after->ev_rounds, 0)); // one round chain at a time
        for (int noff = 0; noff < (int)nstates; noff += gsz) {
            const int gn = std::min(gsz, (int)nstates - noff);
            const int next = std::max(0, std::min(gsz, (int)nstates - noff - gsz));
            launch_rounds<C>(noff, gn, next, std::make_integer_sequence<int, C::K>{});
        }
        launch_expand<C>(nstates);
        BCP_HIP_CHECK(hipEventRecord(ev_rounds, stream));
        if (pow) {
            const int grid = (int)std::min<size_t>(C::MAXCAND * nstates, 2048); // grid-stride over the entries
            hipLaunchKernelGGL((bcpk::eh_pow_filter<P>), dim3(grid), dim3(64), 0, stream, *pow, (int)nstates, d_in140.p,
                               d_nout.p, d_out.p, (uint32_t)(C::MAXCAND * nstates), d_powctr.p, d_win.p, debug ? 1 : 0);
        }
        BCP_HIP_CHECK(hipGetLastError());
        BCP_HIP_CHECK(hipEventRecord(ev1, stream));
        BCP_HIP_CHECK(
            hipMemcpyAsync(h_ncand.p, d_ncand.p, nstates * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        // pair-list and row drops of every nonce (a few words)
        BCP_HIP_CHECK(hipMemcpyAsync(h_pdrop.p, d_pdrop.p, d_pdrop.n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (debug) { // per-stage fills of nonce 0's buckets
            for (int s = 0; s < C::K; ++s)
                BCP_HIP_CHECK(hipMemcpyAsync(h_ctr0.p + (size_t)s * C::NB, d_ctr.p + (size_t)s * batch * C::NB,
                                             C::NB * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            BCP_HIP_CHECK(hipMemcpyAsync(h_ctr_all.p, d_ctr.p, d_ctr.n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        }
        BCP_HIP_CHECK(hipMemcpyAsync(h_nout.p, d_nout.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (pow) { // the winners instead of the index lists
            BCP_HIP_CHECK(hipMemcpyAsync(h_powctr.p, d_powctr.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            BCP_HIP_CHECK(hipMemcpyAsync(h_win.p, d_win.p, outq * P::WINW * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        } else
            BCP_HIP_CHECK(hipMemcpyAsync(h_out.p, d_out.p, outq * (C::L + 2) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                         stream));
        if (debug) // every candidate of nonce 0, valid or not
            BCP_HIP_CHECK(hipMemcpyAsync(h_idx.p, d_idx.p, C::MAXCAND * C::L * sizeof(uint32_t),
                                         hipMemcpyDeviceToHost, stream));
    }

    // What a public method returns: f(C{}) of this solver's configuration C.
    template <class R, class F> R with_cfg(F&& f) {
        R out;
        dispatch_cfg(n, k, [&](auto c) { out = f(c); });
        return out;
    }
    // The solver a launch is pipelined behind, checked.
    const Impl* behind(const EquihashGpuSolver& prev) const {
        if (prev.impl.get() == this) throw std::invalid_argument("EquihashGpuSolver: cannot pipeline behind itself");
        if (prev.impl->device != device) throw std::invalid_argument("EquihashGpuSolver: pipelined solvers on different devices");
        return prev.impl.get();
    }
    void launch_states(const std::vector<EhBaseState>& states, const Impl* after) {
        if (states.empty() || (int)states.size() > batch) throw std::invalid_argument("bad number of states");
        if (inflight) throw std::runtime_error("EquihashGpuSolver: Collect() the previous launch first");
        BCP_HIP_CHECK(hipSetDevice(device));
        memcpy(h_states.p, states.data(), states.size() * sizeof(EhBaseState));
        dispatch_cfg(n, k, [&](auto c) { launch<decltype(c)>(states.size(), nullptr, after); });
        inflight = (int)states.size();
    }
    void launch_pow(const EhPowJob& job, const Impl* after) {
        if (job.count < 1 || job.count > batch) throw std::invalid_argument("LaunchPow: count must be 1..Batch()");
        if (inflight) throw std::runtime_error("EquihashGpuSolver: Collect() the previous launch first");
        BCP_HIP_CHECK(hipSetDevice(device));
        bcpk::EhPowParams p;
        static_assert(sizeof(p.prefix) == sizeof(job.prefix) && sizeof(p.nonce) == 32 && sizeof(p.target) == 32, "job words");
        memcpy(p.prefix, job.prefix, sizeof(p.prefix));
        memcpy(p.nonce, job.nonce_first, 32);
        memcpy(p.target, job.target_le, 32);
        dispatch_cfg(n, k, [&](auto c) {
            alloc_pow<decltype(c)>();
            launch<decltype(c)>((size_t)job.count, &p, after);
        });
        pow_job = job;
        pow_inflight = true;
        inflight = job.count;
    }

    // The end of a launch, for Collect and CollectPow: the wait, the event time, the drop and fill
    // statistics and the candidate counts. Returns the number of nonces that were in flight.
    template <class C> int finish() {
        pow_inflight = false;
        BCP_HIP_CHECK(hipSetDevice(device));
        BCP_HIP_CHECK(hipStreamSynchronize(stream));
        const int ns = inflight;
        inflight = 0;
        float ms = 0;
        BCP_HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
        stats.gpu_ms += ms;
        stats.nonces += ns;
        constexpr size_t K = C::K, NB = C::NB;
        // every nonce: pair-list drops per round and rows past a round's capacity per stage (accumulated)
        stats.pair_dropped_all.resize(K + 1, 0);
        stats.stage_dropped_all.resize(K, 0);
        stats.pair_dropped_nonce.assign(ns, 0);
        stats.stage_dropped_nonce.assign(ns, 0);
        std::vector<uint64_t> pd(K + 1, 0);
        for (int nn = 0; nn < ns; ++nn) {
            const uint32_t* q = h_pdrop.p + (size_t)nn * C::PDW;
            for (size_t r = 0; r <= K; ++r) {
                pd[r] += q[r];
                stats.pair_dropped_all[r] += q[r];
                stats.pair_dropped_nonce[nn] += q[r];
            }
            for (size_t s = 0; s < K; ++s) {
                stats.stage_dropped_all[s] += q[K + 1 + s];
                stats.stage_dropped_nonce[nn] += q[K + 1 + s];
            }
            // slot rounds: rows past the key slots, and the most in one bucket
            stats.overflow_rows_all.resize(K + 1, 0);
            stats.overflow_bucket_max.resize(K + 1, 0);
            for (size_t r = 1; r <= K; ++r) {
                stats.overflow_rows_all[r] += q[2 * K + 1 + r];
                stats.overflow_bucket_max[r] = std::max<uint64_t>(stats.overflow_bucket_max[r], q[3 * K + 1 + r]);
            }
        }
        if (debug) stats.pair_dropped = pd;
        if (debug) {
            // nonce 0: per stage, rows offered to each bucket (its fill counter) vs the LDS capacity
            // of the round that reads it
            stats.stage_rows.assign(K, 0);
            stats.stage_dropped.assign(K, 0);
            stats.stage_maxfill.assign(K, 0);
            stats.stage_top.assign(K, {});
            // every nonce of the batch: the fullest bucket per stage and the buckets past capacity
            stats.stage_maxfill_all.assign(K, 0);
            for (size_t s = 0; s < K; ++s)
                for (size_t x = 0; x < (size_t)ns * NB; ++x) {
                    const uint64_t fill = h_ctr_all.p[(s * batch) * NB + x];
                    stats.stage_maxfill_all[s] = std::max<uint64_t>(stats.stage_maxfill_all[s], fill);
                    if (fill > (uint64_t)C::cap(s + 1)) stats.overflow_fills.push_back((uint64_t)s << 32 | fill);
                }
            for (size_t s = 0; s < K; ++s) {
                const uint64_t cap = C::cap(s + 1);
                std::vector<uint64_t> fills;
                for (size_t dd = 0; dd < NB; ++dd) {
                    const uint64_t fill = h_ctr0.p[s * NB + dd];
                    fills.push_back(fill);
                    stats.stage_rows[s] += fill;
                    stats.stage_maxfill[s] = std::max<uint64_t>(stats.stage_maxfill[s], fill);
                    if (fill > cap) {
                        stats.stage_dropped[s] += fill - cap;
                        stats.dropped_rows += fill - cap;
                    }
                }
                std::sort(fills.rbegin(), fills.rend());
                fills.resize(std::min<size_t>(fills.size(), 8));
                stats.stage_top[s] = fills;
            }
            stats.debug_cands.clear();
            const uint32_t nc = std::min<uint32_t>(h_ncand.p[0], (uint32_t)C::MAXCAND);
            for (uint32_t c = 0; c < nc; ++c) {
                const uint32_t* p = h_idx.p + (size_t)c * C::L;
                stats.debug_cands.emplace_back(p, p + C::L);
            }
        }
        uint64_t cands = 0;
        for (int nn = 0; nn < ns; ++nn) {
            const uint32_t c = h_ncand.p[nn];
            cands += std::min<uint32_t>(c, (uint32_t)C::MAXCAND);
            stats.cand_max = std::max<uint64_t>(stats.cand_max, c);
            if (c > (uint32_t)C::MAXCAND) stats.cand_dropped += c - C::MAXCAND; // lost candidates, maybe solutions
        }
        stats.candidates += cands;
        stats.duplicates += cands - h_nout.p[0];
        return ns;
    }

    template <class C> std::vector<std::vector<std::vector<uint32_t>>> collect() {
        const int ns = finish<C>();
        std::vector<std::vector<std::vector<uint32_t>>> out(ns);
        constexpr size_t ew = C::L + 2; // compact-list entry: nonce, candidate, L indices
        const size_t nout = h_nout.p[0];
        if (nout > outq) // more valid solutions than the per-batch copy holds: fetch the rest
            BCP_HIP_CHECK(hipMemcpy(h_out.p + outq * ew, d_out.p + outq * ew, (nout - outq) * ew * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost));
        // the list is in completion order: put every nonce's solutions in candidate order
        std::vector<std::pair<uint64_t, const uint32_t*>> ents;
        ents.reserve(nout);
        for (size_t e = 0; e < nout; ++e) {
            const uint32_t* p = h_out.p + e * ew;
            if (p[0] < (uint32_t)ns) ents.emplace_back(((uint64_t)p[0] << 32) | p[1], p + 2);
        }
        std::sort(ents.begin(), ents.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (const auto& en : ents) {
            const int nn = (int)(en.first >> 32);
            std::vector<uint32_t> v(en.second, en.second + C::L);
            bool seen = false;
            for (auto& prev : out[nn]) seen |= (prev == v);
            if (seen) continue;
            out[nn].push_back(std::move(v));
            stats.solutions++;
        }
        return out;
    }

    // The winners of a LaunchPow (the index lists stayed on the device).
    template <class C> EhPowResult collect_pow() {
        constexpr size_t winw = bcpk::PowCfg<C::N, C::K>::WINW; // words per winner entry
        const int ns = finish<C>();
        const size_t nout = h_nout.p[0], nwin = h_powctr.p[0], ndup = h_powctr.p[1];
        if (nwin > outq) // more winners than the per-batch copy holds: fetch the rest
            BCP_HIP_CHECK(hipMemcpy(h_win.p + outq * winw, d_win.p + outq * winw, (nwin - outq) * winw * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost));
        EhPowResult res;
        res.solutions = nout - ndup;
        stats.solutions += res.solutions;
        const size_t solw = (winw - 11) * 4;
        // the list is in completion order: by position in the nonce range, then by hash as an integer
        std::vector<const uint32_t*> ents;
        for (size_t e = 0; e < nwin; ++e) {
            const uint32_t* p = h_win.p + e * winw;
            if (p[0] < (uint32_t)ns) ents.push_back(p);
        }
        std::sort(ents.begin(), ents.end(), [](const uint32_t* a, const uint32_t* b) {
            if (a[0] != b[0]) return a[0] < b[0];
            for (int i = 7; i >= 0; --i)
                if (a[3 + i] != b[3 + i]) return a[3 + i] < b[3 + i];
            return a[1] < b[1];
        });
        for (const uint32_t* p : ents) {
            EhPowHit h;
            uint64_t carry = p[0];
            for (int q = 0; q < 4; ++q) { // nonce_first + position, 256-bit little-endian
                uint64_t a;
                memcpy(&a, pow_job.nonce_first + 8 * q, 8);
                const uint64_t s = a + carry;
                carry = s < a ? 1 : 0;
                memcpy(h.nonce + 8 * q, &s, 8);
            }
            memcpy(h.hash, p + 3, 32);
            h.solution.assign(reinterpret_cast<const unsigned char*>(p + 11), reinterpret_cast<const unsigned char*>(p + 11) + solw);
            if (debug) {
                res.all.push_back(h);
                res.all_pass.push_back(p[2] ? 1 : 0);
            }
            if (p[2]) res.hits.push_back(std::move(h));
        }
        return res;
    }

    // Mean cycles per phase per round (diagnostic stamp builds): [stage][phase delta], deltas
    // 1..6 = commit, next-bucket issue + barrier, key sort, pair enumeration, claim + pair sort, emit;
    // [0] = whole bucket. A slot round has no key sort: it stamps the phase's end with its start, 0 cycles.
    template <class C> std::vector<std::vector<double>> phase_cycles(int nonces) {
        BCP_HIP_CHECK(hipSetDevice(device));
        BCP_HIP_CHECK(hipStreamSynchronize(stream));
        const size_t per = (size_t)batch * C::NB * 16;
        std::vector<uint64_t> h(C::K * per);
        BCP_HIP_CHECK(hipMemcpy(h.data(), d_stamps.p, h.size() * 8, hipMemcpyDeviceToHost));
        std::vector<std::vector<double>> out;
        for (size_t s = 0; s < (size_t)C::K; ++s) {
            // phases 1..6, then D2 split at stamp 7: listing (3 -> 7) and filtering (7 -> 4)
            std::vector<double> acc(9, 0.0);
            size_t cnt = 0;
            for (size_t wg = 0; wg < (size_t)nonces * C::NB; ++wg) {
                const uint64_t* t = &h[s * per + wg * 16];
                if (t[0] == 0) continue;
                for (int k = 1; k < 7; ++k) // (a phase counts when both of its stamps were taken)
                    if (t[k] >= t[k - 1] && t[k - 1] != 0) acc[k] += (double)(t[k] - t[k - 1]);
                acc[0] += (double)(t[6] - t[0]);
                if (t[7] >= t[3] && t[4] >= t[7] && t[7] != 0) {
                    acc[7] += (double)(t[7] - t[3]);
                    acc[8] += (double)(t[4] - t[7]);
                }
                ++cnt;
            }
            for (auto& a : acc) a = cnt ? a / cnt : 0;
            out.push_back(acc);
        }
        return out;
    }

    // Debug mode: one nonce of the last batch, its bucket fill counters (rows offered to each bucket),
    // K stages of NB.
    template <class C> std::vector<uint32_t> debug_fills(int nonce) {
        if (!debug || nonce < 0 || nonce >= batch) throw std::invalid_argument("DebugFills: debug mode and a nonce of the batch");
        BCP_HIP_CHECK(hipSetDevice(device));
        BCP_HIP_CHECK(hipStreamSynchronize(stream));
        std::vector<uint32_t> out;
        for (size_t s = 0; s < (size_t)C::K; ++s) {
            const uint32_t* p = h_ctr_all.p + (s * batch + nonce) * C::NB;
            out.insert(out.end(), p, p + C::NB);
        }
        return out;
    }

    // Debug: one nonce of the last batch, K arrays of ROWS slots: stage-0 leaf indices (zero-extended),
    // then the parent triples of stages 1..K-1; with SetDebug(true) never-written slots read all-ones.
    template <class C> std::vector<uint64_t> debug_dump(int nonce) {
        if (nonce < 0 || nonce >= batch) throw std::invalid_argument("DebugDump: nonce outside the batch");
        BCP_HIP_CHECK(hipSetDevice(device));
        BCP_HIP_CHECK(hipStreamSynchronize(stream));
        constexpr size_t R = C::ROWS, NB = C::NB;
        std::vector<uint64_t> out(C::K * R);
        std::vector<uint32_t> leaf(R);
        BCP_HIP_CHECK(hipMemcpy(leaf.data(), d_leaf.p + (size_t)nonce * R, R * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < R; ++i) out[i] = leaf[i];
        for (int s = 1; s < C::K; ++s) {
            const size_t sw = C::sw(s), w = C::words(s), pw = C::ptab(s);
            std::vector<uint32_t> buf(R * sw), bt, pt;
            BCP_HIP_CHECK(hipMemcpy(buf.data(), d_rst[s].p + (size_t)nonce * R * sw, R * sw * 4, hipMemcpyDeviceToHost));
            if (C::tp(s)) { // the triple through the run-base and pair tables, as eh_expand walks it
                bt.resize(NB * NB), pt.resize(NB * pw);
                BCP_HIP_CHECK(hipMemcpy(bt.data(), d_btab[s].p + (size_t)nonce * NB * NB, bt.size() * 4, hipMemcpyDeviceToHost));
                BCP_HIP_CHECK(hipMemcpy(pt.data(), d_ptab[s].p + (size_t)nonce * NB * pw, pt.size() * 4, hipMemcpyDeviceToHost));
            }
            for (size_t i = 0; i < R; ++i) {
                const uint32_t* slot = &buf[i * sw];
                // A slot never written keeps the SetDebug fill. Table parents: in every row word (a
                // row ends in zero padding above its producing bucket, or is not all-ones with
                // overwhelming odds); else in its parent word (no LDS row index is all-ones).
                bool unwritten = C::tp(s) || (C::cp(s) && slot[w] == bcpk::NIL), in_range;
                for (size_t x = 0; x < w && C::tp(s); ++x) unwritten &= slot[x] == bcpk::NIL;
                out[s * R + i] = unwritten   ? ~0ull
                                 : C::tp(s) ? bcpk::table_parent<C>(s, slot, i / C::AREA, i % C::AREA, bt.data(), pt.data(), &in_range)
                                            : bcpk::slot_parent<C>(s, slot);
            }
        }
        return out;
    }

    // DebugExpandCorrupt (gpu_api.h): corrupt one parent of nonce 0's first candidate, expand again.
    template <class C> std::vector<uint32_t> debug_expand_corrupt(int mode) {
        BCP_HIP_CHECK(hipSetDevice(device));
        BCP_HIP_CHECK(hipStreamSynchronize(stream));
        uint32_t nc = 0;
        BCP_HIP_CHECK(hipMemcpy(&nc, d_ncand.p, 4, hipMemcpyDeviceToHost));
        nc = std::min<uint32_t>(nc, (uint32_t)C::MAXCAND);
        if (nc == 0) return {};
        uint64_t tri = 0;
        BCP_HIP_CHECK(hipMemcpy(&tri, d_cand.p, 8, hipMemcpyDeviceToHost));
        constexpr int ST = C::K - 1; // the stage the final round read: its slots carry their parent word(s)
        static_assert(!C::tp(ST), "the last stage keeps its parents in the slots");
        const uint32_t d = (uint32_t)(tri >> 32), i = (uint32_t)tri & 0xffff;
        uint32_t* slot = d_rst[ST].p + ((size_t)d * C::AREA + i) * C::sw(ST);
        uint32_t w[C::sw(ST)] = {};
        if (mode != 0) BCP_HIP_CHECK(hipMemcpy(w, slot, sizeof(w), hipMemcpyDeviceToHost));
        uint32_t* pw = w + C::words(ST); // the parent word(s)
        if (mode == 3 || mode == 4) {
            // The table walk of a stage-(K-2) parent of the first candidate: mode 3 sets a padding bit
            // above the producing bucket in its row (a bucket >= NB), mode 4 rewrites the run base of
            // its (bucket, area) so that the slot's ordinal is the first one past the pair table.
            if (ST < 2 || !C::tp(ST - 1) || C::tpmask(ST - 1) < (uint32_t)C::NB)
                throw std::invalid_argument("DebugExpandCorrupt: modes 3 and 4 need table parents with spare padding in stage K-2");
            const uint64_t par = bcpk::slot_parent<C>(ST, w); // the slot's left parent: area d1, position i1
            const uint32_t d1 = (uint32_t)(par >> 32), i1 = (uint32_t)par & 0xffff;
            if (d1 >= (uint32_t)C::NB || i1 >= (uint32_t)C::AREA) throw std::runtime_error("DebugExpandCorrupt: the first candidate's parent is out of range");
            uint32_t* lw = d_rst[ST - 1].p + ((size_t)d1 * C::AREA + i1) * C::sw(ST - 1) + C::words(ST - 1) - 1;
            uint32_t x = 0;
            BCP_HIP_CHECK(hipMemcpy(&x, lw, 4, hipMemcpyDeviceToHost));
            if (mode == 3) {
                x |= (uint32_t)C::NB;
                BCP_HIP_CHECK(hipMemcpy(lw, &x, 4, hipMemcpyHostToDevice));
            } else {
                const uint32_t d2 = x & C::tpmask(ST - 1);
                if (d2 >= (uint32_t)C::NB) throw std::runtime_error("DebugExpandCorrupt: the parent row's bucket is out of range");
                const uint32_t rb = i1 - (uint32_t)C::ptab(ST - 1);
                BCP_HIP_CHECK(hipMemcpy(d_btab[ST - 1].p + (size_t)d2 * C::NB + d1, &rb, 4, hipMemcpyHostToDevice));
            }
        } else if (mode != 0) {
            if (C::cp(ST)) // compact word: i | j << 16 with the bucket's bits in the spare high bits of each half
                pw[0] = mode == 1 ? (pw[0] | (C::DHM << C::IB) | (C::DHM << (16 + C::IB))) : (pw[0] | ((1u << C::IB) - 1));
            else if (mode == 1) pw[1] = 0xffffu;          // producing bucket far past NB
            else pw[0] = (pw[0] & 0xffff0000u) | 0xffffu; // LDS row far past the area
            BCP_HIP_CHECK(hipMemcpy(slot + C::words(ST), pw, (C::sw(ST) - C::words(ST)) * 4, hipMemcpyHostToDevice));
        }
        BCP_HIP_CHECK(hipMemsetAsync(d_nout.p, 0, 4, stream));
        launch_expand<C>(1);
        BCP_HIP_CHECK(hipGetLastError());
        BCP_HIP_CHECK(hipStreamSynchronize(stream));
        std::vector<uint32_t> valid(nc);
        BCP_HIP_CHECK(hipMemcpy(valid.data(), d_valid.p, nc * 4, hipMemcpyDeviceToHost));
        return valid;
    }
};

EquihashGpuSolver::EquihashGpuSolver(unsigned n, unsigned k, int batch, int device) : impl(new Impl) {
    if (batch < 1) throw std::invalid_argument("batch must be >= 1");
    impl->n = n;
    impl->k = k;
    impl->batch = batch;
    impl->device = UseDevice(device);
    // BCP_EH_GROUPS=n: split every launch into n nonce groups (1 = no carried generation)
    impl->groups = BCP_EH_GROUPS_DEFAULT(batch);
    if (const char* e = getenv("BCP_EH_GROUPS")) impl->groups = std::max(1, atoi(e));
    impl->groups = std::min(impl->groups, batch);
    BCP_HIP_CHECK(hipDeviceGetAttribute(&impl->ncu, hipDeviceAttributeMultiprocessorCount, impl->device));
    BCP_HIP_CHECK(hipStreamCreateWithFlags(&impl->stream, hipStreamNonBlocking));
    BCP_HIP_CHECK(hipEventCreateWithFlags(&impl->ev_gen, hipEventDisableTiming));
    BCP_HIP_CHECK(hipEventCreateWithFlags(&impl->ev_rounds, hipEventDisableTiming));
    BCP_HIP_CHECK(hipEventCreate(&impl->ev0));
    BCP_HIP_CHECK(hipEventCreate(&impl->ev1));
    dispatch_cfg(n, k, [&](auto c) { impl->alloc<decltype(c)>(); });
}

EquihashGpuSolver::~EquihashGpuSolver() {
    if (impl) {
        (void)hipSetDevice(impl->device);
        if (impl->stream) (void)hipStreamSynchronize(impl->stream);
        if (impl->ev0) (void)hipEventDestroy(impl->ev0);
        if (impl->ev1) (void)hipEventDestroy(impl->ev1);
        if (impl->stream) (void)hipStreamDestroy(impl->stream);
        if (impl->ev_gen) (void)hipEventDestroy(impl->ev_gen);
        if (impl->ev_rounds) (void)hipEventDestroy(impl->ev_rounds);
    }
}

unsigned EquihashGpuSolver::N() const { return impl->n; }
unsigned EquihashGpuSolver::K() const { return impl->k; }
int EquihashGpuSolver::Batch() const { return impl->batch; }
const EhGpuStats& EquihashGpuSolver::Stats() const { return impl->stats; }
void EquihashGpuSolver::SetDebug(bool on) { impl->debug = on; }
void EquihashGpuSolver::SetStampMode(bool on) {
    impl->stamp_mode = on;
    if (on) { // a stamp no kernel writes (the final round has no phases 4, 5 and 7) reads as zero: PhaseCycles skips it
        BCP_HIP_CHECK(hipSetDevice(impl->device));
        BCP_HIP_CHECK(hipMemsetAsync(impl->d_stamps.p, 0, impl->d_stamps.n * sizeof(uint64_t), impl->stream));
    }
}
void EquihashGpuSolver::ResetStats() { impl->stats = EhGpuStats(); }
size_t EquihashGpuSolver::DeviceBytes() const { return impl->bytes; }

std::vector<std::vector<double>> EquihashGpuSolver::PhaseCycles(int nonces) {
    return impl->with_cfg<std::vector<std::vector<double>>>([&](auto c) { return impl->phase_cycles<decltype(c)>(nonces); });
}
std::vector<uint32_t> EquihashGpuSolver::DebugFills(int nonce) {
    return impl->with_cfg<std::vector<uint32_t>>([&](auto c) { return impl->debug_fills<decltype(c)>(nonce); });
}
std::vector<uint64_t> EquihashGpuSolver::DebugDump(int nonce) {
    return impl->with_cfg<std::vector<uint64_t>>([&](auto c) { return impl->debug_dump<decltype(c)>(nonce); });
}
std::vector<uint32_t> EquihashGpuSolver::DebugExpandCorrupt(int mode) {
    return impl->with_cfg<std::vector<uint32_t>>([&](auto c) { return impl->debug_expand_corrupt<decltype(c)>(mode); });
}

void EquihashGpuSolver::Launch(const std::vector<EhBaseState>& states) { impl->launch_states(states, nullptr); }
void EquihashGpuSolver::Launch(const std::vector<EhBaseState>& states, const EquihashGpuSolver& prev) {
    impl->launch_states(states, impl->behind(prev));
}
void EquihashGpuSolver::LaunchPow(const EhPowJob& job) { impl->launch_pow(job, nullptr); }
void EquihashGpuSolver::LaunchPow(const EhPowJob& job, const EquihashGpuSolver& prev) {
    impl->launch_pow(job, impl->behind(prev));
}

EhPowResult EquihashGpuSolver::CollectPow() {
    if (!impl->inflight) throw std::runtime_error("EquihashGpuSolver: nothing in flight");
    if (!impl->pow_inflight) throw std::runtime_error("EquihashGpuSolver: the launch in flight is a Launch(); use Collect()");
    return impl->with_cfg<EhPowResult>([&](auto c) { return impl->collect_pow<decltype(c)>(); });
}

std::vector<std::vector<std::vector<uint32_t>>> EquihashGpuSolver::Collect() {
    if (!impl->inflight) throw std::runtime_error("EquihashGpuSolver: nothing in flight");
    if (impl->pow_inflight) throw std::runtime_error("EquihashGpuSolver: the launch in flight is a LaunchPow(); use CollectPow()");
    return impl->with_cfg<std::vector<std::vector<std::vector<uint32_t>>>>([&](auto c) { return impl->collect<decltype(c)>(); });
}

std::vector<std::vector<std::vector<uint32_t>>> EquihashGpuSolver::Solve(const std::vector<EhBaseState>& states) {
    Launch(states);
    return Collect();
}

} // namespace gpu
} // namespace bcp

