// bloomscan_tests: the batched BIP37 scan of a transaction list (csrc/net/bloomscan.h) on the CPU
// (allowGpu = false): which elements it extracts and in what order, and that verdicts and filter
// equal a loop of CBloomFilter::IsRelevantAndUpdate (reference src/bloom.cpp:121-178) over the
// list, where inserts under BLOOM_UPDATE_ALL / P2PUBKEY_ONLY make later matches depend on
// earlier ones. tests/test_bloom_gpu.py runs the same cases with the passes on the device.
#include "test/unittest.h"

#include "consensus/merkleblock.h"
#include "net/bloomscan.h"
#include "primitives/serialize.h"
#include "script/script.h"
#include "util/strencodings.h"
#include "util/util.h"

#include <algorithm>
#include <random>
#include <tuple>

using namespace bcp;
using namespace bcp::test;

namespace {

typedef std::vector<unsigned char> Bytes;

Bytes RandBytes(std::mt19937& rng, size_t n) {
    Bytes v(n);
    for (auto& c : v) c = (unsigned char)rng();
    return v;
}
uint256 RandHash(std::mt19937& rng) {
    uint256 h;
    for (int j = 0; j < 32; j++) h.begin()[j] = (unsigned char)rng();
    return h;
}
Bytes FakePubKey(std::mt19937& rng) {
    Bytes k = RandBytes(rng, 33);
    k[0] = 0x02;
    return k;
}
CScript P2PKH(const Bytes& h20) { return CScript() << OP_DUP << OP_HASH160 << h20 << OP_EQUALVERIFY << OP_CHECKSIG; }
CScript P2PK(const Bytes& pub) { return CScript() << pub << OP_CHECKSIG; }
CScript P2SH(const Bytes& h20) { return CScript() << OP_HASH160 << h20 << OP_EQUAL; }
CScript Multisig1of2(const Bytes& a, const Bytes& b) { return CScript() << OP_1 << a << b << OP_2 << OP_CHECKMULTISIG; }
CScript RawScript(const Bytes& b) { return CScript(b.begin(), b.end()); }
CScript SigScript(const Bytes& sig, const Bytes& pub) { return CScript() << sig << pub; }

CTransactionRef Tx(const std::vector<std::pair<COutPoint, CScript>>& ins, const std::vector<CScript>& outs) {
    CMutableTransaction t;
    t.nVersion = 1;
    for (const auto& i : ins) {
        CTxIn in;
        in.prevout = i.first;
        in.scriptSig = i.second;
        t.vin.push_back(in);
    }
    for (size_t i = 0; i < outs.size(); i++) t.vout.push_back(CTxOut(1000 + i, outs[i]));
    return MakeTransactionRef(t);
}

// a filter from its parts, in the state net processing keeps a loaded one in
CBloomFilter MakeFilter(const Bytes& vData, unsigned nHashFuncs, unsigned nTweak, unsigned char nFlags) {
    Bytes ser;
    VectorWriter w(ser);
    w << vData << nHashFuncs << nTweak << nFlags;
    SpanReader r(ser.data(), ser.size(), SER_NETWORK, PROTOCOL_VERSION);
    CBloomFilter f;
    r >> f;
    f.UpdateEmptyFull();
    return f;
}
std::string SerHex(const CBloomFilter& f) {
    const Bytes v = SerializeToBytes(f);
    return HexStr(v.begin(), v.end());
}

typedef std::tuple<int, int, Bytes> El; // kind, index, data
std::vector<El> Extract(const CTransactionRef& tx) {
    std::vector<El> out;
    for (const BloomElement& e : BloomExtractElements({tx})) {
        CHECK_EQ(e.tx, 0u);
        out.emplace_back((int)e.kind, (int)e.index, e.data);
    }
    return out;
}
// what IsRelevantAndUpdate tests, written with CScript::GetOp as it is there
std::vector<El> ModelExtract(const CTransaction& tx) {
    std::vector<El> out;
    out.emplace_back(BLOOM_EL_TXID, 0, Bytes(tx.GetHash().begin(), tx.GetHash().end()));
    auto pushes = [&](const CScript& s, int kind, int index) {
        CScript::const_iterator pc = s.begin();
        Bytes data;
        while (pc < s.end()) {
            opcodetype op;
            if (!s.GetOp(pc, op, data)) break;
            if (!data.empty()) out.emplace_back(kind, index, data);
        }
    };
    for (size_t i = 0; i < tx.vout.size(); i++) pushes(tx.vout[i].scriptPubKey, BLOOM_EL_OUT_PUSH, (int)i);
    for (size_t i = 0; i < tx.vin.size(); i++) {
        out.emplace_back(BLOOM_EL_PREVOUT, (int)i, SerializeToBytes(tx.vin[i].prevout));
        pushes(tx.vin[i].scriptSig, BLOOM_EL_IN_PUSH, (int)i);
    }
    return out;
}

// the scan against the loop: verdicts and filter bytes
BloomScanInfo CheckScan(const std::vector<CTransactionRef>& txs, const CBloomFilter& f, std::vector<bool>* verdicts = nullptr,
                        bool allowGpu = false) {
    CBloomFilter ref = f, got = f;
    std::vector<bool> want;
    for (const auto& tx : txs) want.push_back(ref.IsRelevantAndUpdate(*tx));
    BloomScanInfo info;
    const std::vector<bool> have = BloomScanTransactions(txs, got, allowGpu, &info);
    CHECK(have == want);
    CHECK_EQ(SerHex(got), SerHex(ref));
    if (verdicts) *verdicts = have;
    return info;
}

} // namespace

TEST_CASE(bloomscan_tests, extract_standard_outputs) {
    std::mt19937 rng(1);
    const Bytes h1 = RandBytes(rng, 20), h2 = RandBytes(rng, 20), pk = FakePubKey(rng), m1 = FakePubKey(rng),
                m2 = FakePubKey(rng), d1 = RandBytes(rng, 4), d2 = RandBytes(rng, 40), sig = RandBytes(rng, 71),
                spub = FakePubKey(rng);
    const COutPoint prev(RandHash(rng), 7);
    const CTransactionRef tx = Tx({{prev, SigScript(sig, spub)}},
                                  {P2PKH(h1), P2PK(pk), Multisig1of2(m1, m2), P2SH(h2), CScript() << OP_RETURN << d1 << d2});
    Bytes op(prev.hash.begin(), prev.hash.end());
    op.insert(op.end(), {7, 0, 0, 0});
    const std::vector<El> want = {
        El(BLOOM_EL_TXID, 0, Bytes(tx->GetHash().begin(), tx->GetHash().end())),
        El(BLOOM_EL_OUT_PUSH, 0, h1),
        El(BLOOM_EL_OUT_PUSH, 1, pk),
        El(BLOOM_EL_OUT_PUSH, 2, m1),
        El(BLOOM_EL_OUT_PUSH, 2, m2),
        El(BLOOM_EL_OUT_PUSH, 3, h2),
        El(BLOOM_EL_OUT_PUSH, 4, d1),
        El(BLOOM_EL_OUT_PUSH, 4, d2),
        El(BLOOM_EL_PREVOUT, 0, op),
        El(BLOOM_EL_IN_PUSH, 0, sig),
        El(BLOOM_EL_IN_PUSH, 0, spub),
    };
    CHECK(Extract(tx) == want);
    CHECK(ModelExtract(*tx) == want);
}

TEST_CASE(bloomscan_tests, extract_small_ints_and_empty_pushes) {
    std::mt19937 rng(2);
    CScript s;
    s << OP_0 << OP_1NEGATE;
    for (int op = OP_1; op <= OP_16; op++) s << (opcodetype)op;
    Bytes raw(s.begin(), s.end());
    raw.insert(raw.end(), {OP_PUSHDATA1, 0});          // empty pushes in each encoding
    raw.insert(raw.end(), {OP_PUSHDATA2, 0, 0});
    raw.insert(raw.end(), {OP_PUSHDATA4, 0, 0, 0, 0});
    raw.insert(raw.end(), {1, 0x2a});                  // and one real byte after them
    const CTransactionRef tx = Tx({{COutPoint(RandHash(rng), 0), CScript()}}, {RawScript(raw)});
    const std::vector<El> got = Extract(tx);
    REQUIRE(got.size() == 3);
    CHECK(got[1] == El(BLOOM_EL_OUT_PUSH, 0, Bytes{0x2a}));
    CHECK_EQ(std::get<0>(got[2]), (int)BLOOM_EL_PREVOUT);
    CHECK(got == ModelExtract(*tx));
}

TEST_CASE(bloomscan_tests, extract_pushdata_forms) {
    std::mt19937 rng(3);
    const Bytes a = RandBytes(rng, 75), b = RandBytes(rng, 76), c = RandBytes(rng, 255), d = RandBytes(rng, 256),
                e = RandBytes(rng, 3000), f = RandBytes(rng, 5);
    Bytes raw;
    raw.push_back(75);
    raw.insert(raw.end(), a.begin(), a.end());
    raw.insert(raw.end(), {OP_PUSHDATA1, 76});
    raw.insert(raw.end(), b.begin(), b.end());
    raw.insert(raw.end(), {OP_PUSHDATA1, 255});
    raw.insert(raw.end(), c.begin(), c.end());
    raw.insert(raw.end(), {OP_PUSHDATA2, 0x00, 0x01});
    raw.insert(raw.end(), d.begin(), d.end());
    raw.insert(raw.end(), {OP_PUSHDATA2, 0xb8, 0x0b});
    raw.insert(raw.end(), e.begin(), e.end());
    raw.insert(raw.end(), {OP_PUSHDATA4, 5, 0, 0, 0});
    raw.insert(raw.end(), f.begin(), f.end());
    const CTransactionRef tx = Tx({{COutPoint(RandHash(rng), 1), RawScript(raw)}}, {RawScript(raw)});
    const std::vector<El> got = Extract(tx);
    REQUIRE(got.size() == 14);
    const Bytes* want[6] = {&a, &b, &c, &d, &e, &f};
    for (int i = 0; i < 6; i++) {
        CHECK(got[1 + i] == El(BLOOM_EL_OUT_PUSH, 0, *want[i]));
        CHECK(got[8 + i] == El(BLOOM_EL_IN_PUSH, 0, *want[i]));
    }
    CHECK(got == ModelExtract(*tx));
}

TEST_CASE(bloomscan_tests, extract_truncated_push_and_coinbase) {
    std::mt19937 rng(4);
    const Bytes h = RandBytes(rng, 20);
    // output 0: a good push, then a push of 5 with 2 bytes left, then nothing more of this script;
    // output 1 is read as usual. PUSHDATA2 with one length byte and PUSHDATA4 with three fail too.
    const CTransactionRef tx = Tx({{COutPoint(RandHash(rng), 0), RawScript({2, 0xaa, 0xbb, OP_PUSHDATA2, 0xff})},
                                   {COutPoint(RandHash(rng), 1), RawScript({OP_PUSHDATA4, 1, 0, 0})},
                                   {COutPoint(RandHash(rng), 2), RawScript({OP_PUSHDATA1})}},
                                  {RawScript({2, 0x01, 0x02, 5, 0x03, 0x04}), P2PKH(h)});
    const std::vector<El> got = Extract(tx);
    REQUIRE(got.size() == 7);
    CHECK(got[1] == El(BLOOM_EL_OUT_PUSH, 0, Bytes{0x01, 0x02}));
    CHECK(got[2] == El(BLOOM_EL_OUT_PUSH, 1, h));
    CHECK_EQ(std::get<0>(got[3]), (int)BLOOM_EL_PREVOUT);
    CHECK(got[4] == El(BLOOM_EL_IN_PUSH, 0, Bytes{0xaa, 0xbb}));
    CHECK(got[5] == El(BLOOM_EL_PREVOUT, 1, std::get<2>(got[5])));
    CHECK(got[6] == El(BLOOM_EL_PREVOUT, 2, std::get<2>(got[6])));
    CHECK(got == ModelExtract(*tx));

    // a coinbase: the null prevout is an element like any other, its scriptSig (height push, then
    // bytes that are no script) gives what parses
    const CTransactionRef cb = Tx({{COutPoint(), RawScript({3, 0x10, 0x27, 0x00, 0x4b, 0x01})}}, {P2PKH(h)});
    REQUIRE(cb->IsCoinBase());
    Bytes nullop(32, 0);
    nullop.insert(nullop.end(), {0xff, 0xff, 0xff, 0xff});
    const std::vector<El> c = Extract(cb);
    REQUIRE(c.size() == 4);
    CHECK(c[2] == El(BLOOM_EL_PREVOUT, 0, nullop));
    CHECK(c[3] == El(BLOOM_EL_IN_PUSH, 0, Bytes{0x10, 0x27, 0x00}));
    CHECK(c == ModelExtract(*cb));
}

TEST_CASE(bloomscan_tests, extract_random_scripts_like_getop) {
    std::mt19937 rng(5);
    std::vector<CTransactionRef> txs;
    for (int i = 0; i < 400; i++) {
        // bytes biased towards push opcodes, so that pushes nest, truncate and run on
        auto script = [&]() {
            Bytes b = RandBytes(rng, rng() % 40);
            for (auto& c : b)
                if (rng() % 3 == 0) c = (unsigned char)(rng() % 0x50);
            return RawScript(b);
        };
        txs.push_back(Tx({{COutPoint(RandHash(rng), i), script()}, {COutPoint(RandHash(rng), 0), script()}},
                         {script(), script(), script()}));
    }
    const std::vector<BloomElement> all = BloomExtractElements(txs);
    size_t at = 0;
    for (size_t t = 0; t < txs.size(); t++)
        for (const El& e : ModelExtract(*txs[t])) {
            REQUIRE(at < all.size());
            CHECK_EQ(all[at].tx, (uint32_t)t);
            CHECK(El((int)all[at].kind, (int)all[at].index, all[at].data) == e);
            at++;
        }
    CHECK_EQ(at, all.size());
}

TEST_CASE(bloomscan_tests, scan_update_none) {
    std::mt19937 rng(10);
    std::vector<CTransactionRef> txs;
    std::vector<Bytes> hashes;
    for (int i = 0; i < 40; i++) {
        hashes.push_back(RandBytes(rng, 20));
        txs.push_back(Tx({{COutPoint(RandHash(rng), i), SigScript(RandBytes(rng, 71), FakePubKey(rng))}},
                         {P2PKH(hashes.back()), P2PKH(RandBytes(rng, 20))}));
    }
    CBloomFilter f(20, 0.0001, 77, BLOOM_UPDATE_NONE);
    f.insert(hashes[3]);
    f.insert(hashes[17]);
    f.insert(txs[5]->GetHash());
    f.insert(txs[9]->vin[0].prevout);
    {
        const CScript& sig = txs[21]->vin[0].scriptSig; // its second push, the key
        f.insert(Bytes(sig.end() - 33, sig.end()));
    }
    // a transaction that spends output 0 of the one paying hashes[3]: no insert, no match
    txs.push_back(Tx({{COutPoint(txs[3]->GetHash(), 0), CScript()}}, {P2PKH(RandBytes(rng, 20))}));
    const std::string before = SerHex(f);
    std::vector<bool> v;
    const BloomScanInfo info = CheckScan(txs, f, &v);
    for (size_t i = 0; i < v.size(); i++) CHECK_EQ((bool)v[i], i == 3 || i == 17 || i == 5 || i == 9 || i == 21);
    CHECK_EQ(info.rounds, (size_t)1);
    CHECK_EQ(info.cpuReruns, (size_t)2);
    CHECK(!info.usedGpu);
    CBloomFilter g = f;
    BloomScanTransactions(txs, g, false);
    CHECK_EQ(SerHex(g), before);
}

TEST_CASE(bloomscan_tests, scan_update_all_chain_and_reversed) {
    std::mt19937 rng(11);
    const Bytes watched = RandBytes(rng, 20);
    const CTransactionRef a = Tx({{COutPoint(RandHash(rng), 0), CScript()}}, {P2PKH(watched)});
    const CTransactionRef b = Tx({{COutPoint(a->GetHash(), 0), CScript()}}, {P2PKH(RandBytes(rng, 20))});
    const CTransactionRef c = Tx({{COutPoint(b->GetHash(), 0), CScript()}}, {P2PKH(RandBytes(rng, 20))});
    CBloomFilter f(10, 0.000001, 5, BLOOM_UPDATE_ALL);
    f.insert(watched);
    std::vector<bool> v;
    BloomScanInfo info = CheckScan({a, b, c}, f, &v);
    CHECK(v == std::vector<bool>({true, true, false}));
    CHECK(info.rounds >= 2); // B matches only through A's insert: a single pass reports it 0
    // B before A: the outpoint A inserts must not reach back
    info = CheckScan({b, a}, f, &v);
    CHECK(v == std::vector<bool>({false, true}));
}

TEST_CASE(bloomscan_tests, scan_update_p2pubkey_only) {
    std::mt19937 rng(12);
    const Bytes h = RandBytes(rng, 20), pk = FakePubKey(rng), m1 = FakePubKey(rng), m2 = FakePubKey(rng);
    const CTransactionRef tPkh = Tx({{COutPoint(RandHash(rng), 0), CScript()}}, {P2PKH(h)});
    const CTransactionRef tPk = Tx({{COutPoint(RandHash(rng), 1), CScript()}}, {P2PK(pk)});
    const CTransactionRef tMs = Tx({{COutPoint(RandHash(rng), 2), CScript()}}, {P2PKH(RandBytes(rng, 20)), Multisig1of2(m1, m2)});
    auto spend = [&](const CTransactionRef& t, uint32_t n) {
        return Tx({{COutPoint(t->GetHash(), n), CScript()}}, {P2PKH(RandBytes(rng, 20))});
    };
    CBloomFilter f(10, 0.000001, 9, BLOOM_UPDATE_P2PUBKEY_ONLY);
    f.insert(h);
    f.insert(pk);
    f.insert(m2);
    std::vector<bool> v;
    CheckScan({tPkh, spend(tPkh, 0), tPk, spend(tPk, 0), tMs, spend(tMs, 1), spend(tMs, 0)}, f, &v);
    CHECK(v == std::vector<bool>({true, false, true, true, true, true, false}));
}

TEST_CASE(bloomscan_tests, scan_same_transaction_effect) {
    // 2 bytes, 2 hash functions: look for a transaction whose output 1 does not match the filter
    // as loaded but does once the outpoint of its matching output 0 went in
    std::mt19937 rng(13);
    const Bytes watched = RandBytes(rng, 20);
    int found = -1;
    for (int attempt = 0; attempt < 1000 && found < 0; attempt++) {
        CBloomFilter f = MakeFilter(Bytes(2, 0), 2, (unsigned)attempt, BLOOM_UPDATE_ALL);
        f.insert(watched);
        const Bytes other = RandBytes(rng, 20);
        const CTransactionRef tx = Tx({{COutPoint(RandHash(rng), 0), CScript()}}, {P2PKH(watched), P2PKH(other)});
        if (f.contains(other) || f.contains(tx->GetHash())) continue;
        CBloomFilter g = f;
        g.insert(COutPoint(tx->GetHash(), 0));
        if (!g.contains(other)) continue;
        found = attempt;
        // the loop inserts (tx, 1) as well, so a transaction spending it matches
        const CTransactionRef spend1 = Tx({{COutPoint(tx->GetHash(), 1), CScript()}}, {P2PKH(RandBytes(rng, 20))});
        CBloomFilter ref = f;
        CHECK(ref.IsRelevantAndUpdate(*tx));
        CHECK(ref.contains(COutPoint(tx->GetHash(), 1)));
        CheckScan({tx, spend1}, f);
    }
    CHECK(found >= 0);
}

TEST_CASE(bloomscan_tests, scan_filter_edge_cases) {
    std::mt19937 rng(14);
    std::vector<CTransactionRef> txs;
    for (int i = 0; i < 20; i++)
        txs.push_back(Tx({{COutPoint(RandHash(rng), i), SigScript(RandBytes(rng, 72), FakePubKey(rng))}}, {P2PKH(RandBytes(rng, 20))}));
    std::vector<bool> v;
    BloomScanInfo info = CheckScan(txs, MakeFilter(Bytes(50, 0xff), 5, 1, BLOOM_UPDATE_ALL), &v);
    CHECK(v == std::vector<bool>(20, true));
    CHECK_EQ(info.rounds, (size_t)0);
    info = CheckScan(txs, MakeFilter(Bytes(50, 0), 5, 1, BLOOM_UPDATE_ALL), &v);
    CHECK(v == std::vector<bool>(20, false));
    CHECK_EQ(info.rounds, (size_t)0);
    CheckScan(txs, MakeFilter(Bytes(), 5, 1, BLOOM_UPDATE_ALL), &v); // full and empty at once: full wins
    CHECK(v == std::vector<bool>(20, true));
    CheckScan(txs, CBloomFilter(), &v);
    CHECK(v == std::vector<bool>(20, true));
    // no hash functions: contains() holds for everything; past the protocol's limits: the loop
    CheckScan(txs, MakeFilter(Bytes(8, 0x10), 0, 1, BLOOM_UPDATE_ALL), &v);
    CHECK(v == std::vector<bool>(20, true));
    CheckScan(txs, MakeFilter(Bytes(8, 0x5a), 51, 1, BLOOM_UPDATE_ALL));
    CheckScan(txs, MakeFilter(Bytes(36001, 0x01), 3, 1, BLOOM_UPDATE_NONE));
    CheckScan({}, MakeFilter(Bytes(8, 0x5a), 3, 1, BLOOM_UPDATE_ALL));
    // a one-byte filter, half set, 50 functions
    CheckScan(txs, MakeFilter(Bytes(1, 0x0f), 50, 3, BLOOM_UPDATE_ALL));
}

static std::vector<CTransactionRef> RandomBlock(std::mt19937& rng, int ntx, std::vector<Bytes>& keyHashes) {
    std::vector<CTransactionRef> txs;
    for (int i = 0; i < ntx; i++) {
        // a third spend an output of an earlier transaction of the list
        COutPoint prev(RandHash(rng), rng() % 4);
        if (i && rng() % 3 == 0) prev = COutPoint(txs[rng() % i]->GetHash(), rng() % 2);
        keyHashes.push_back(RandBytes(rng, 20));
        txs.push_back(Tx({{prev, SigScript(RandBytes(rng, 71 + rng() % 2), FakePubKey(rng))}},
                         {P2PKH(keyHashes.back()), rng() % 8 ? P2PKH(RandBytes(rng, 20)) : P2PK(FakePubKey(rng))}));
    }
    return txs;
}

TEST_CASE(bloomscan_tests, scan_random_block) {
    std::mt19937 rng(15);
    std::vector<Bytes> keyHashes;
    const std::vector<CTransactionRef> txs = RandomBlock(rng, 3000, keyHashes);
    for (unsigned char flags : {BLOOM_UPDATE_NONE, BLOOM_UPDATE_ALL, BLOOM_UPDATE_P2PUBKEY_ONLY}) {
        CBloomFilter f(200, 0.001, 4242, flags);
        for (int i = 0; i < 30; i++) f.insert(keyHashes[(i * 97) % keyHashes.size()]);
        std::vector<bool> v;
        const BloomScanInfo info = CheckScan(txs, f, &v);
        CHECK(std::count(v.begin(), v.end(), true) >= 30);
        CHECK(std::count(v.begin(), v.end(), false) >= 1000);
        CHECK(info.elements >= 3000u * 6);
        CHECK(info.rounds >= 1 && info.rounds <= 8);
    }
    // few matches: every insert gets its own pass and the passes do not run out
    CBloomFilter f(200, 0.001, 4243, BLOOM_UPDATE_ALL);
    for (int i = 0; i < 3; i++) f.insert(keyHashes[1000 * i + 500]);
    const BloomScanInfo info = CheckScan(txs, f);
    CHECK(info.rounds >= 4 && info.rounds <= 8);
}

TEST_CASE(bloomscan_tests, scan_fault_injection_falls_back) {
    std::mt19937 rng(16);
    std::vector<Bytes> keyHashes;
    const std::vector<CTransactionRef> txs = RandomBlock(rng, 300, keyHashes);
    CBloomFilter f(50, 0.001, 1, BLOOM_UPDATE_ALL);
    for (int i = 0; i < 5; i++) f.insert(keyHashes[i * 50]);
    ResetBloomScanFailures();
    const uint64_t before = GetBloomScanStats().gpu_failures;
    SetGpuFaultInjection(true);
    const BloomScanInfo info = CheckScan(txs, f, nullptr, /*allowGpu=*/true);
    SetGpuFaultInjection(false);
    CHECK(!info.usedGpu);
    CHECK_EQ(GetBloomScanStats().gpu_failures, before + 1);
    ResetBloomScanFailures();
}

TEST_CASE(bloomscan_tests, merkle_block_from_verdicts) {
    std::mt19937 rng(17);
    std::vector<Bytes> keyHashes;
    CBlock block;
    block.nVersion = 4;
    block.nBits = 0x207fffff;
    block.vtx = RandomBlock(rng, 33, keyHashes);
    CBloomFilter f(20, 0.0001, 3, BLOOM_UPDATE_ALL);
    f.insert(keyHashes[4]);
    f.insert(keyHashes[30]);
    CBloomFilter f1 = f, f2 = f;
    const CMerkleBlock want(block, f1);
    const CMerkleBlock got(block, BloomScanTransactions(block.vtx, f2, false));
    CHECK(got.vMatchedTxn == want.vMatchedTxn);
    CHECK(SerializeToBytes(got) == SerializeToBytes(want));
    CHECK_EQ(SerHex(f2), SerHex(f1));
}
