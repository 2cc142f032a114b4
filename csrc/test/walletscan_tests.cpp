// The batched wallet scan (csrc/wallet/walletscan.cpp) against the loop of
// CWallet::AddToWalletIfInvolvingMe, with the match passes on the host twin of
// wallet_match_kernel: the no-op argument of wallet/walletscan.h case by case, growth inside a
// list, conflict marks through a real chainstate, the table kept between scans, and the fallback
// after an injected device error. The device passes are covered by tests/test_wallet_scan_gpu.py.
#include "test/unittest.h"

#include "crypto/hashes.h"
#include "node/validation.h"
#include "script/standard.h"
#include "util/util.h"
#include "wallet/wallet.h"
#include "wallet/walletmatch.h"
#include "wallet/walletscan.h"

#include <map>
#include <random>
#include <tuple>

namespace bcp {
namespace {

typedef std::vector<unsigned char> Bytes;

Bytes RandBytes(std::mt19937& rng, size_t n) {
    Bytes b(n);
    for (auto& c : b) c = (unsigned char)rng();
    return b;
}
CPubKey FakePubKey(std::mt19937& rng, bool compressed = true) {
    Bytes b = RandBytes(rng, compressed ? 33 : 65);
    b[0] = compressed ? 2 : 4; // IsMine hashes a key and never checks the point
    return CPubKey(b.begin(), b.end());
}
Bytes IdBytes(const CPubKey& p) {
    const CKeyID id = p.GetID();
    return Bytes(id.begin(), id.end());
}
CScript P2PKH(const Bytes& h) { return CScript() << OP_DUP << OP_HASH160 << h << OP_EQUALVERIFY << OP_CHECKSIG; }
CScript Raw(const Bytes& b) { return CScript(b.begin(), b.end()); }

CTransactionRef MakeTx(const std::vector<COutPoint>& ins, const std::vector<CScript>& outs) {
    CMutableTransaction m;
    for (const COutPoint& o : ins) m.vin.push_back(CTxIn(o));
    for (size_t i = 0; i < outs.size(); i++) m.vout.push_back(CTxOut(1000 + i, outs[i]));
    return MakeTransactionRef(std::move(m));
}
COutPoint RandOutPoint(std::mt19937& rng) {
    const Bytes h = RandBytes(rng, 32);
    uint256 u;
    memcpy(u.begin(), h.data(), 32);
    return COutPoint(u, rng() % 4);
}
CTransactionRef Fresh(std::mt19937& rng, const std::vector<CScript>& outs) { return MakeTx({RandOutPoint(rng)}, outs); }

// what a scan may change of a wallet
typedef std::tuple<std::map<uint256, std::pair<uint256, int>>, std::multimap<COutPoint, uint256>> State;
State StateOf(CWallet& w) {
    WalletLock l(w);
    std::map<uint256, std::pair<uint256, int>> txs;
    for (const auto& kv : w.mapWallet) txs[kv.first] = {kv.second.hashBlock, kv.second.nIndex};
    return State(txs, w.TxSpends());
}

// Two wallets filled alike: one runs the loop, the other the scan. Returns the scan's info.
struct Pair {
    CWallet loop{"loop", "", true}, scan{"scan", "", true};
    CKey dummy;
    Pair() { dummy.MakeNewKey(true); }
    void Key(const CPubKey& p) {
        loop.LoadKey(dummy, p);
        scan.LoadKey(dummy, p);
    }
    void Script(const CScript& s) {
        loop.AddCScript(s);
        scan.AddCScript(s);
    }
    void Watch(const CScript& s) {
        loop.AddWatchOnly(s);
        scan.AddWatchOnly(s);
    }
    void Have(const CTransactionRef& tx) {
        loop.AddToWallet(CWalletTx(&loop, tx), false);
        scan.AddToWallet(CWalletTx(&scan, tx), false);
    }
    WalletScanInfo Check(const std::vector<CTransactionRef>& txs, const CBlockIndex* pindex, bool fUpdate,
                         std::vector<bool>* verdicts = nullptr, bool allowGpu = false) {
        std::vector<bool> want;
        for (size_t i = 0; i < txs.size(); i++) want.push_back(loop.AddToWalletIfInvolvingMe(txs[i], pindex, (int)i, fUpdate));
        WalletScanInfo info;
        const std::vector<bool> got = WalletScanTransactions(scan, txs, pindex, fUpdate, allowGpu, &info);
        CHECK(got == want);
        CHECK(StateOf(scan) == StateOf(loop));
        if (verdicts) *verdicts = got;
        return info;
    }
};

const uint256 kBlock = uint256S("00000000000000000000000000000000000000000000000000000000000b10c0");
CBlockIndex FakeIndex() {
    CBlockIndex i;
    i.phashBlock = &kBlock;
    return i;
}

} // namespace

TEST_CASE(walletscan_tests, table_insert_grow_and_dirty) {
    WalletMatchTable t(1, 2);
    CHECK_EQ(t.Slots(), 8u);
    std::mt19937 rng(1);
    std::vector<Bytes> members;
    for (int i = 0; i < 1000; i++) members.push_back(RandBytes(rng, 20));
    const uint64_t layout0 = t.Layout();
    for (int i = 0; i < 4; i++) CHECK(t.Insert(wm::TAG_K, members[i].data(), 20));
    CHECK_EQ(t.Slots(), 8u); // load 1/2 exactly
    CHECK_EQ(t.Layout(), layout0);
    CHECK_EQ(t.TakeDirty().size(), (size_t)4);
    CHECK(!t.Insert(wm::TAG_K, members[0].data(), 20)); // there already
    CHECK(t.TakeDirty().empty());
    CHECK(t.Insert(wm::TAG_T, members[0].data(), 20)); // another set: another member
    CHECK(t.Layout() != layout0 && t.Slots() == 16u);
    CHECK(t.TakeDirty().size() == 1); // the rebuild moved everything: only what came after it is listed
    for (int i = 4; i < 1000; i++) t.Insert(wm::TAG_K, members[i].data(), 20);
    CHECK_EQ(t.Entries(), (size_t)1001);
    CHECK(t.Slots() >= 2048u && (t.Slots() & (t.Slots() - 1)) == 0);
    for (const Bytes& m : members) CHECK(t.Contains(wm::TAG_K, m.data(), 20));
    CHECK(!t.Contains(wm::TAG_S, members[0].data(), 20) && t.Contains(wm::TAG_T, members[0].data(), 20));
    CHECK(!t.HasWatch());
    t.Insert(wm::TAG_W, nullptr, 0); // the empty script
    CHECK(t.HasWatch() && t.Contains(wm::TAG_W, nullptr, 0));
    // every entry within WM_MAX_PROBE slots of its home, none empty in between
    const uint32_t mask = t.Slots() - 1;
    for (uint32_t s = 0; s <= mask; s++) {
        const uint64_t e = t.Data()[s];
        if (!e) continue;
        const uint32_t home = wm::HomeOf(e, mask);
        CHECK(((s - home) & mask) < wm::WM_MAX_PROBE);
        for (uint32_t at = home; at != s; at = (at + 1) & mask) CHECK(t.Data()[at] != 0);
    }
}

TEST_CASE(walletscan_tests, device_ripemd160_code_on_the_host) {
    std::mt19937 rng(2);
    for (int i = 0; i < 100; i++) {
        const Bytes m = RandBytes(rng, 32);
        uint32_t d[8], o[5];
        for (int w = 0; w < 8; w++) d[w] = wm::LoadLE32(m.data() + 4 * w);
        wm::Ripemd160Of32(d, o);
        unsigned char want[20];
        CRIPEMD160().Write(m.data(), 32).Finalize(want);
        for (int w = 0; w < 5; w++) CHECK_EQ(o[w], wm::LoadLE32(want + 4 * w));
    }
}

// Each reason AddToWalletIfInvolvingMe can have to act, one transaction each, and the same
// transaction against a wallet without that reason: flagged and found, or not even rerun.
TEST_CASE(walletscan_tests, no_op_argument_case_by_case) {
    std::mt19937 rng(3);
    const CPubKey p1 = FakePubKey(rng), p2 = FakePubKey(rng, false), p3 = FakePubKey(rng), other = FakePubKey(rng);
    const CScript redeem = GetScriptForRawPubKey(p3), watch = Raw({0x51, 0x75, 0x51});
    const CBlockIndex index = FakeIndex();
    Bytes h1 = IdBytes(p1);
    Bytes bad(p1.begin(), p1.end());
    bad[0] = 5; // CPubKey clears it: the id of no bytes
    const CTransactionRef known = Fresh(rng, {P2PKH(h1)});
    const COutPoint knownIn = known->vin[0].prevout;
    struct Case {
        const char* what;
        CTransactionRef tx;
        bool added;
        bool flagged = true;
    };
    const std::vector<Case> cases = {
        {"P2PKH of our key", Fresh(rng, {P2PKH(h1)}), true},
        {"P2PK, compressed", Fresh(rng, {GetScriptForRawPubKey(p1)}), true},
        {"P2PK, uncompressed", Fresh(rng, {GetScriptForRawPubKey(p2)}), true},
        {"P2SH of our script", Fresh(rng, {GetScriptForDestination(CScriptID(redeem))}), true},
        {"bare multisig, every key ours", Fresh(rng, {GetScriptForMultisig(1, {p1, p3})}), true},
        {"bare multisig, one key ours", Fresh(rng, {GetScriptForMultisig(1, {FakePubKey(rng), p1})}), false},
        {"watch-only script", Fresh(rng, {watch}), true},
        {"second output ours", Fresh(rng, {Raw({0x6a}), P2PKH(h1)}), true},
        {"spends a wallet transaction's output that is ours", MakeTx({COutPoint(known->GetHash(), 0)}, {Raw({0x51})}), true},
        {"spends an output the wallet transaction does not have", MakeTx({COutPoint(known->GetHash(), 5)}, {Raw({0x51})}), false},
        {"double-spends a wallet transaction's input", MakeTx({knownIn}, {Raw({0x51})}), false},
        {"the wallet transaction itself", known, true},
        {"ill-formed key before CHECKSIG", Fresh(rng, {CScript() << bad << OP_CHECKSIG}), false, false},
        {"our key hash, then a push that runs past the end", Fresh(rng, {Raw([&] {
                                                                      const CScript k = P2PKH(h1);
                                                                      Bytes s(k.begin(), k.end());
                                                                      s.push_back(0x4c);
                                                                      return s;
                                                                  }())}),
         false},
    };
    for (const Case& c : cases) {
        // with the reason: flagged, and the verdict is the loop's
        Pair with;
        for (const CPubKey& p : {p1, p2, p3}) with.Key(p);
        with.Script(redeem);
        with.Watch(watch);
        with.Have(known);
        std::vector<bool> v;
        const WalletScanInfo a = with.Check({c.tx}, &index, true, &v);
        CHECK_EQ(v[0], c.added);
        if (a.cpuReruns != (c.flagged ? 1u : 0u)) test::RecordFailure(std::string("flagged or not, against the case: ") + c.what, __FILE__, __LINE__);
        // a wallet of strangers' keys: not even rerun
        Pair without;
        without.Key(other);
        without.Script(GetScriptForRawPubKey(other));
        without.Watch(Raw({0x52}));
        without.Have(Fresh(rng, {Raw({0x51})}));
        const WalletScanInfo b = without.Check({c.tx}, &index, true, &v);
        CHECK(!v[0]);
        if (b.cpuReruns != 0) test::RecordFailure(std::string("rerun without a reason: ") + c.what, __FILE__, __LINE__);
    }
    // a wallet that holds the id of no bytes (it cannot: this is the table's view of such a wallet)
    WalletMatchTable t(7, 8);
    unsigned char idOfNothing[20];
    Hash160(nullptr, 0, idOfNothing);
    t.Insert(wm::TAG_K, idOfNothing, 20);
    const CScript s = CScript() << bad << OP_CHECKSIG;
    const uint8_t kind = wm::ITEM_OUTPUT;
    const uint32_t off = 0, len = (uint32_t)s.size();
    uint8_t flag = 0;
    WalletMatchCpu(t, wm::KIND_MASK_ALL, &kind, s.data(), s.size(), &off, &len, 1, &flag);
    CHECK_EQ((int)flag, (int)wm::HIT_K);
}

TEST_CASE(walletscan_tests, growth_inside_the_list) {
    std::mt19937 rng(4);
    const CPubKey p1 = FakePubKey(rng), p2 = FakePubKey(rng);
    const Bytes h1 = IdBytes(p1), h2 = IdBytes(p2);
    const CBlockIndex index = FakeIndex();
    const CTransactionRef a = Fresh(rng, {P2PKH(h1)});
    const CTransactionRef b = MakeTx({COutPoint(a->GetHash(), 0)}, {P2PKH(h2)});
    const CTransactionRef c = MakeTx({COutPoint(b->GetHash(), 0)}, {Raw({0x51})});
    const CTransactionRef d = Fresh(rng, {Raw({0x51})});
    const CTransactionRef twice = MakeTx({a->vin[0].prevout}, {Raw({0x52})}); // double-spends A's input
    std::vector<bool> v;
    {
        Pair p;
        p.Key(p1);
        p.Key(p2);
        const WalletScanInfo info = p.Check({d, a, d, b, c, twice, d}, &index, true, &v);
        CHECK(v == std::vector<bool>({false, true, false, true, true, false, false}));
        CHECK(info.passes >= 2);
        CHECK_EQ(info.cpuReruns, (size_t)4);
    }
    {
        Pair p; // B before A: A is not in the wallet when B is judged
        p.Key(p1);
        const CTransactionRef b2 = MakeTx({COutPoint(a->GetHash(), 0)}, {Raw({0x51})});
        p.Check({b2, a}, &index, true, &v);
        CHECK(v == std::vector<bool>({false, true}));
    }
    {
        Pair p; // more additions than device passes: the exact sets on the host take over
        p.Key(p1);
        std::vector<CTransactionRef> chain{a};
        for (int i = 0; i < 40; i++) chain.push_back(MakeTx({COutPoint(chain.back()->GetHash(), 0)}, {P2PKH(h1)}));
        chain.push_back(d);
        const WalletScanInfo info = p.Check(chain, &index, true, &v);
        CHECK_EQ(info.passes, (size_t)16);
        CHECK_EQ(info.cpuReruns, (size_t)41);
        CHECK(!v.back() && v[40]);
    }
    {
        Pair p; // fUpdate both ways on a transaction the wallet has
        p.Key(p1);
        p.Have(a);
        p.Check({a, d}, &index, false, &v);
        CHECK(v == std::vector<bool>({false, false}));
        p.Check({a, d}, &index, true, &v);
        CHECK(v == std::vector<bool>({true, false}));
        p.Check({}, &index, true, &v);
        CHECK(v.empty());
    }
}

TEST_CASE(walletscan_tests, table_kept_between_scans) {
    std::mt19937 rng(5);
    const CPubKey p1 = FakePubKey(rng), p2 = FakePubKey(rng);
    const Bytes h1 = IdBytes(p1), h2 = IdBytes(p2);
    const CBlockIndex index = FakeIndex();
    Pair p;
    p.Key(p1);
    const CTransactionRef a = Fresh(rng, {P2PKH(h1)}), forP2 = Fresh(rng, {P2PKH(h2)});
    std::vector<bool> v;
    p.Check({a, forP2}, &index, true, &v);
    CHECK(v == std::vector<bool>({true, false}));
    // what the first scan added is in the table of the second
    const CTransactionRef b = MakeTx({COutPoint(a->GetHash(), 0)}, {Raw({0x51})});
    p.Check({b}, &index, true, &v);
    CHECK(v == std::vector<bool>({true}));
    // a key that arrives between scans is seen by the next one
    p.Key(p2);
    const CTransactionRef again = Fresh(rng, {P2PKH(h2)});
    p.Check({again}, &index, true, &v);
    CHECK(v == std::vector<bool>({true}));
    // a watch-only script removed and another added: the sizes are as before, the table is not
    p.Watch(Raw({0x51, 0x51}));
    p.Check({Fresh(rng, {Raw({0x51, 0x51})})}, &index, true, &v);
    CHECK(v[0]);
    p.loop.RemoveWatchOnly(Raw({0x51, 0x51}));
    p.scan.RemoveWatchOnly(Raw({0x51, 0x51}));
    p.Watch(Raw({0x52, 0x52}));
    p.Check({Fresh(rng, {Raw({0x52, 0x52})}), Fresh(rng, {Raw({0x51, 0x51})})}, &index, true, &v);
    CHECK(v == std::vector<bool>({true, false}));
}

TEST_CASE(walletscan_tests, mark_conflicted_through_a_chainstate) {
    test::TestingSetup setup;
    Chainstate& cs = *setup.node->chainstate;
    std::mt19937 rng(6);
    const CPubKey p1 = FakePubKey(rng);
    const Bytes h1 = IdBytes(p1);
    const CBlockIndex* tip = cs.TipNow();
    REQUIRE(tip != nullptr);
    Pair p;
    p.loop.Attach(&cs, setup.node->mempool.get());
    p.scan.Attach(&cs, setup.node->mempool.get());
    p.Key(p1);
    // an unconfirmed wallet transaction, and its unconfirmed child
    const CTransactionRef parent = Fresh(rng, {P2PKH(h1)});
    const CTransactionRef child = MakeTx({COutPoint(parent->GetHash(), 0)}, {P2PKH(h1)});
    p.Have(parent);
    p.Have(child);
    // the block spends the parent's input otherwise
    const CTransactionRef rival = MakeTx({parent->vin[0].prevout}, {Raw({0x51})});
    std::vector<bool> v;
    const WalletScanInfo info = p.Check({Fresh(rng, {Raw({0x51})}), rival}, tip, true, &v);
    CHECK(v == std::vector<bool>({false, false}));
    CHECK_EQ(info.cpuReruns, (size_t)1);
    for (CWallet* w : {&p.loop, &p.scan}) {
        WalletLock l(*w);
        for (const CTransactionRef& t : {parent, child}) {
            const CWalletTx& wtx = w->mapWallet.at(t->GetHash());
            CHECK_EQ(wtx.nIndex, -1);
            CHECK(wtx.hashBlock == tip->GetBlockHash());
        }
    }
}

TEST_CASE(walletscan_tests, fault_injection_falls_back) {
    std::mt19937 rng(7);
    const CPubKey p1 = FakePubKey(rng);
    const Bytes h1 = IdBytes(p1);
    const CBlockIndex index = FakeIndex();
    std::vector<CTransactionRef> txs;
    for (int i = 0; i < 300; i++) txs.push_back(Fresh(rng, {i % 50 ? Raw({0x51}) : P2PKH(h1)}));
    Pair p;
    p.Key(p1);
    ResetWalletScanFailures();
    const uint64_t before = GetWalletScanStats().gpu_failures;
    SetGpuFaultInjection(true);
    std::vector<bool> v;
    const WalletScanInfo info = p.Check(txs, &index, true, &v, /*allowGpu=*/true);
    CHECK(!info.usedGpu);
    CHECK_EQ(GetWalletScanStats().gpu_failures, before + 1);
    // three in a row close the path: the wallet's callers then keep to the loop
    SetGpuWalletScanThreshold(1);
    CHECK(GpuWalletScanWanted(300));
    p.Check(txs, &index, true, &v, true);
    CHECK(GpuWalletScanWanted(300));
    p.Check(txs, &index, true, &v, true);
    CHECK(!GpuWalletScanWanted(300));
    SetGpuFaultInjection(false);
    SetGpuWalletScanThreshold(DEFAULT_GPU_WALLET_SCAN_THRESHOLD);
    ResetWalletScanFailures();
}

} // namespace bcp
