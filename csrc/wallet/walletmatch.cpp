#include "wallet/walletmatch.h"

#include "crypto/hashes.h"
#include "keys/key.h"

#include <stdexcept>

namespace bcp {

namespace {
uint32_t SlotsFor(size_t entries) {
    size_t s = wm::WM_MIN_SLOTS;
    while (s < 2 * entries) s <<= 1;
    if (s > ((size_t)1 << 28)) throw std::length_error("wallet match table: more than 2^27 entries");
    return (uint32_t)s;
}
struct HostHash160 {
    void operator()(const uint8_t* p, uint32_t len, uint32_t id[5]) const {
        unsigned char h[20];
        Hash160(p, len, h);
        for (int w = 0; w < 5; ++w) id[w] = wm::LoadLE32(h + 4 * w);
    }
};
} // namespace

WalletMatchTable::WalletMatchTable() {
    unsigned char salt[16];
    GetRandBytes(salt, sizeof(salt));
    k0 = wm::LoadLE64(salt);
    k1 = wm::LoadLE64(salt + 8);
    slots.assign(wm::WM_MIN_SLOTS, 0);
}
WalletMatchTable::WalletMatchTable(uint64_t k0In, uint64_t k1In) : k0(k0In), k1(k1In) { slots.assign(wm::WM_MIN_SLOTS, 0); }

wm::TableView WalletMatchTable::View() const {
    wm::TableView v;
    v.slots = slots.data();
    v.mask = (uint32_t)slots.size() - 1;
    v.k0 = k0;
    v.k1 = k1;
    v.hasWatch = HasWatch() ? 1 : 0;
    return v;
}

uint64_t WalletMatchTable::FingerprintOf(const unsigned char* p, size_t len) const {
    return wm::Fingerprint(k0, k1, p, (uint32_t)len);
}

// Within WM_MAX_PROBE slots of the entry's home: true and *at = its slot when placed, true and
// *at = UINT32_MAX when it is there already, false when the run is full.
bool WalletMatchTable::Place(std::vector<uint64_t>& into, uint64_t entry, uint32_t* at) const {
    const uint32_t mask = (uint32_t)into.size() - 1;
    uint32_t s = wm::HomeOf(entry, mask); // the entry keeps the fingerprint's high half
    for (uint32_t i = 0; i < wm::WM_MAX_PROBE; ++i) {
        if (into[s] == entry) {
            *at = UINT32_MAX;
            return true;
        }
        if (into[s] == 0) {
            into[s] = entry;
            *at = s;
            return true;
        }
        s = (s + 1) & mask;
    }
    return false;
}

void WalletMatchTable::Grow(size_t minSlots) {
    for (size_t want = minSlots;; want <<= 1) {
        if (want > ((size_t)1 << 28)) throw std::length_error("wallet match table: more than 2^28 slots");
        std::vector<uint64_t> next(want, 0);
        bool ok = true;
        uint32_t at;
        for (uint64_t e : slots)
            if (e && !Place(next, e, &at)) {
                ok = false;
                break;
            }
        if (!ok) continue;
        slots.swap(next);
        layout++;
        dirty.clear();
        return;
    }
}

void WalletMatchTable::Reserve(size_t entries) {
    const uint32_t want = SlotsFor(entries);
    if (want > slots.size()) Grow(want);
}

bool WalletMatchTable::Insert(wm::Tag tag, const unsigned char* p, size_t len) {
    if (len > 0xFFFFFFFFu) throw std::length_error("wallet match table: member longer than 4 GiB");
    const uint64_t entry = wm::EntryOf(FingerprintOf(p, len), tag);
    if (2 * (nEntries + 1) > slots.size()) Grow(slots.size() * 2);
    uint32_t at;
    while (!Place(slots, entry, &at)) Grow(slots.size() * 2);
    if (at == UINT32_MAX) return false;
    dirty.push_back(at);
    nEntries++;
    count[tag]++;
    return true;
}

bool WalletMatchTable::Contains(wm::Tag tag, const unsigned char* p, size_t len) const {
    return wm::Probe(slots.data(), (uint32_t)slots.size() - 1, FingerprintOf(p, len), tag);
}

std::vector<uint32_t> WalletMatchTable::TakeDirty() {
    std::vector<uint32_t> d;
    d.swap(dirty);
    return d;
}

void WalletMatchCpu(const WalletMatchTable& table, uint32_t kindMask, const uint8_t* kinds, const unsigned char* blob,
                    size_t blobBytes, const uint32_t* offs, const uint32_t* lens, size_t n, uint8_t* flags) {
    const wm::TableView t = table.View();
    for (size_t i = 0; i < n; ++i) {
        if (offs[i] > blobBytes || lens[i] > blobBytes - offs[i]) {
            flags[i] = wm::NOT_READ;
            continue;
        }
        flags[i] = wm::MatchItem(t, kindMask, kinds[i], blob + offs[i], lens[i], HostHash160());
    }
}

} // namespace bcp
