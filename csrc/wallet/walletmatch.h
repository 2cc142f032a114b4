// The host side of wallet matching: the match table's builder and the CPU twin of
// wallet_match_kernel (csrc/kernels/wallet_match.hip). Both run the item code of
// kernels/wallet_match.h, so the twin's flags equal the kernel's byte for byte, false positives
// of the 61-bit fingerprints included. No HIP here: this is what a host without a device runs.
#pragma once
#include "kernels/wallet_match.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bcp {

// Open addressing over salted fingerprints as kernels/wallet_match.h lays it out. Members are
// only ever added. The salt is drawn at random per table (or given, for tests), so outputs
// crafted against one node's table do not pile into a probe chain of another's, nor of the
// same node's next table.
class WalletMatchTable {
public:
    WalletMatchTable(); // a fresh random salt
    WalletMatchTable(uint64_t k0, uint64_t k1);
    void Reserve(size_t entries); // room for this many at load factor 1/2
    // false when the member was there already
    bool Insert(wm::Tag tag, const unsigned char* p, size_t len);
    bool Contains(wm::Tag tag, const unsigned char* p, size_t len) const;
    uint64_t FingerprintOf(const unsigned char* p, size_t len) const;
    size_t Entries() const { return nEntries; }
    size_t Count(wm::Tag tag) const { return count[tag]; }
    uint32_t Slots() const { return (uint32_t)slots.size(); }
    const uint64_t* Data() const { return slots.data(); }
    uint64_t K0() const { return k0; }
    uint64_t K1() const { return k1; }
    bool HasWatch() const { return count[wm::TAG_W] != 0; }
    wm::TableView View() const;
    // For uploads: Layout() changes whenever the table was rebuilt at another size (every slot
    // may have moved); otherwise TakeDirty() lists the slots written since the last call.
    uint64_t Layout() const { return layout; }
    std::vector<uint32_t> TakeDirty();

private:
    bool Place(std::vector<uint64_t>& into, uint64_t entry, uint32_t* at) const;
    void Grow(size_t minSlots);
    uint64_t k0, k1;
    std::vector<uint64_t> slots;
    size_t nEntries = 0;
    size_t count[4] = {0, 0, 0, 0};
    uint64_t layout = 0;
    std::vector<uint32_t> dirty;
};

// flags[i] = wm::MatchItem of item i = (kinds[i], blob[offs[i] .. offs[i] + lens[i])), wm::NOT_READ
// for one that reaches past the blob: what wallet_match_kernel writes.
void WalletMatchCpu(const WalletMatchTable& table, uint32_t kindMask, const uint8_t* kinds, const unsigned char* blob,
                    size_t blobBytes, const uint32_t* offs, const uint32_t* lens, size_t n, uint8_t* flags);

} // namespace bcp
