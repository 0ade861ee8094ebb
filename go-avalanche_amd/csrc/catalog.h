// The Hash catalog of one engine: the caller's 64-bit hashes (avalanche.go:71, `Hash int`) mapped to
// the slots of the engine's target range. The host side (Catalog) is authoritative: hash -> slot,
// slot -> hash, the free slots, and the exact image of the open-addressing table the device probes
// (catalog.hip k_catalog_pack). Pure C++17, no HIP include: host/catalog_test.cpp checks it without
// a GPU. probe() below is the one lookup, compiled for the host and for the device.
//
// Slots here are local: 0 .. n_slots-1 stands for target_begin .. target_end-1 of the engine.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define AVCAT_HD __host__ __device__
#else
#define AVCAT_HD
#endif

namespace avcat {

// One table entry, 16 bytes (one dwordx4 load). The state is a field of its own: every int64 is a
// legal hash (0, -1 and INT64_MIN among them), so no key value can mark an empty entry.
enum : uint32_t { kEmpty = 0u, kUsed = 1u, kTomb = 2u };
struct alignas(16) Entry {
  int64_t key;
  int32_t slot;
  uint32_t state;
};
static_assert(sizeof(Entry) == 16, "table entry");

// splitmix64's finalizer (the update digest's mixer, log_ops.hip): the table index of a key is its
// low bits, so consecutive and strided hashes spread over the table.
AVCAT_HD inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The slot of key in the table image tab (mask + 1 entries, a power of two), or -1. Linear probing:
// an empty entry ends the search, a tombstone does not. The walk is bounded by the table size, so it
// ends on any image; Catalog keeps at least a quarter of the entries empty.
template <typename EntryPtr>
AVCAT_HD inline int32_t probe(EntryPtr tab, uint32_t mask, int64_t key) {
  uint32_t i = (uint32_t)mix64((uint64_t)key) & mask;
  for (uint32_t n = 0; n <= mask; ++n) {
    const Entry e = tab[i];
    if (e.state == kEmpty) return -1;
    if (e.state == kUsed && e.key == key) return e.slot;
    i = (i + 1u) & mask;
  }
  return -1;
}

// Table size for n_slots slots: the power of two that keeps the live entries at or below half of it
// (DESIGN.md "Hash catalog"): an unsuccessful linear probe then reads 2.5 entries on average, and
// with the tombstone bound below (used + tombstones <= 3/4) 8.5 on average at worst.
inline uint32_t table_entries(uint32_t n_slots) {
  uint32_t c = 16u;
  while (c < 2u * n_slots) c <<= 1;
  return c;
}

class Catalog {
 public:
  // (re)start with n_slots free slots and an empty table
  void init(uint32_t n_slots) {
    n_slots_ = n_slots;
    image_.assign(table_entries(n_slots), Entry{0, 0, kEmpty});
    mask_ = (uint32_t)image_.size() - 1u;
    hash_of_.assign(n_slots, 0);
    used_.assign(n_slots, 0);
    free_.assign(((size_t)n_slots + 63) / 64, 0ull);
    for (uint32_t s = 0; s < n_slots; ++s) free_[s >> 6] |= 1ull << (s & 63);
    free_hint_ = 0;
    n_used_ = n_tomb_ = 0;
    rebuilds_ = 0;
    dirty_.clear();
    dirty_all_ = true;
  }
  bool ready() const { return !image_.empty(); }
  uint32_t n_slots() const { return n_slots_; }
  uint32_t n_used() const { return n_used_; }
  uint32_t n_tombstones() const { return n_tomb_; }
  uint64_t rebuilds() const { return rebuilds_; }
  // the table image: what the device copy must equal before its next lookup
  const Entry* image() const { return image_.data(); }
  uint32_t mask() const { return mask_; }
  uint32_t entries() const { return mask_ + 1u; }
  bool slot_used(uint32_t s) const { return used_[s] != 0; }
  int64_t hash_of(uint32_t s) const { return hash_of_[s]; }

  int32_t find(int64_t key) const { return ready() ? probe(image_.data(), mask_, key) : -1; }

  // The slot of key: its own if catalogued, else the lowest free slot (*fresh = true), else -1 with
  // nothing changed.
  int32_t intern(int64_t key, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    const int32_t have = find(key);
    if (have >= 0) return have;
    const int32_t s = lowest_free();
    if (s < 0) return -1;
    free_[(uint32_t)s >> 6] &= ~(1ull << (s & 63));
    hash_of_[(size_t)s] = key;
    used_[(size_t)s] = 1;
    ++n_used_;
    place(key, s);
    if (fresh) *fresh = true;
    return s;
  }

  // Remove key and free its slot; false if it is not catalogued. The entry becomes a tombstone; once
  // the tombstones pass a quarter of the table the image is rebuilt without them.
  bool retire(int64_t key) {
    if (!ready()) return false;
    uint32_t i = (uint32_t)mix64((uint64_t)key) & mask_;
    for (uint32_t n = 0; n <= mask_; ++n, i = (i + 1u) & mask_) {
      Entry& e = image_[i];
      if (e.state == kEmpty) return false;
      if (e.state != kUsed || e.key != key) continue;
      const uint32_t s = (uint32_t)e.slot;
      e.state = kTomb;
      touch(i);
      ++n_tomb_;
      --n_used_;
      used_[s] = 0;
      free_[s >> 6] |= 1ull << (s & 63);
      free_hint_ = free_hint_ < (s >> 6) ? free_hint_ : (s >> 6);
      if (n_tomb_ > entries() / 4u) rebuild();
      return true;
    }
    return false;
  }

  // What changed in the image since the last clear_dirty(): single entries, or all of it (after
  // init, a rebuild, or more single changes than are worth sending one by one).
  bool dirty_all() const { return dirty_all_; }
  const std::vector<uint32_t>& dirty() const { return dirty_; }
  void clear_dirty() {
    dirty_.clear();
    dirty_all_ = false;
  }

 private:
  static constexpr size_t kMaxDirty = 64;

  void touch(uint32_t i) {
    if (dirty_all_) return;
    if (dirty_.size() >= kMaxDirty) {
      dirty_all_ = true;
      dirty_.clear();
      return;
    }
    dirty_.push_back(i);
  }

  // key (not in the table) into the first tombstone or empty entry of its probe sequence
  void place(int64_t key, int32_t slot) {
    uint32_t i = (uint32_t)mix64((uint64_t)key) & mask_;
    while (image_[i].state == kUsed) i = (i + 1u) & mask_;  // used <= half the table: ends
    if (image_[i].state == kTomb) --n_tomb_;
    image_[i] = Entry{key, slot, kUsed};
    touch(i);
  }

  void rebuild() {
    for (Entry& e : image_) e = Entry{0, 0, kEmpty};
    n_tomb_ = 0;
    dirty_all_ = true;
    dirty_.clear();
    for (uint32_t s = 0; s < n_slots_; ++s)
      if (used_[s]) place(hash_of_[s], (int32_t)s);
    ++rebuilds_;
  }

  int32_t lowest_free() {
    for (size_t w = free_hint_; w < free_.size(); ++w) {
      if (!free_[w]) continue;
      free_hint_ = (uint32_t)w;
      return (int32_t)(w * 64 + (size_t)__builtin_ctzll(free_[w]));
    }
    free_hint_ = (uint32_t)free_.size();
    return -1;
  }

  uint32_t n_slots_ = 0, mask_ = 0, n_used_ = 0, n_tomb_ = 0, free_hint_ = 0;
  uint64_t rebuilds_ = 0;
  std::vector<Entry> image_;
  std::vector<int64_t> hash_of_;
  std::vector<uint8_t> used_;
  std::vector<uint64_t> free_;  // bit s: slot s is free
  std::vector<uint32_t> dirty_;
  bool dirty_all_ = true;
};

}  // namespace avcat
