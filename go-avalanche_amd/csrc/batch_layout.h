// Where the drop-in write batches, the admission table, the census sums and the catalog's parity dump
// keep their arrays inside one buffer: each layout is one function that takes regions from a bump
// carver, so the same description gives the size (a carver over no base) and the pointers (the same
// function over the real base), in pinned and in device memory alike. Host C++17 with no HIP include:
// host/batch_layout_test.cpp checks it on the CPU. A base is 256-byte aligned (hipMalloc,
// hipHostMalloc); alignments are met as offsets from it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace avk {

// The grouping of m entries by lane: launch_dropin_keys writes keys / vidx / info, launch_group_votes
// sorts them and leaves the runs (kernels.h).
struct GroupScratch {
  uint32_t *keys, *vidx, *info;                  // [m] lane key, position and packed vote of every entry
  uint32_t *keys_s, *perm_s, *keys_t, *perm_t;   // [m] the radix sort's two buffer sets; sorted: (keys_s, perm_s)
  uint32_t *lanes, *offs, *nruns, *entries;      // the runs: lanes [m], offs [m + 1], their number, entries [2m]
  uint64_t* temp;                                // the radix sort's and run scan's u64 words, 256-byte aligned
};

}  // namespace avk

namespace avlay {

// Takes regions one after the other from base, or measures them when base is null.
class Carver {
 public:
  explicit Carver(void* base = nullptr) : base_(static_cast<unsigned char*>(base)) {}
  template <typename T>
  T* take(size_t count, size_t align = alignof(T)) {
    off_ = (off_ + align - 1) / align * align;
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += count * sizeof(T);
    return p;
  }
  size_t bytes() const { return off_; }  // the extent so far

 private:
  unsigned char* base_;
  size_t off_ = 0;
};

// The caller's request table as the kernels read it (DropInParams): request r = entries
// [off[r], off[r + 1]) of local node node[r]; for votes also the Responses grouped by node (order,
// grp_off), which the adds leave out.
struct Table {
  uint32_t *off, *node, *order, *grp_off;
};
inline Table table(Carver& c, size_t n_resp, size_t n_groups, bool grouped = true) {
  Table t{};
  t.off = c.take<uint32_t>(n_resp + 1);
  t.node = c.take<uint32_t>(n_resp);
  if (grouped) {
    t.order = c.take<uint32_t>(n_resp);
    t.grp_off = c.take<uint32_t>(n_groups + 1);
  }
  return t;
}

// temp_words: avk::group_votes_scratch_words(m)
inline avk::GroupScratch group_scratch(Carver& c, size_t m, size_t temp_words) {
  avk::GroupScratch g{};
  g.keys = c.take<uint32_t>(m);
  g.vidx = c.take<uint32_t>(m);
  g.info = c.take<uint32_t>(m);
  g.keys_s = c.take<uint32_t>(m);
  g.perm_s = c.take<uint32_t>(m);
  g.keys_t = c.take<uint32_t>(m);
  g.perm_t = c.take<uint32_t>(m);
  g.lanes = c.take<uint32_t>(m);
  g.offs = c.take<uint32_t>(m + 1);
  g.nruns = c.take<uint32_t>(1);
  g.entries = c.take<uint32_t>(2 * m);
  g.temp = c.take<uint64_t>(temp_words, 256);
  return g;
}

// The batch heads. [base, base + prefix_bytes) is what the host fills and one copy moves to the
// device; the last region is the bytes that come back.

// av_register_votes_batch: m packed votes (dropin_word)
struct VoteBatch {
  uint32_t* packed;
  Table tab;
  int8_t* status;
  size_t prefix_bytes;
};
inline VoteBatch vote_batch(Carver& c, size_t m, size_t n_resp, size_t n_groups) {
  VoteBatch b{};
  b.packed = c.take<uint32_t>(m);
  b.tab = table(c, n_resp, n_groups);
  b.prefix_bytes = c.bytes();
  b.status = c.take<int8_t>(m);
  return b;
}

// av_register_votes_hashed: the caller's hashes and errs go in, the lookup kernel writes packed (two
// votes per store) and the unordered flag
struct HashedBatch {
  int64_t* hashes;
  uint32_t* errs;
  Table tab;
  uint32_t *packed, *flag;
  int8_t* status;
  size_t prefix_bytes;
};
inline HashedBatch hashed_batch(Carver& c, size_t m, size_t n_resp, size_t n_groups) {
  HashedBatch b{};
  b.hashes = c.take<int64_t>(m, 16);
  b.errs = c.take<uint32_t>(m);
  b.tab = table(c, n_resp, n_groups);
  b.prefix_bytes = c.bytes();
  b.packed = c.take<uint32_t>(m, 8);
  b.flag = c.take<uint32_t>(1);
  b.status = c.take<int8_t>(m);
  return b;
}

// av_add_targets_batch: m packed entries (add_word)
struct AddBatch {
  uint32_t* packed;
  Table tab;
  uint8_t* added;
  size_t prefix_bytes;
};
inline AddBatch add_batch(Carver& c, size_t m, size_t n_req) {
  AddBatch b{};
  b.packed = c.take<uint32_t>(m);
  b.tab = table(c, n_req, 0, false);
  b.prefix_bytes = c.bytes();
  b.added = c.take<uint8_t>(m);
  return b;
}

// av_admit_targets: the touched blocks (AdmitParams), then cnt_words counters (0: none, counts null)
struct AdmitTable {
  uint32_t *tblk, *treq, *tacc, *counts;
  size_t prefix_bytes;
};
inline AdmitTable admit_table(Carver& c, size_t tb, size_t cnt_words) {
  AdmitTable t{};
  t.tblk = c.take<uint32_t>(tb);
  t.treq = c.take<uint32_t>(tb);
  t.tacc = c.take<uint32_t>(tb);
  t.prefix_bytes = c.bytes();
  uint32_t* counts = c.take<uint32_t>(cnt_words);
  t.counts = cnt_words ? counts : nullptr;
  return t;
}

// av_census: the u64 sums the host copies back as one block of head_bytes (the pad word keeps that a
// multiple of 16), then nn node rows of four int32 (0: none, ncls null)
struct CensusSums {
  unsigned long long *tcls, *tsum, *hist, *counted;
  int32_t* ncls;
  size_t head_bytes;
};
inline CensusSums census_sums(Carver& c, size_t tn, size_t nn) {
  CensusSums s{};
  s.tcls = c.take<unsigned long long>(tn * 3);
  s.tsum = c.take<unsigned long long>(tn);
  s.hist = c.take<unsigned long long>(256);
  s.counted = c.take<unsigned long long>(1);
  c.take<unsigned long long>(1);
  s.head_bytes = c.bytes();
  int32_t* ncls = c.take<int32_t>(nn * 4, 16);
  s.ncls = nn ? ncls : nullptr;
  return s;
}

// av_catalog_find_device: hashes in, packed words back
struct FindStaging {
  int64_t* hashes;
  uint32_t* packed;
};
inline FindStaging find_staging(Carver& c, size_t m) {
  FindStaging f{};
  f.hashes = c.take<int64_t>(m, 16);
  f.packed = c.take<uint32_t>(m, 8);
  return f;
}

}  // namespace avlay
