// The batch layouts (csrc/batch_layout.h) checked on the CPU. For every layout and a grid of
// dimensions: the measuring pass gives the extent of the placing pass; every region lies inside the
// buffer, meets its alignment and overlaps no other; the bytes one copy moves end where the table
// ends; a second instance over another base (pinned against device) has the same offsets. The placing
// pass runs over a heap block of exactly the measured size and every region is filled to its last
// element, so an undersized layout is an address sanitizer report.
// Stand-alone: g++ -std=c++17 host/batch_layout_test.cpp (tests/test_batch_layout_cpu.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/batch_layout.h"

namespace {

int failures = 0;
long long cases = 0;

#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
      if (++failures > 20) std::exit(1);                         \
    }                                                            \
  } while (0)

struct Region {
  const char* name;
  unsigned char* at;
  size_t bytes, align;
};
template <typename T>
Region region(const char* name, T* p, size_t count, size_t align = alignof(T)) {
  return {name, reinterpret_cast<unsigned char*>(p), count * sizeof(T), align};
}

void table_regions(std::vector<Region>& r, const avlay::Table& t, size_t n_resp, size_t n_groups, bool grouped) {
  r.push_back(region("off", t.off, n_resp + 1));
  r.push_back(region("node", t.node, n_resp));
  if (grouped) {
    r.push_back(region("order", t.order, n_resp));
    r.push_back(region("grp_off", t.grp_off, n_groups + 1));
  }
}

// a 256-byte-aligned heap block of exactly this size, as the engine's buffers are aligned
unsigned char* block(size_t bytes) {
  void* p = nullptr;
  if (posix_memalign(&p, 256, bytes) != 0) std::exit(2);
  return static_cast<unsigned char*>(p);
}

// lay(carver, regions*) runs one layout and, with regions, lists what it placed; it returns the copy
// prefix's length and where the table ends (both 0 for a layout with no prefix)
struct Prefix {
  size_t bytes;
  const void* table_end;
};
template <typename Lay>
void check_layout(const char* what, Lay lay) {
  ++cases;
  avlay::Carver measure;
  lay(measure, nullptr);
  const size_t bytes = measure.bytes();
  CHECK(bytes > 0, "%s: empty layout", what);
  unsigned char *a = block(bytes), *b = block(bytes);
  std::vector<Region> ra, rb;
  avlay::Carver ca(a), cb(b);
  const Prefix pa = lay(ca, &ra);
  lay(cb, &rb);
  CHECK(ca.bytes() == bytes && cb.bytes() == bytes, "%s: measured %zu, placed %zu", what, bytes, ca.bytes());
  for (size_t i = 0; i < ra.size(); ++i) {
    const Region& r = ra[i];
    CHECK(r.at >= a && r.at + r.bytes <= a + bytes, "%s: %s [%td, +%zu) outside %zu bytes", what, r.name, r.at - a,
          r.bytes, bytes);
    CHECK(reinterpret_cast<uintptr_t>(r.at) % r.align == 0, "%s: %s not %zu-byte aligned", what, r.name, r.align);
    CHECK(r.at - a == rb[i].at - b, "%s: %s at %td in one instance, %td in the other", what, r.name, r.at - a,
          rb[i].at - b);
    std::memset(r.at, 0xA5, r.bytes);  // to its last element: the block is exactly `bytes` long
  }
  std::vector<Region> s = ra;
  std::sort(s.begin(), s.end(),
            [](const Region& x, const Region& y) { return x.at != y.at ? x.at < y.at : x.bytes < y.bytes; });
  for (size_t i = 0; i + 1 < s.size(); ++i)
    CHECK(s[i].at + s[i].bytes <= s[i + 1].at, "%s: %s overlaps %s", what, s[i].name, s[i + 1].name);
  if (pa.table_end)
    CHECK(a + pa.bytes == pa.table_end, "%s: prefix %zu, the table ends at %td", what, pa.bytes,
          static_cast<const unsigned char*>(pa.table_end) - a);
  std::free(a);
  std::free(b);
}

const size_t kM[] = {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4097};
const size_t kResp[] = {1, 2, 3, 64};
const size_t kTemp[] = {0, 1, 7, 1000};

void group_regions(std::vector<Region>& r, const avk::GroupScratch& g, size_t m, size_t temp_words) {
  r.push_back(region("keys", g.keys, m));
  r.push_back(region("vidx", g.vidx, m));
  r.push_back(region("info", g.info, m));
  r.push_back(region("keys_s", g.keys_s, m));
  r.push_back(region("perm_s", g.perm_s, m));
  r.push_back(region("keys_t", g.keys_t, m));
  r.push_back(region("perm_t", g.perm_t, m));
  r.push_back(region("lanes", g.lanes, m));
  r.push_back(region("offs", g.offs, m + 1));
  r.push_back(region("nruns", g.nruns, 1));
  r.push_back(region("entries", g.entries, 2 * m));
  r.push_back(region("temp", g.temp, temp_words, 256));
}

void batches(size_t m, size_t n_resp, size_t n_groups, size_t temp_words) {
  char what[96];
  std::snprintf(what, sizeof what, "m=%zu n_resp=%zu n_groups=%zu temp=%zu", m, n_resp, n_groups, temp_words);
  check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
    const avlay::Table t = avlay::table(c, n_resp, n_groups);
    if (r) table_regions(*r, t, n_resp, n_groups, true);
    return Prefix{0, nullptr};
  });
  // a batch head, alone (pinned memory; the fast path's device buffer) and with the grouping scratch
  // behind it (the general path's device buffer)
  for (int with_group = 0; with_group < 2; ++with_group) {
    check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
      const avlay::VoteBatch b = avlay::vote_batch(c, m, n_resp, n_groups);
      const avk::GroupScratch g = with_group ? avlay::group_scratch(c, m, temp_words) : avk::GroupScratch{};
      if (!r) return Prefix{0, nullptr};
      r->push_back(region("packed", b.packed, m));
      table_regions(*r, b.tab, n_resp, n_groups, true);
      r->push_back(region("status", b.status, m));
      if (with_group) group_regions(*r, g, m, temp_words);
      CHECK(reinterpret_cast<unsigned char*>(b.packed) == r->front().at, "%s: packed is the base", what);
      return Prefix{b.prefix_bytes, b.tab.grp_off + n_groups + 1};
    });
    check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
      const avlay::AddBatch b = avlay::add_batch(c, m, n_resp);
      const avk::GroupScratch g = with_group ? avlay::group_scratch(c, m, temp_words) : avk::GroupScratch{};
      if (!r) return Prefix{0, nullptr};
      r->push_back(region("packed", b.packed, m));
      table_regions(*r, b.tab, n_resp, 0, false);
      CHECK(!b.tab.order && !b.tab.grp_off, "%s: the adds' table has no grouping", what);
      r->push_back(region("added", b.added, m));
      if (with_group) group_regions(*r, g, m, temp_words);
      return Prefix{b.prefix_bytes, b.tab.node + n_resp};
    });
  }
  check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
    const avlay::HashedBatch b = avlay::hashed_batch(c, m, n_resp, n_groups);
    if (!r) return Prefix{0, nullptr};
    r->push_back(region("hashes", b.hashes, m, 16));
    r->push_back(region("errs", b.errs, m));
    table_regions(*r, b.tab, n_resp, n_groups, true);
    r->push_back(region("packed", b.packed, m, 8));
    r->push_back(region("flag", b.flag, 1));
    r->push_back(region("status", b.status, m));
    return Prefix{b.prefix_bytes, b.tab.grp_off + n_groups + 1};
  });
  // the hashed call's grouping scratch: a buffer of its own
  check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
    const avk::GroupScratch g = avlay::group_scratch(c, m, temp_words);
    if (r) group_regions(*r, g, m, temp_words);
    return Prefix{0, nullptr};
  });
}

// the smaller layouts: m doubles as touched blocks, local targets and nodes
void small_layouts(size_t m) {
  char what[64];
  std::snprintf(what, sizeof what, "small m=%zu", m);
  for (size_t cnt : {(size_t)0, m * 32}) {
    check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
      const avlay::AdmitTable t = avlay::admit_table(c, m, cnt);
      if (!r) return Prefix{0, nullptr};
      r->push_back(region("tblk", t.tblk, m));
      r->push_back(region("treq", t.treq, m));
      r->push_back(region("tacc", t.tacc, m));
      CHECK((t.counts != nullptr) == (cnt != 0), "%s: counts only when asked for", what);
      if (cnt) r->push_back(region("counts", t.counts, cnt));
      return Prefix{t.prefix_bytes, t.tacc + m};
    });
  }
  for (size_t nn : {(size_t)0, (size_t)1, m}) {
    check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
      const avlay::CensusSums s = avlay::census_sums(c, m, nn);
      if (!r) return Prefix{0, nullptr};
      r->push_back(region("tcls", s.tcls, m * 3));
      r->push_back(region("tsum", s.tsum, m));
      r->push_back(region("hist", s.hist, 256));
      r->push_back(region("counted", s.counted, 1));
      CHECK((s.ncls != nullptr) == (nn != 0), "%s: node rows only when asked for", what);
      if (nn) r->push_back(region("ncls", s.ncls, nn * 4, 16));
      CHECK(s.head_bytes % 16 == 0 && s.head_bytes == (m * 4 + 256 + 2) * 8, "%s: head of %zu bytes", what,
            s.head_bytes);
      return Prefix{0, nullptr};
    });
  }
  check_layout(what, [&](avlay::Carver& c, std::vector<Region>* r) {
    const avlay::FindStaging f = avlay::find_staging(c, m);
    if (!r) return Prefix{0, nullptr};
    r->push_back(region("hashes", f.hashes, m, 16));
    r->push_back(region("packed", f.packed, m, 8));
    return Prefix{0, nullptr};
  });
}

}  // namespace

int main() {
  // the carver itself: offsets round up, a measuring carver returns no pointer
  avlay::Carver c;
  CHECK(c.take<uint8_t>(3) == nullptr && c.bytes() == 3, "3 bytes");
  c.take<uint32_t>(1);
  CHECK(c.bytes() == 8, "a u32 after 3 bytes ends at %zu", c.bytes());
  c.take<uint64_t>(0, 256);
  CHECK(c.bytes() == 256, "an empty 256-byte-aligned region ends at %zu", c.bytes());
  for (size_t m : kM) {
    for (size_t n_resp : kResp)
      for (size_t n_groups = 1; n_groups <= n_resp; ++n_groups)
        for (size_t temp : kTemp) batches(m, n_resp, n_groups, temp);
    small_layouts(m);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("PASS batch_layout (%lld layouts)\n", cases);
  return 0;
}
