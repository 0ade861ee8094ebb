// The Hash catalog (csrc/catalog.h) checked on the CPU against a std::map model: random walks of
// intern / retire / find, the lowest-free-slot rule, duplicates inside one call, the full catalog,
// the keys no sentinel could stand for, and enough churn that the table image is rebuilt several
// times. After every step the image is walked with probe(), the function the device lookup shares.
// Stand-alone: g++ -std=c++17 host/catalog_test.cpp (tests/test_catalog_cpu.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../csrc/catalog.h"

namespace {

int failures = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      if (++failures > 20) std::exit(1);                  \
    }                                                     \
  } while (0)

// the slot rule as a caller's model: hash -> slot, the free slots ordered
struct Model {
  std::map<int64_t, int32_t> slot_of;
  std::set<int32_t> free;
  explicit Model(uint32_t n) {
    for (uint32_t s = 0; s < n; ++s) free.insert((int32_t)s);
  }
  int32_t intern(int64_t k) {
    auto it = slot_of.find(k);
    if (it != slot_of.end()) return it->second;
    if (free.empty()) return -1;
    const int32_t s = *free.begin();
    free.erase(free.begin());
    slot_of[k] = s;
    return s;
  }
  bool retire(int64_t k) {
    auto it = slot_of.find(k);
    if (it == slot_of.end()) return false;
    free.insert(it->second);
    slot_of.erase(it);
    return true;
  }
  int32_t find(int64_t k) const {
    auto it = slot_of.find(k);
    return it == slot_of.end() ? -1 : it->second;
  }
};

// the whole image against the model: every model key is found by probe() at its slot, every used
// entry of the image is a model key, the bookkeeping adds up and a quarter of the table is empty
void check_image(const avcat::Catalog& c, const Model& m, const std::vector<int64_t>& seen, const char* where) {
  const avcat::Entry* tab = c.image();
  uint32_t used = 0, tomb = 0, empty = 0;
  for (uint32_t i = 0; i < c.entries(); ++i) {
    const avcat::Entry& e = tab[i];
    CHECK(e.state <= avcat::kTomb, "%s: state %u at %u", where, e.state, i);
    if (e.state == avcat::kUsed) {
      ++used;
      CHECK(m.find(e.key) == e.slot, "%s: entry %u holds key %" PRId64 " slot %d, model %d", where, i, e.key, e.slot,
            m.find(e.key));
    } else if (e.state == avcat::kTomb) {
      ++tomb;
    } else {
      ++empty;
    }
  }
  CHECK(used == m.slot_of.size() && used == c.n_used(), "%s: used %u, model %zu, counter %u", where, used,
        m.slot_of.size(), c.n_used());
  CHECK(tomb == c.n_tombstones(), "%s: tombstones %u, counter %u", where, tomb, c.n_tombstones());
  CHECK(tomb <= c.entries() / 4u && used <= c.entries() / 2u && empty >= c.entries() / 4u,
        "%s: used %u tomb %u empty %u of %u", where, used, tomb, empty, c.entries());
  for (int64_t k : seen) {
    const int32_t got = avcat::probe(tab, c.mask(), k);
    CHECK(got == m.find(k) && got == c.find(k), "%s: probe(%" PRId64 ") = %d, model %d", where, k, got, m.find(k));
  }
  for (uint32_t s = 0; s < c.n_slots(); ++s) {
    const bool free = m.free.count((int32_t)s) != 0;
    CHECK(c.slot_used(s) == !free, "%s: slot %u used %d, model free %d", where, s, (int)c.slot_used(s), (int)free);
    if (!free) CHECK(m.find(c.hash_of(s)) == (int32_t)s, "%s: hash_of(%u)", where, s);
  }
}

const int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();

void edge_keys(uint32_t n_slots) {
  avcat::Catalog c;
  CHECK(!c.ready() && c.find(0) == -1 && !c.retire(0), "an uninitialised catalog finds nothing");
  c.init(n_slots);
  Model m(n_slots);
  std::vector<int64_t> seen = {0, -1, kMin, kMax, 1, 2, 3, (int64_t)n_slots - 1, (int64_t)n_slots};
  CHECK(c.find(0) == -1 && c.find(-1) == -1 && c.find(kMin) == -1, "an empty catalog finds nothing");
  check_image(c, m, seen, "empty");
  // call order decides the slot: the lowest free one, whatever the key's value (a key equal to a
  // slot number is not that slot)
  int32_t want = 0;
  for (int64_t k : {(int64_t)3, kMin, (int64_t)0, (int64_t)-1, kMax, (int64_t)1}) {
    bool fresh = false;
    const int32_t s = c.intern(k, &fresh);
    CHECK(s == want && fresh && m.intern(k) == s, "intern(%" PRId64 ") = %d, expected %d", k, s, want);
    ++want;
    check_image(c, m, seen, "edge intern");
  }
  // duplicates, inside one call's list too: the same slot, nothing new
  for (int64_t k : {kMin, kMin, (int64_t)0, (int64_t)3, (int64_t)-1, (int64_t)-1}) {
    bool fresh = true;
    const int32_t s = c.intern(k, &fresh);
    CHECK(s == m.find(k) && !fresh && c.n_used() == 6u, "duplicate intern(%" PRId64 ") = %d", k, s);
  }
  // freed slots are taken lowest first
  CHECK(c.retire(0) && m.retire(0) && c.retire(3) && m.retire(3), "retire");
  CHECK(!c.retire(0) && !c.retire(12345), "retiring an uncatalogued key changes nothing");
  check_image(c, m, seen, "edge retire");
  CHECK(c.find(0) == -1 && c.find(3) == -1 && c.find(kMin) == 1, "retired keys are gone");
  bool fresh = false;
  CHECK(c.intern(2, &fresh) == 0 && fresh && m.intern(2) == 0, "the lowest free slot (0) first");
  CHECK(c.intern(0, &fresh) == 2 && fresh && m.intern(0) == 2, "then slot 2");
  check_image(c, m, seen, "edge reuse");
  // fill up, then past it: -1 and nothing changes
  int64_t k = 1000;
  while (!m.free.empty()) {
    const int32_t s = c.intern(k, &fresh);
    CHECK(s == m.intern(k) && fresh, "fill intern(%" PRId64 ")", k);
    seen.push_back(k);
    ++k;
  }
  check_image(c, m, seen, "full");
  const uint64_t rb = c.rebuilds();
  for (int64_t q : {(int64_t)-7, (int64_t)999999, kMax - 1}) {
    fresh = true;
    CHECK(c.intern(q, &fresh) == -1 && !fresh && c.find(q) == -1, "a full catalog refuses a new key");
    seen.push_back(q);
  }
  CHECK(c.n_used() == n_slots && c.rebuilds() == rb, "a refused intern changes nothing");
  CHECK(c.intern(kMin) == 1 && c.intern(1000) == m.find(1000), "a full catalog still finds what it holds");
  check_image(c, m, seen, "past full");
}

void random_walk(uint32_t n_slots, uint64_t seed, int steps) {
  std::mt19937_64 rng(seed);
  avcat::Catalog c;
  c.init(n_slots);
  Model m(n_slots);
  // a small key pool (so that finds and retires hit) of edge keys, slot numbers and random values
  std::vector<int64_t> pool = {0, -1, kMin, kMax, kMin + 1, kMax - 1};
  for (uint32_t s = 0; s < n_slots; ++s) pool.push_back((int64_t)s);
  while (pool.size() < 4u * n_slots) pool.push_back((int64_t)rng());
  char where[64];
  for (int step = 0; step < steps; ++step) {
    std::snprintf(where, sizeof where, "walk %u/%" PRIu64 " step %d", n_slots, seed, step);
    const int64_t k = pool[rng() % pool.size()];
    const unsigned op = (unsigned)(rng() % 8u);
    if (op < 4) {
      bool fresh = false;
      const bool had = m.find(k) >= 0, room = !m.free.empty();
      const int32_t s = c.intern(k, &fresh);
      CHECK(s == m.intern(k) && fresh == (!had && room), "%s: intern(%" PRId64 ") = %d", where, k, s);
    } else if (op < 7) {
      const bool exp = m.retire(k);
      CHECK(c.retire(k) == exp, "%s: retire(%" PRId64 ")", where, k);
    } else {
      CHECK(c.find(k) == m.find(k), "%s: find(%" PRId64 ")", where, k);
    }
    check_image(c, m, pool, where);
  }
  std::printf("walk slots=%u seed=%" PRIu64 ": %d steps, %" PRIu64 " rebuilds, %u used, %u tombstones\n", n_slots,
              seed, steps, c.rebuilds(), c.n_used(), c.n_tombstones());
  CHECK(c.rebuilds() > 2, "churn at %u slots rebuilt the image %" PRIu64 " times", n_slots, c.rebuilds());
}

// what the engine sends to the device: single entries while few change, the whole image otherwise
void dirty_tracking() {
  avcat::Catalog c;
  c.init(64);
  CHECK(c.dirty_all(), "a new image is sent whole");
  c.clear_dirty();
  std::vector<avcat::Entry> copy(c.image(), c.image() + c.entries());
  std::mt19937_64 rng(5);
  std::vector<int64_t> keys;
  for (int step = 0; step < 4000; ++step) {
    if (keys.empty() || (rng() % 3u && keys.size() < 64)) {
      keys.push_back((int64_t)rng());
      c.intern(keys.back());
    } else {
      const size_t i = rng() % keys.size();
      c.retire(keys[i]);
      keys.erase(keys.begin() + (long)i);
    }
    if (rng() % 4u) continue;  // several changes per transfer
    if (c.dirty_all()) {
      copy.assign(c.image(), c.image() + c.entries());
    } else {
      for (uint32_t i : c.dirty()) copy[i] = c.image()[i];
    }
    c.clear_dirty();
    for (uint32_t i = 0; i < c.entries(); ++i) {
      const avcat::Entry &a = copy[i], &b = c.image()[i];
      CHECK(a.key == b.key && a.slot == b.slot && a.state == b.state, "patched copy differs at entry %u (step %d)", i,
            step);
    }
  }
  CHECK(c.rebuilds() > 0, "the walk rebuilt the image");
}

}  // namespace

int main() {
  CHECK(avcat::table_entries(33) == 128u && avcat::table_entries(64) == 128u && avcat::table_entries(65) == 256u &&
            avcat::table_entries(1) == 16u,
        "table sizes");
  edge_keys(33);
  edge_keys(64);
  for (uint64_t seed = 1; seed <= 3; ++seed) {
    random_walk(33, seed, 3000);
    random_walk(64, seed, 3000);
  }
  random_walk(7, 9, 1500);
  dirty_tracking();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("PASS catalog\n");
  return 0;
}
