// CPU checks of csrc/peer_list_check.h (no GPU, no HIP): what av_set_peer_lists accepts and refuses,
// that a refusal leaves the outputs as they were, and that the 32-bit form holds what was passed.
// Stand-alone, so it also runs under a host sanitizer. Exit status 0 = all passed
// (tests/test_peer_list_check.py).
#include <cstdio>
#include <vector>

#include "../csrc/peer_list_check.h"

using namespace avk;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond) && ++g_failed <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
  } while (0)

static PeerListError run(int64_t n, int64_t n0, const std::vector<int64_t>& offs, const std::vector<int64_t>& peers,
                         std::vector<uint32_t>* o, std::vector<uint32_t>* l, int64_t* bad = nullptr) {
  return check_peer_lists(n, n0, (int64_t)offs.size() - 1, offs.data(), peers.empty() ? nullptr : peers.data(), o, l,
                          bad);
}

int main() {
  std::vector<uint32_t> o{7}, l{8, 9};
  const std::vector<uint32_t> o0 = o, l0 = l;
  int64_t bad = 0;
  // four local nodes 4..7 of a network of 10: degrees 2, 0, 3, 1
  const std::vector<int64_t> offs{0, 2, 2, 5, 6}, peers{0, 9, 1, 5, 7, 4};
  CHECK(run(10, 4, offs, peers, &o, &l, &bad) == PeerListError::Ok && bad == -1);
  CHECK((o == std::vector<uint32_t>{0, 2, 2, 5, 6}) && (l == std::vector<uint32_t>{0, 9, 1, 5, 7, 4}));
  // every list empty, with no peer array at all
  CHECK(run(10, 4, {0, 0, 0, 0, 0}, {}, &o, &l) == PeerListError::Ok && o.size() == 5 && l.empty());
  // no local node
  CHECK(run(10, 4, {0}, {}, &o, &l) == PeerListError::Ok && o.size() == 1 && l.empty());
  o = o0, l = l0;
  struct Case {
    std::vector<int64_t> offs, peers;
    PeerListError want;
    int64_t bad;
  };
  const Case cases[] = {
      {{1, 2, 2, 5, 6}, peers, PeerListError::FirstOffset, -1},
      {{0, 2, 1, 5, 6}, peers, PeerListError::Decreasing, 1},
      {{0, 2, 2, 5, (int64_t)1 << 31}, peers, PeerListError::TooLong, 3},
      {{0, (int64_t)1 << 40, (int64_t)1 << 40, (int64_t)1 << 40, (int64_t)1 << 40}, peers, PeerListError::TooLong, 0},
      {{0, 2, 2, 5, 6}, {}, PeerListError::Null, -1},
      {offs, {0, 10, 1, 5, 7, 4}, PeerListError::Range, 0},
      {offs, {-1, 9, 1, 5, 7, 4}, PeerListError::Range, 0},
      {offs, {0, 9, 1, 6, 7, 4}, PeerListError::Self, 2},
      {offs, {0, 9, 1, 5, 7, 7}, PeerListError::Self, 3},
      {offs, {9, 0, 1, 5, 7, 4}, PeerListError::Order, 0},
      {offs, {0, 9, 1, 5, 5, 4}, PeerListError::Order, 2},  // a duplicate
      {offs, {0, 9, 7, 5, 1, 4}, PeerListError::Order, 2},
  };
  for (const Case& c : cases) {
    bad = 99;
    const PeerListError got = run(10, 4, c.offs, c.peers, &o, &l, &bad);
    CHECK(got == c.want);
    if (c.want != PeerListError::FirstOffset && c.want != PeerListError::Null) CHECK(bad == c.bad);
    CHECK(o == o0 && l == l0);  // nothing changed
    CHECK(peer_list_error_text(got)[0] != '?');
  }
  // the longest list a node can have: every other node
  std::vector<int64_t> full;
  for (int64_t q = 0; q < 10; ++q)
    if (q != 6) full.push_back(q);
  CHECK(run(10, 6, {0, 9}, full, &o, &l) == PeerListError::Ok && l.size() == 9 && l[6] == 7);
  std::printf("peer_list_check_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
