// The peer draw over per-node peer lists (rule R6): a node's Connman (net.go:11-31), from
// whose NodesIDs() the reference picks whom to query (processor.go:173-182). Included by the listed
// round kernel and by the parity dumps (round_listed.hip), which therefore cannot disagree.
//
// Node n has a list C(n) of d global ids, strictly ascending, none of them n (av_set_peer_lists
// validates this on the host: peer_list_check.h). d <= K: slot s < d polls C(n)[s], slots s >= d are
// empty. d > K: R1's candidate stream with "the other N - 1 nodes" replaced by "the list":
// u = (x[i] * d) >> 32 over x = philox4x32-10({n, r, blk, kDomPeers}, seed), blk = 0, 1, ...; the first
// K distinct u in stream order; slot s polls C(n)[u_s]. A list of every other node draws what
// sample_peers draws (C(n)[u] = u + (u >= n)).
//
// Everything here is per-lane code with no cross-lane operation: the walk's trip count differs
// between nodes that share a wave, and a node whose lanes straddle two waves draws once in each, from
// (seed, node, round) and its list alone.
#pragma once

#include "round_common.h"

namespace avk {

// General form: the first K distinct indices below d of the candidate stream. Terminates because
// d > K (the caller's branch, on d taken from the validated offsets).
template <int K>
__device__ __forceinline__ void listed_walk(uint64_t seed, uint32_t node, uint32_t round, uint32_t d,
                                            uint32_t (&u)[K]) {
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) u[j] = 0u;
  for (uint32_t blk = 0; cnt < (uint32_t)K; ++blk) {
    uint32_t x[4];
    philox(x, seed, node, round, blk, kDomPeers);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t c = (uint32_t)(((uint64_t)x[i] * d) >> 32);
      bool dup = false;
#pragma unroll
      for (int j = 0; j < K; ++j) dup |= ((uint32_t)j < cnt) && (u[j] == c);
      if (!dup && cnt < (uint32_t)K) {
#pragma unroll
        for (int j = 0; j < K; ++j) u[j] = ((uint32_t)j == cnt) ? c : u[j];
        ++cnt;
      }
    }
  }
}

// The K peers of local node nl (global id `node`) in `round` and, returned, its empty-slot mask
// (bit s: slot s polls nobody; out[s] is then 0 and must not be used as an index). offsets: [NL + 1]
// into list, by local node.
template <int K>
__device__ __forceinline__ uint32_t sample_listed(uint64_t seed, uint32_t node, uint32_t round,
                                                  const uint32_t* offsets, const uint32_t* list, uint32_t nl,
                                                  uint32_t (&out)[K]) {
  constexpr uint32_t kAll = (1u << K) - 1u;
  const uint32_t o0 = offsets[nl], d = offsets[nl + 1] - o0;
  const uint32_t* const C = list + o0;
  if (d <= (uint32_t)K) {
#pragma unroll
    for (int j = 0; j < K; ++j) out[j] = (uint32_t)j < d ? C[j] : 0u;
    return kAll & ~((1u << d) - 1u);
  }
  // fast path as in sample_peers: the first ceil(K/4) blocks hold K distinct candidates
  constexpr int NB = (K + 3) / 4;
  uint32_t cand[NB * 4], u[K];
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    uint32_t x[4];
    philox(x, seed, node, round, (uint32_t)blk, kDomPeers);
#pragma unroll
    for (int i = 0; i < 4; ++i) cand[blk * 4 + i] = (uint32_t)(((uint64_t)x[i] * d) >> 32);
  }
  bool distinct = true;
#pragma unroll
  for (int i = 1; i < K; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) distinct &= cand[i] != cand[j];
  if (distinct) {
#pragma unroll
    for (int j = 0; j < K; ++j) u[j] = cand[j];
  } else {
    listed_walk<K>(seed, node, round, d, u);  // the normal case at d = K + 1
  }
#pragma unroll
  for (int j = 0; j < K; ++j) out[j] = C[u[j]];
  return 0u;
}

}  // namespace avk
