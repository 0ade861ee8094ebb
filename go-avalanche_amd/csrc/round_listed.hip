// The round over per-node peer lists (rule R6) for CDNA4 (gfx950): k_round_listed, one lane
// per 32-record block like k_round_lossy, whose body it shares (round_lossy_body.h), uncapped,
// k = 1..16, and k_sample_listed, the parity dump of its draw and of the lost mask that follows it
// (av_sample_peers / av_sample_lost of an engine with lists).
//
// In the reference every Processor owns a Connman (net.go:11-31) and picks whom to query from its
// NodesIDs() (processor.go:173-182). A node that knows d < k peers sends d queries: the other k - d
// slots are empty, which is a RegisterVotes call that never happens, and not a lost Response either.
// The kernel therefore carries two masks per node: `empty` (always sat out) and `lost` (sat out or
// neutral by the loss mode, rule R5). It runs every sim round of an engine with lists, with or
// without R5.
//
// Next to k_round_lossy a lane reads its node's two offsets and then up to k list entries: two
// dependent loads ahead of the preference gather. The lists live in HBM (at 1M nodes of degree 64
// they are 256 MB): the 32 lanes of a node read the same words, so a wave's draw costs a handful of
// cache lines, but nothing here assumes that the lists stay resident between rounds. Measured at C4
// (DESIGN.md §4, round 14): 1.36x R5's skip round at degree 64, 1.68x at degree 9 (the walk); the
// excess is the same in every round, which points at the serialised chain, not at the bytes.
//
// Divergence. Two nodes that share a wave (BL <= 32) may take different branches of the draw and
// walk its candidate stream a different number of times; sample_listed has no cross-lane operation,
// and every ballot and wave sum below comes after it, where the wave has reconverged. A node whose
// lanes straddle two waves (BL = 66) draws in each from (seed, node, round) and its list alone.
// Lanes past the last tile read no list and no bitset: their slots are all empty.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "peer_lists.h"
#include "round_lossy_body.h"

namespace avk {

namespace {

template <int K, bool NEUTRAL>
__global__ __launch_bounds__(256) void k_round_listed(const ListedParams q) {
  const LossyParams& lp = q.l;
  const RoundParams& p = lp.r;
  constexpr uint32_t kAll = (1u << K) - 1u;
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  if ((g & ~63u) >= p.L) return;  // whole wave beyond the last tile
  const bool active = g < p.L;
  const uint32_t nl = active ? g / p.BL : 0u;
  const uint32_t b = active ? g - nl * p.BL : 0u;
  const uint32_t node = p.n0 + nl;
  // a node whose run loop has returned (main.go:160-162) polls nothing; it still answers
  const bool polls = !p.nopoll || !((p.nopoll[nl >> 5] >> (nl & 31u)) & 1u);
  uint32_t peers[K];
#pragma unroll
  for (int j = 0; j < K; ++j) peers[j] = 0u;
  uint32_t empty = kAll;
  if (active) empty = sample_listed<K>(p.seed, node, p.round, q.offsets, q.list, nl, peers);
  // (an empty slot's peers[] entry indexes nothing: lost_mask and the body's gather sit under the mask)
  const uint32_t lost = lost_mask<K>(p.seed, node, p.round, lp.loss_threshold, lp.responding, peers, empty);
  if constexpr (!NEUTRAL) {
    if (p.warm_skip) {
      // (a lane that sits every slot out touches no consider plane: it does not read C7 either)
      const uint32_t c7 = active && (lost | empty) != kAll ? *pw(p.planes, g, kPC + 7) : ~0u;
      if (__all(c7 == ~0u)) {  // wave-uniform
        if (p.plane_nt)
          round_lossy_body<K, false, true, true, true>(lp, g, lane, active, b, node, polls, lost, peers, empty, q.unsent);
        else
          round_lossy_body<K, false, true, false, true>(lp, g, lane, active, b, node, polls, lost, peers, empty, q.unsent);
        return;
      }
    }
  }
  if (p.plane_nt)
    round_lossy_body<K, NEUTRAL, false, true, true>(lp, g, lane, active, b, node, polls, lost, peers, empty, q.unsent);
  else
    round_lossy_body<K, NEUTRAL, false, false, true>(lp, g, lane, active, b, node, polls, lost, peers, empty, q.unsent);
}

template <int K>
hipError_t launch_listed_k(const ListedParams& p, bool neutral, hipStream_t s) {
  const uint32_t blocks = (p.l.r.Lpad + 255u) / 256u;
  if (neutral)
    hipLaunchKernelGGL((k_round_listed<K, true>), dim3(blocks), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL((k_round_listed<K, false>), dim3(blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

// Local nodes [a, b) of `round`: the peers ([b - a][K], AV_NO_PEER = -1 in empty slots) and / or the
// lost mask ([b - a][K] bytes, 0 in empty slots).
template <int K>
__global__ void k_sample_listed(uint64_t seed, uint32_t n0, uint32_t a, uint32_t b, uint32_t round,
                                const uint32_t* offsets, const uint32_t* list, uint32_t threshold,
                                const uint32_t* responding, int32_t* peers_out, uint8_t* lost_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (a + i >= b) return;
  uint32_t peers[K];
  const uint32_t empty = sample_listed<K>(seed, n0 + a + i, round, offsets, list, a + i, peers);
  if (peers_out) {
#pragma unroll
    for (int j = 0; j < K; ++j) peers_out[(size_t)i * K + j] = (empty >> j) & 1u ? -1 : (int32_t)peers[j];
  }
  if (lost_out) {
    const uint32_t lost = lost_mask<K>(seed, n0 + a + i, round, threshold, responding, peers, empty);
#pragma unroll
    for (int j = 0; j < K; ++j) lost_out[(size_t)i * K + j] = (uint8_t)((lost >> j) & 1u);
  }
}

template <int K>
hipError_t launch_sample_listed_k(uint64_t seed, uint32_t n0, uint32_t a, uint32_t b, uint32_t round,
                                  const uint32_t* offsets, const uint32_t* list, uint32_t threshold,
                                  const uint32_t* responding, int32_t* peers_out, uint8_t* lost_out, hipStream_t s) {
  const uint32_t n = b - a;
  hipLaunchKernelGGL((k_sample_listed<K>), dim3((n + 255) / 256), dim3(256), 0, s, seed, n0, a, b, round, offsets,
                     list, threshold, responding, peers_out, lost_out);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_round_listed(const ListedParams& p, int k, bool neutral, hipStream_t s) {
  if (!p.l.lost || !p.unsent || !p.offsets || !p.list || !p.l.r.L) return hipErrorInvalidValue;
  return dispatch_k<kMaxK>(k, [&](auto K) { return launch_listed_k<K()>(p, neutral, s); });
}

hipError_t launch_sample_listed(uint64_t seed, uint32_t n0, uint32_t a, uint32_t b, uint32_t round, int k,
                                const uint32_t* offsets, const uint32_t* list, uint32_t loss_threshold,
                                const uint32_t* responding, int32_t* peers_out, uint8_t* lost_out, hipStream_t s) {
  if (b <= a) return hipSuccess;
  if (!offsets || !list) return hipErrorInvalidValue;
  return dispatch_k<kMaxK>(k, [&](auto K) {
    return launch_sample_listed_k<K()>(seed, n0, a, b, round, offsets, list, loss_threshold, responding, peers_out,
                                       lost_out, s);
  });
}

}  // namespace avk
