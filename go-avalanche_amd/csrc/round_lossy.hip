// The round with lost Responses and unresponsive nodes (rule R5) for CDNA4 (gfx950):
// k_round_lossy, one lane per 32-record block like k_round_fast (round_firstgen.hip), uncapped,
// k = 1..16, and k_sample_lost, the parity dump of its loss draw (av_sample_lost). The lost mask and
// the lane's body stand in round_lossy_body.h, which the round over peer lists (round_listed.hip,
// rule R6) shares; this unit instantiates them with LISTED = false.
//
// The reference has two behaviours that a perfect network never shows. RegisterVotes returns
// before it reads a vote when the query is unknown or expired (processor.go:66-76,
// AvalancheRequestTimeout avalanche.go:19-21): with that check disabled, a Response that does not
// arrive is a RegisterVotes call that never happens (AV_LOSS_SKIP). And a vote with a negative err
// shifts consider = 0 into the window (vote.go:55-56): a Response from a peer that cannot answer
// (AV_LOSS_NEUTRAL). Which Responses are lost depends on (seed, node, round, slot) and on the
// peer alone, never on the target: target shards agree with the whole network with no exchange.
//
// Like its model the kernel streams the record planes once; next to it a lane makes ceil(K/4) more
// Philox calls (the node's lost mask) and one L2-resident word load per slot (the peer's bit of the
// responding bitset), and does not gather the preference word of a lost slot. Measured at C4 with
// 10 % loss (profiles/r13): neutral mode runs at 1.04x the first-generation round
// that moves the same planes, skip mode at 1.24x of its warm form while moving fewer bytes, so
// skip mode is not bound by HBM traffic. Skip mode differs from neutral mode in two places: each
// gather sits under the per-node lost mask, and each slot's vote_step sits in a branch on that
// mask, which diverges wherever two nodes share a wave (BL <= 32): up to K divergent regions per
// wave in place of straight-line code. The issue describes the lost slot as a vote_step with an
// empty step mask; the branch gives the same records (vote_step has no cross-lane operation) and
// was taken to save the masked form's bfi per plane. That these two are what the 24 % pays for
// is a supposition from the code: no profile has separated them yet.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "round_common.h"
#include "round_lossy_body.h"

namespace avk {

namespace {
template <int K, bool NEUTRAL>
__global__ __launch_bounds__(256) void k_round_lossy(const LossyParams lp) {
  const RoundParams& p = lp.r;
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
  sample_peers<K>(p.seed, node, p.round, p.n_nodes, p.peer_mode, peers);
  const uint32_t lost = lost_mask<K>(p.seed, node, p.round, lp.loss_threshold, lp.responding, peers);
  if constexpr (!NEUTRAL) {
    if (p.warm_skip) {
      constexpr uint32_t kAll = (1u << K) - 1u;
      // (a lane that lost every Response touches no consider plane: it does not read C7 either)
      const uint32_t c7 = active && lost != kAll ? *pw(p.planes, g, kPC + 7) : ~0u;
      if (__all(c7 == ~0u)) {  // wave-uniform
        if (p.plane_nt)
          round_lossy_body<K, false, true, true>(lp, g, lane, active, b, node, polls, lost, peers);
        else
          round_lossy_body<K, false, true, false>(lp, g, lane, active, b, node, polls, lost, peers);
        return;
      }
    }
  }
  if (p.plane_nt)
    round_lossy_body<K, NEUTRAL, false, true>(lp, g, lane, active, b, node, polls, lost, peers);
  else
    round_lossy_body<K, NEUTRAL, false, false>(lp, g, lane, active, b, node, polls, lost, peers);
}

template <int K>
hipError_t launch_lossy_k(const LossyParams& p, bool neutral, hipStream_t s) {
  const uint32_t blocks = (p.r.Lpad + 255u) / 256u;
  if (neutral)
    hipLaunchKernelGGL((k_round_lossy<K, true>), dim3(blocks), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL((k_round_lossy<K, false>), dim3(blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

template <int K>
__global__ void k_sample_lost(uint64_t seed, uint32_t n_nodes, uint32_t a, uint32_t b, uint32_t round, int mode,
                              uint32_t threshold, const uint32_t* responding, uint8_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (a + i >= b) return;
  uint32_t peers[K];
  sample_peers<K>(seed, a + i, round, n_nodes, mode, peers);
  const uint32_t lost = lost_mask<K>(seed, a + i, round, threshold, responding, peers);
#pragma unroll
  for (int j = 0; j < K; ++j) out[(size_t)i * K + j] = (uint8_t)((lost >> j) & 1u);
}

template <int K>
hipError_t launch_sample_lost_k(uint64_t seed, uint32_t n_nodes, uint32_t a, uint32_t b, uint32_t round, int mode,
                                uint32_t threshold, const uint32_t* responding, uint8_t* out, hipStream_t s) {
  const uint32_t n = b - a;
  hipLaunchKernelGGL((k_sample_lost<K>), dim3((n + 255) / 256), dim3(256), 0, s, seed, n_nodes, a, b, round, mode,
                     threshold, responding, out);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_round_lossy(const LossyParams& p, int k, bool neutral, hipStream_t s) {
  if (!p.lost || !p.r.L) return hipErrorInvalidValue;
  return dispatch_k<kMaxK>(k, [&](auto K) { return launch_lossy_k<K()>(p, neutral, s); });
}

hipError_t launch_sample_lost(uint64_t seed, uint32_t n_nodes, uint32_t a, uint32_t b, uint32_t round, int k,
                              int mode, uint32_t loss_threshold, const uint32_t* responding, uint8_t* out,
                              hipStream_t s) {
  if (b <= a) return hipSuccess;
  return dispatch_k<kMaxK>(k, [&](auto K) {
    return launch_sample_lost_k<K()>(seed, n_nodes, a, b, round, mode, loss_threshold, responding, out, s);
  });
}

}  // namespace avk
