// The round with lost Responses and unresponsive nodes (rule R5) for CDNA4 (gfx950):
// k_round_lossy, one lane per 32-record block like k_round_fast (round_firstgen.hip), uncapped,
// k = 1..16, and k_sample_lost, the parity dump of its loss draw (av_sample_lost).
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

namespace avk {

namespace {
constexpr uint32_t kDomLoss = 6u;

// Bit j: the Response of slot j of `node` in `round` is lost: drawn lost, or its peer does not respond.
template <int K>
__device__ __forceinline__ uint32_t lost_mask(uint64_t seed, uint32_t node, uint32_t round, uint32_t threshold,
                                              const uint32_t* responding, const uint32_t (&peers)[K]) {
  uint32_t lost = 0u;
  if (threshold) {
#pragma unroll
    for (int blk = 0; blk < (K + 3) / 4; ++blk) {
      uint32_t x[4];
      philox(x, seed, node, round, (uint32_t)blk, kDomLoss);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (blk * 4 + i < K) lost |= (x[i] < threshold ? 1u : 0u) << (blk * 4 + i);
    }
  }
  if (responding) {
#pragma unroll
    for (int j = 0; j < K; ++j) lost |= (~(responding[peers[j] >> 5] >> (peers[j] & 31u)) & 1u) << j;
  }
  return lost;
}

// ---------------------------------------------------------------------------
// Body for one lane. `lost`: the node's lost mask (the same in every lane of a node).
// NEUTRAL = false: a lost slot registers nothing; its preference word is not gathered and its
//   vote_step does not run (the lanes of the node sit the slot out under the exec mask), so no
//   window shifts, no update is logged and nothing is applied; `alive` carries on, and an update
//   of a later slot carries its own slot index. A lane whose node lost all K Responses (`idle`)
//   reads only A and K7, republishes and stores no plane. WARM as in k_round_fast: every consider
//   plane of the wave's blocks is all-ones and stays so (a skipped vote shifts nothing).
// NEUTRAL = true: a lost slot registers err = 0x80000000 on every polled record: votes and
//   consider both shift in 0 (vote.go:55-56), it counts as applied and follows vote.go:58-75
//   literally (seven agreeing considered votes around it still conclude). Never WARM.
// ---------------------------------------------------------------------------
template <int K, bool NEUTRAL, bool WARM, bool NT>
__device__ __forceinline__ void round_lossy_body(const LossyParams& lp, uint32_t g, uint32_t lane, bool active,
                                                 uint32_t b, uint32_t node, bool polls, uint32_t lost,
                                                 const uint32_t (&peers)[K]) {
  static_assert(!(NEUTRAL && WARM), "a neutral vote shifts in consider = 0");
  const RoundParams& p = lp.r;
  constexpr uint32_t kAll = K >= 32 ? ~0u : (1u << K) - 1u;
  const bool idle = !NEUTRAL && active && lost == kAll;  // every Response lost: no plane changes
  const bool work = active && !idle;
  St s;
  uint32_t* const tile = tile_of(p.planes, g);
  u32x4* const grp = reinterpret_cast<u32x4*>(tile) + lane;  // V0-3, V4-7, K0-3, K4-7 at +0, +64, +128, +192
  dead_state(s);
  if (work) {
    const u32x4 v0 = pld4<NT>(grp), v1 = pld4<NT>(grp + 64), k0 = pld4<NT>(grp + 128), k1 = pld4<NT>(grp + 192);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.V[i] = v0[i];
      s.V[4 + i] = v1[i];
      s.K[i] = k0[i];
      s.K[4 + i] = k1[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s.C[i] = WARM ? ~0u : pld<NT>(tile + plane_off(kPC + i, lane));
    s.A = pld<NT>(tile + plane_off(kPA, lane));
  } else if (idle) {
    s.A = pld<NT>(tile + plane_off(kPA, lane));
    s.K[7] = pld<NT>(tile + plane_off(kPK + 7, lane));
  }

  uint32_t w[K];
#pragma unroll
  for (int j = 0; j < K; ++j)
    w[j] = work && !((lost >> j) & 1u) ? p.pref_in[(size_t)peers[j] * p.PS + b] : 0u;
  const uint32_t vmask = work ? p.valid[b] : 0u;
  const uint32_t live0 = ~s.K[7];
  const uint32_t P0 = polls ? live0 & vmask : 0u;  // (idle lanes: vmask = 0, nothing polled)

  uint32_t alive = P0, applied = 0, E[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const bool gone = (lost >> j) & 1u;
    E[j] = 0u;
    if (NEUTRAL || !gone) {
      applied += __popc(alive);
      uint32_t fin;
      vote_step<false>(s, w[j], NEUTRAL && gone ? 0u : ~0u, alive, E[j], fin);
      alive &= ~fin;
    }
  }
  const uint32_t died = P0 & ~alive;
  const uint32_t keep = live0 & ~P0;  // live but !IsValid() (processor.go:101-103) or not polling: untouched
  if (p.died_out && active) p.died_out[g] = died;

  if (work) {
    uint32_t Vo[8], Co[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) Vo[i] = Co[i] = 0u;
    if (keep) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        Vo[i] = tile[plane_off(kPV + i, lane)];
        if (!WARM) Co[i] = tile[plane_off(kPC + i, lane)];
      }
    }
    const uint32_t dead = ~(alive | keep);
    u32x4 v0, v1, k0, k1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v0[i] = (s.V[i] & alive) | (Vo[i] & keep);
      v1[i] = (s.V[4 + i] & alive) | (Vo[4 + i] & keep);
      k0[i] = s.K[i];
      k1[i] = s.K[4 + i];
    }
    pst4<NT>(grp, v0);
    pst4<NT>(grp + 64, v1);
    pst4<NT>(grp + 128, k0);
    pst4<NT>(grp + 192, k1);
    if (!WARM) {  // WARM: consider planes stay all-ones (dead records are canonical all-ones too)
#pragma unroll
      for (int i = 0; i < 8; ++i) pst<NT>(tile + plane_off(kPC + i, lane), (s.C[i] & alive) | (Co[i] & keep) | dead);
    }
    pst<NT>(tile + plane_off(kPA, lane), s.A);
  }
  if (active)  // (the snapshot buffers rotate: a lane that changed nothing still publishes its word)
    p.pref_out[(size_t)node * p.PS + b] =
        is_byz(p.byz, node) ? byz_pattern(p.round + 1u) : publish_word(s.A, s.K[7], p.pub_mode);

  const uint32_t wave_id = g >> 6;
  uint32_t upd = 0;
  const uint32_t emitted = emit_updates<K>(p, wave_id, lane, node, p.t0 + b * 32u, E, s.A, died, upd);
  // model bytes of this lane: the planes read and written, a word per Response gathered, the
  // published word; an idle lane: A, K7 and the published word
  constexpr uint32_t plane_bytes = WARM ? (18u + 17u) * 4u : 2u * kPlanes * 4u;
  const uint32_t nlost = (uint32_t)__popc(lost & kAll);
  const uint32_t mine = work ? plane_bytes + 4u * ((uint32_t)K - nlost) + 4u : idle ? 12u : 0u;
  count_stats(p, wave_id, lane, applied, active, 0u, emitted + wave_sum(mine), upd, died);
  // lost Responses, once per (node, slot): the lane of the node's first block counts them
  const uint32_t nl_sum = wave_sum(active && polls && b == 0u ? nlost : 0u);
  if (lane == 0 && nl_sum) atomicAdd(&lp.lost[wave_id % p.log_shards], (unsigned long long)nl_sum);
}

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
