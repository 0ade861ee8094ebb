// What k_round_lossy (round_lossy.hip, rule R5) and k_round_listed (round_listed.hip, rule R6) share:
// the lost mask of a node's k slots and the body of one lane over its 32-record block.
// LISTED = false instantiates what round_lossy.hip held before the split: every `none` below is a
// compile-time 0 and folds away.
#pragma once

#include "kernels.h"
#include "round_common.h"

namespace avk {

constexpr uint32_t kDomLoss = 6u;

// Bit j: the Response of slot j of `node` in `round` is lost: drawn lost, or its peer does not respond.
// none: slots that poll nobody (R6: no query went out, so nothing is lost; their peers[] entry is
// never used as an index).
template <int K>
__device__ __forceinline__ uint32_t lost_mask(uint64_t seed, uint32_t node, uint32_t round, uint32_t threshold,
                                              const uint32_t* responding, const uint32_t (&peers)[K],
                                              uint32_t none = 0u) {
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
    for (int j = 0; j < K; ++j)
      if (!((none >> j) & 1u)) lost |= (~(responding[peers[j] >> 5] >> (peers[j] & 31u)) & 1u) << j;
  }
  return lost & ~none;
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
// LISTED: `empty` holds the node's empty slots (R6; disjoint from `lost`). An empty slot is sat out
//   like a skipped one in either loss mode, is no lost Response, and is counted into `unsent` once
//   per (polling node, slot). A lane whose every slot is empty or skipped is idle in either mode.
// ---------------------------------------------------------------------------
template <int K, bool NEUTRAL, bool WARM, bool NT, bool LISTED = false>
__device__ __forceinline__ void round_lossy_body(const LossyParams& lp, uint32_t g, uint32_t lane, bool active,
                                                 uint32_t b, uint32_t node, bool polls, uint32_t lost,
                                                 const uint32_t (&peers)[K], uint32_t empty = 0u,
                                                 unsigned long long* unsent = nullptr) {
  static_assert(!(NEUTRAL && WARM), "a neutral vote shifts in consider = 0");
  const RoundParams& p = lp.r;
  constexpr uint32_t kAll = K >= 32 ? ~0u : (1u << K) - 1u;
  const uint32_t none = LISTED ? empty & kAll : 0u;     // no query goes out
  const uint32_t out = NEUTRAL ? none : lost | none;    // slots that register nothing
  // every slot sat out: no plane changes
  const bool idle = (LISTED || !NEUTRAL) && active && out == kAll;
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
    w[j] = work && !(((lost | none) >> j) & 1u) ? p.pref_in[(size_t)peers[j] * p.PS + b] : 0u;
  const uint32_t vmask = work ? p.valid[b] : 0u;
  const uint32_t live0 = ~s.K[7];
  const uint32_t P0 = polls ? live0 & vmask : 0u;  // (idle lanes: vmask = 0, nothing polled)

  uint32_t alive = P0, applied = 0, E[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const bool gone = (lost >> j) & 1u;
    const bool sent = !((none >> j) & 1u);
    E[j] = 0u;
    if (sent && (NEUTRAL || !gone)) {
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
  // published word; an idle lane: A, K7 and the published word. LISTED: every active lane also reads
  // its node's two offsets and one list entry per slot that is not empty.
  constexpr uint32_t plane_bytes = WARM ? (18u + 17u) * 4u : 2u * kPlanes * 4u;
  const uint32_t nlost = (uint32_t)__popc(lost & kAll);
  const uint32_t nnone = (uint32_t)__popc(none);
  const uint32_t drawn = LISTED && active ? 8u + 4u * ((uint32_t)K - nnone) : 0u;
  const uint32_t mine = (work ? plane_bytes + 4u * ((uint32_t)K - nlost - nnone) + 4u : idle ? 12u : 0u) + drawn;
  count_stats(p, wave_id, lane, applied, active, 0u, emitted + wave_sum(mine), upd, died);
  // lost Responses, once per (node, slot): the lane of the node's first block counts them
  const uint32_t nl_sum = wave_sum(active && polls && b == 0u ? nlost : 0u);
  if (lane == 0 && nl_sum) atomicAdd(&lp.lost[wave_id % p.log_shards], (unsigned long long)nl_sum);
  if constexpr (LISTED) {  // and the polls that were never sent
    const uint32_t ns_sum = wave_sum(active && polls && b == 0u ? nnone : 0u);
    if (lane == 0 && ns_sum) atomicAdd(&unsent[wave_id % p.log_shards], (unsigned long long)ns_sum);
  }
}

}  // namespace avk
