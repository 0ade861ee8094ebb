// The sweep kernel's general tile (k_round_sweep, sweep_kernel.h): what a 64-lane tile loads (TileIn,
// load_tile), the peer draws a wave's run shares (WaveDraw), a lane's indices (lane_idx) and the round
// step (process_tile). Included by the sweep translation units only.
// Build knobs read here: AVK_ABLATE_PHASE (load_tile, process_tile) and AVK_PUB_PRELOAD (process_tile).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "round_common.h"
#include "round_slots.h"
#include "sweep_publish.h"

// The build knobs' defaults (described in round_sweep.hip, which sets them before its includes), so that
// the header stands alone
#ifndef AVK_ABLATE_PHASE
#define AVK_ABLATE_PHASE 0
#endif
#ifndef AVK_PUB_PRELOAD
#define AVK_PUB_PRELOAD 0
#endif

namespace avk {
namespace {

constexpr bool kAblatePhase = AVK_ABLATE_PHASE != 0;

// Everything one 64-lane tile loads before its round step: the state planes
// (vote.go:25-29; V0-7 and K0-7 as dwordx4 groups, A, C0-7 unless warm), the
// validity word, the node's Byzantine word, and the k vote words (replayed
// planes, or the peers' published preference words). Split from the step so
// that a wave can issue tile t + stride's loads before it computes tile t.
template <int K, bool REPLAY, bool WARM>
struct TileIn {
  u32x4 v0, v1, k0, k1;
  uint32_t A, vmask, byzw;
  uint32_t stale;                // wave-uniform: V planes stale, v0/v1 regathered (kernels.h vstale & kVMask)
  uint32_t cflag;                // wave-uniform: vstale & kCAll (consider planes virtual, all-ones); and the
                                 // word's kVCalm bit as stored, so that the tile's new word is compared with it
  uint32_t kw;                   // wave-uniform: kpend[tile] (kernels.h klazy); K planes not loaded if all-live
  uint32_t C[WARM ? 1 : 8];
  uint32_t uref;                 // uniform rows (p.uni_out): ref_node's word of pref_in for the lane's block
  uint32_t old;                  // always 0 (was a retired variant's prefetched word): removing the field moves w
                                 // and cw and reorders the pipelined kernels' loop set-up; it goes with their next change
                                 // (as sensitive: one helper for the `p.lean && p.settled_fast && p.klazy && p.vv` gate
                                 // was tried, changed the twelve warm k = 8 kernels, the headline one 94 -> 95 VGPRs, and was left out)
  uint32_t w[K];                 // yes bits: err == 0 (vote.go:55)
  uint32_t cw[REPLAY ? K : 1];   // consider bits: int32(err) >= 0 (vote.go:56); sim votes: all-ones
};

// The peer draws of a wave's run of consecutive tiles, made once for the
// whole run (kModeWarm with p.tpw, k = 8): `pair` = round - 1's and round's
// draws (some tile of the run is kVStale), else round's only; `ok` = the
// run's nodes fit the producer lanes (otherwise every tile draws its own).
struct WaveDraw {
  // the draws parked in LDS (round_slots.h park_draw): node rel of the run has its 8 candidates at
  // sdc + rel * 8 (this round) and sdp + rel * 8 (round - 1, if pair); badc / badp: the draws'
  // repeated-candidate ballots, bit rel * 2 (and rel * 2 + 1) for node rel
  const uint32_t* sdc;
  const uint32_t* sdp;
  unsigned long long badc, badp;
  uint32_t fofs;  // REF: bit offset of this round's producer lanes in flagok (32 in the paired layout)
  uint32_t nlA, t0, nn;
  // REF: producer lane q's 4 candidates all carry pref_in's reference-row tag (bit q): a node's 8
  // peers are flagged iff both of its producer lanes' bits are set
  unsigned long long flagok;
  uint32_t meta;  // lane i: tile t0 + i's vstale << 8 | kpend & (kPendAllLive | 0xFF)
  bool pair, ok;
};

__device__ __forceinline__ uint32_t meta_of(const WaveDraw& wd, uint32_t tile) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wd.meta, (int)(tile - wd.t0));
}

// word at a 32-bit byte offset from a wave-uniform base (SGPR base + VGPR
// offset addressing: one VALU add per gather instead of a 64-bit multiply-add)
__device__ __forceinline__ uint32_t at_byte(const uint32_t* base, uint32_t off) {
  return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(base) + off);
}

struct LaneIdx {
  uint32_t g, gc, nl, b, node;
  bool active;
};

__device__ __forceinline__ LaneIdx lane_idx(const RoundParams& p, uint32_t tile, uint32_t lane) {
  LaneIdx x;
  x.g = tile * 64u + lane;
  x.active = x.g < p.L;
  x.gc = x.active ? x.g : p.L - 1u;  // inactive lanes read a valid lane, never store
  x.nl = div_bl(p, x.gc);
  x.b = x.gc - x.nl * p.BL;
  x.node = p.n0 + x.nl;
  return x;
}

constexpr uint32_t kUniVotes = 1u, kUniPrev = 2u;
// uflags (p.uni_votes; the warm k = 8 sweep only), kernel-uniform:
//  * kUniVotes: the input snapshot is uniform (kernels.h uni_in): every row of pref_in is the
//    reference row of pref_prev, so each of the 8 votes a lane would gather is that row's word for
//    its block: one load of it instead of 8 gathers (a klazy round whose tiles are not yet settled
//    candidates, e.g. C5's round 4 after the network converged);
//  * kUniPrev: pref_prev is uniform too (kernels.h uni_prev): a stale tile's vote register (last
//    round's 8 votes, gathered from pref_prev) is its reference row's word: no regather (the round
//    after, e.g. C4's and C5's round 5).
template <int K, bool REPLAY, bool WARM, int POL, bool ABLATE, bool VVM = false, bool FRESH = false, bool CC = true>
__device__ __forceinline__ void load_tile(const RoundParams& p, uint32_t tile, uint32_t lane,
                                          TileIn<K, REPLAY, WARM>& in, const WaveDraw* wd = nullptr,
                                          uint32_t uflags = 0u) {
  const LaneIdx x = lane_idx(p, tile, lane);
  const uint32_t* const tp = p.planes + (size_t)tile * (kPlanes * 64u);
  const u32x4* const grp = reinterpret_cast<const u32x4*>(tp) + lane;
  constexpr bool VV = VVM && WARM && !REPLAY && K == 8;  // VVM: the warm sim modes only
  const bool meta = VV && wd && wd->t0 <= tile && tile - wd->t0 < 64u && p.tpw;
  const uint32_t raw = VV && p.vv ? (meta ? (meta_of(*wd, tile) >> 8) & 0xFFu : uni(p.vstale[tile])) : 0u;
  in.stale = raw & kVMask;
  in.cflag = raw & (kCAll | kVCalm);
  in.kw = 0u;
  if constexpr (FRESH) {
    // NewVoteRecords (vote.go:33-35): votes, consider and count all zero; K7
    // marks the slots past the engine's last target (never added)
    const uint32_t rem = p.tn - x.b * 32u;
    const uint32_t real = rem >= 32u ? ~0u : ((1u << rem) - 1u);
    in.v0 = in.v1 = in.k0 = u32x4{0u, 0u, 0u, 0u};
    in.k1 = u32x4{0u, 0u, 0u, ~real};
#pragma unroll
    for (int i = 0; i < (WARM ? 1 : 8); ++i) in.C[i] = 0u;
  } else {
    if (!in.stale) {
      in.v0 = ld4<POL>(grp);
      in.v1 = ld4<POL>(grp + 64);
    }
    if constexpr (VV) {
      if (p.klazy || p.kconsume) in.kw = meta ? meta_of(*wd, tile) & (kPendAllLive | kHiVirt | 0xFFu) : uni(p.kpend[tile]);
    }
    if (kAblatePhase && VV && (p.ablate_phase & 2u)) {  // diagnostics: no K / A loads
      in.k0 = u32x4{lane, 0u, 0u, 0u};
      in.k1 = u32x4{0u, 0u, 0u, ~real_mask(p.tn, x.b)};
    } else if (!(in.kw & kPendAllLive) || !p.klazy) {
      in.k0 = ld4<POL>(grp + 128);
      if (in.kw & kHiVirt)  // the K4..K7 group is virtual (kernels.h kHiVirt)
        in.k1 = u32x4{0u, 0u, 0u, ~real_mask(p.tn, x.b)};
      else
        in.k1 = ld4<POL>(grp + 192);
    } else {
      in.k0 = u32x4{0u, 0u, 0u, 0u};
      in.k1 = u32x4{0u, 0u, 0u, 0u};
    }
    if constexpr (!WARM) {
#pragma unroll
      for (int i = 0; i < 8; ++i) in.C[i] = ld1<POL>(tp + 1024u + (uint32_t)i * 64u + lane);
    }
  }
  in.A = kAblatePhase && VV && (p.ablate_phase & 2u) ? (lane * 0x9E3779B9u) : ld1<POL>(tp + 1536u + lane);
  if (in.stale == kVUniform) {  // the vote register of every polled record = its accepted bit (kernels.h)
    in.v0 = u32x4{in.A, in.A, in.A, in.A};
    in.v1 = u32x4{in.A, in.A, in.A, in.A};
  }
  in.vmask = x.active ? p.valid[x.b] : 0u;
  in.byzw = p.byz[x.node >> 5];
  // loaded with the tile (an in-order vmcnt wait for it late in the step would also wait for the
  // step's plane stores)
  in.uref = p.uni_out ? p.pref_in[p.ref_node * p.PS + x.b] : 0u;
  in.old = 0u;
  if constexpr (REPLAY) {
    replay_load<K>(p.replay, x.gc, in.w, in.cw);
  } else {
    const uint32_t nlA = uni(x.nl), nn = (uint32_t)__builtin_amdgcn_readlane((int)x.nl, 63) - nlA + 1u;
    uint32_t peers[K];
    // the gathers address the preference table by 32-bit byte offsets (SGPR
    // base + VGPR offset: one add per gather): the engine runs the sweep only
    // for tables below 4 GiB (N * BL < 2^30)
    const uint32_t rb = p.PS * 4u, bo = x.b * 4u;
    uint32_t rows[K];  // byte offsets of the peers' rows
    bool drawn = false, have_rows = false;
    if constexpr (VV) {
      if (wd && wd->ok) {  // the wave's draws, made once for its run of tiles (implies off32)
        const uint32_t base = (x.nl - wd->nlA) * 2u;
        const bool nog = kAblatePhase && (p.ablate_phase & 1u);  // diagnostics: no gathers (votes from the row offsets)
        if (in.stale == kVStale && (uflags & kUniPrev)) {  // every regathered word is the reference word
          const uint32_t rp = at_byte(p.pref_prev, p.ref_node * rb + bo);
          in.v0 = u32x4{rp, rp, rp, rp};
          in.v1 = u32x4{rp, rp, rp, 0u};
        } else if (in.stale == kVStale) {
          uint32_t pp[K];
          pick_parked(p, wd->sdp, wd->badp, base, x.node, p.round - 1u, rb, pp);
#pragma unroll
          for (int i = 0; i < 4; ++i) in.v0[i] = nog ? pp[7 - i] * 0x9E3779B9u : at_byte(p.pref_prev, pp[7 - i] + bo);
#pragma unroll
          for (int i = 0; i < 3; ++i) in.v1[i] = nog ? pp[3 - i] * 0x9E3779B9u : at_byte(p.pref_prev, pp[3 - i] + bo);
          in.v1[3] = 0u;
        }
        pick_parked(p, wd->sdc, wd->badc, base, x.node, p.round, rb, rows);
        drawn = have_rows = true;
        if (nog) {
#pragma unroll
          for (int j = 0; j < K; ++j) in.w[j] = (rows[j] + bo) * 0x9E3779B9u;
          return;
        }
      } else if (in.stale == kVStale) {
        // the vote register after last round's 8 sim votes is those votes:
        // V_i = (previous round's slot 7 - i vote); V_7 is never read at k = 8
        const PairDraw pd = pair_draw(p, p.round, nlA, nn, lane);
        {
          uint32_t pp[K];
          pick_peers(p, pd, 0u, p.round, x.node, x.nl, nlA, nn, lane, pp);
#pragma unroll
          for (int i = 0; i < 4; ++i) in.v0[i] = p.pref_prev[pp[7 - i] * p.PS + x.b];
#pragma unroll
          for (int i = 0; i < 3; ++i) in.v1[i] = p.pref_prev[pp[3 - i] * p.PS + x.b];
          in.v1[3] = 0u;
        }
        pick_peers(p, pd, 1u, p.round, x.node, x.nl, nlA, nn, lane, peers);
        drawn = true;
      }
    }
    if (uflags & kUniVotes) {  // kernel-uniform: no draw of this round's peers, no gathers
      const uint32_t rw = at_byte(p.pref_prev, p.ref_node * rb + bo);
#pragma unroll
      for (int j = 0; j < K; ++j) in.w[j] = rw;
      return;
    }
    if (!drawn) draw_peers<K>(p, p.round, x.node, x.nl, nlA, nn, lane, peers);
    if (!have_rows) {
#pragma unroll
      for (int j = 0; j < K; ++j) rows[j] = (ABLATE ? x.node : peers[j]) * rb;
    }
    // ABLATE (timing diagnostics only, results invalid): the node's own row, coalesced
#pragma unroll
    for (int j = 0; j < K; ++j) in.w[j] = at_byte(p.pref_in, rows[j] + bo);
  }
}

// The round step of one loaded tile. WARM: consider planes all-ones (neither
// loaded nor stored; sim votes only). POL: plane-stream cache policy.
// CALM: the walking warm mode's tiles (kModeWarm), which may flag themselves kVCalm (kernels.h calm).
template <int K, bool REPLAY, bool WARM, int POL, bool VVM = false, bool REF = false, bool CC = true, bool CALM = false>
__device__ __forceinline__ void process_tile(const RoundParams& p, uint32_t tile, uint32_t lane,
                                             const TileIn<K, REPLAY, WARM>& in, uint32_t extra_bytes, SweepAcc& acc,
                                             uint32_t uflags = 0u) {
  const LaneIdx x = lane_idx(p, tile, lane);
  const bool active = x.active;
  const uint32_t b = x.b, node = x.node;
  // the node's Byzantine bit from the word loaded with the tile (a load of it here, after the plane
  // stores, made the wave wait for those stores: vmcnt counts in issue order)
  const bool nbyz = ((in.byzw >> (node & 31u)) & 1u) != 0u;
  uint32_t* const tp = p.planes + (size_t)tile * (kPlanes * 64u);
  u32x4* const grp = reinterpret_cast<u32x4*>(tp) + lane;
  const __amdgpu_buffer_rsrc_t tr = __builtin_amdgcn_make_buffer_rsrc(tp, 0, kPlanes * 64 * 4, kRsrcWord3);
  const u32x4 v0 = in.v0, v1 = in.v1;
  u32x4 k0 = in.k0, k1 = in.k1;
  uint32_t A = in.A;
  uint32_t C[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) C[i] = WARM ? ~0u : in.C[WARM ? 0 : i];
  const uint32_t vmask = in.vmask;

  // ---- ys/ns hold y/n of [V_6..V_0, w_0..w_{K-1}]
  constexpr bool SYM = WARM && !REPLAY;  // n == ~y everywhere: ns is never read
  uint32_t ys[7 + K], ns[7 + K], cwv[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t cw = REPLAY ? in.cw[REPLAY ? j : 0] : ~0u;
    const uint32_t yw = in.w[j] & cw;  // err == 0 implies considered
    ys[7 + j] = yw;
    ns[7 + j] = SYM ? 0u : ~yw & cw;
    cwv[j] = cw;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {  // old planes V_6..V_0
    const uint32_t vi = (6 - i) < 4 ? v0[6 - i] : v1[2 - i];
    ys[i] = WARM ? vi : (vi & C[6 - i]);
    ns[i] = SYM ? 0u : WARM ? ~vi : (~vi & C[6 - i]);
  }

  constexpr bool KL = VVM && WARM && !REPLAY && K == 8;  // deferred count planes possible (kernels.h klazy)
  const bool klazy = KL && p.klazy;                      // wave-uniform: no record can finalize this round
  const bool kcons = KL && p.kconsume;                   // wave-uniform: apply pending steps, defer nothing
  const bool kunread = klazy && (in.kw & kPendAllLive);  // K planes not loaded: live == valid
  const uint32_t live0 = kunread ? in.vmask : ~k1[3];    // K7 = no live record
  const uint32_t P0 = live0 & vmask;                     // polled: live and IsValid (processor.go:95-103)
  const uint32_t keep = active ? (live0 & ~vmask) : 0u;  // live but !IsValid: untouched (processor.go:101-103)

  // ---- the shift-register planes after K votes are final for every record
  // that survives the round: store them now (a record deleted this round is
  // rewritten below)
  // a warm sim wave with no live-but-invalid record leaves its V planes
  // unstored: next round (or av materialize) regathers them (kernels.h vv)
  bool virt = false;
  if constexpr (VVM && !REPLAY && K == 8) {
    virt = p.vv && __ballot(keep != 0u) == 0ull;
    if (virt && p.vv_uniform) {
      // uniform form only (narrow rows, BL < vv_min_bl): a tile leaves V unstored only if it is
      // settled this round (V = A next round, nothing to regather); the test is the settled test
      // below, made early (klazy rounds: no record is near 128)
      bool st = false;
      if constexpr (SYM) {
        if (klazy) {
          uint32_t agree = P0;
#pragma unroll
          for (int i = 0; i < 7 + K; ++i) agree &= ~(ys[i] ^ in.A);
          st = __ballot(agree != P0) == 0ull;
        }
      }
      virt = st;
    }
  }
  if (active && !virt) {
    u32x4 o0, o1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t vi = i < 4 ? v0[i] : v1[i - 4];
      const uint32_t vs = i < K ? ys[6 + K - i] : (i - K < 4 ? v0[i - K] : v1[i - K - 4]);
      const uint32_t vn = (vs & P0) | (vi & keep);
      if (i < 4)
        o0[i] = vn;
      else
        o1[i - 4] = vn;
    }
    st4<POL>(tr, grp, lane * 16u, o0);
    st4<POL>(tr, grp + 64, 1024u + lane * 16u, o1);
  }
  // fresh round with virtual vote planes: every consider bit of the tile is 1
  // after the 8 sim votes (C_i = P0 | dead0 with keep = 0): leave them unstored
  const bool cvirt = virt && !WARM && !REPLAY && p.fresh;
  if (!WARM && active && !cvirt) {  // consider planes
    const uint32_t dead0 = ~(P0 | keep);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t cs = i < K ? cwv[K - 1 - i] : C[i - K];
      st1<POL>(tr, tp + 1024u + (uint32_t)i * 64u + lane, (1024u + (uint32_t)i * 64u + lane) * 4u,
               (cs & P0) | (C[i] & keep) | dead0);
    }
  }

  uint32_t Kp[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    Kp[i] = k0[i];
    Kp[4 + i] = k1[i];
  }
  if (kcons && (in.kw & 0xFFu)) {  // pending +8 steps on the polled records: pend added to count bits 3..6
    const uint32_t pend = in.kw & 0xFFu;
    uint32_t cy = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t bi = ((pend >> i) & 1u) ? P0 : 0u;
      const uint32_t t = Kp[3 + i] ^ bi;
      const uint32_t si = t ^ cy;
      cy = (t & cy) | (Kp[3 + i] & bi);
      Kp[3 + i] = si;
    }
  }
  uint32_t E[K], alive = P0, applied = 0u, c[4] = {0u, 0u, 0u, 0u}, F = 0u;
  const uint32_t low3[3] = {Kp[0], Kp[1], Kp[2]};
  constexpr bool KLZ_ABLATE = VVM && WARM && !REPLAY && K == 8;  // the warm general tiles (ablate_phase)
  // count >= 120: may reach 128 (K <= 8); never in a klazy round (engine bound)
  const uint32_t nearfin = klazy ? 0u : P0 & Kp[6] & Kp[5] & Kp[4] & Kp[3];
  const bool det = __ballot(nearfin != 0u) != 0ull;
  const uint32_t A_in = A;
  // Settled tiles (warm sim votes, K == 8, no record near 128): when every
  // polled record's 7 old votes and 8 new votes all agree with its accepted
  // bit, every 8-vote window of the round is unanimous, so each slot is a
  // conclusive agreeing vote (vote.go:58-69: confidence += 2, no flip, no
  // StatusUpdate) and the slot network can be skipped: c = 8, F = 0.
  bool settled = false;
  if constexpr (SYM && K == 8) {
    if (!det) {
      uint32_t agree = P0;
#pragma unroll
      for (int i = 0; i < 7 + K; ++i) agree &= ~(ys[i] ^ A);
      settled = __ballot(agree != P0) == 0ull;
    }
  }
  // Calm tiles (kernels.h calm): the tile leaves V unstored and is not settled. Next round's V6..V0
  // are this round's slots 1..7: on the polled records, x_j = "slot j agrees with A", at most one
  // zero among the 7 (round_slots.h Agg2), one ballot for the tile. The conservative form: a tile
  // in which any record flips this round is not calm (exact), so the bound is taken here, against
  // A_in and before the slot network, while the vote words are live anyway (taken after it, it kept
  // six of them in registers across the network and cost every general tile). A tile holding a
  // record whose slots 1 and 2 both disagree is out after 4 instructions: every tile of a storm.
  bool calm_pre = false;
  if constexpr (CALM && KL && SYM) {
    if (p.calm && klazy && virt && !settled && __ballot(((ys[8] ^ A) & (ys[9] ^ A) & P0) != 0u) == 0ull) {
      Agg2 g{~(ys[8] ^ A), ~0u};
#pragma unroll
      for (int j = 2; j < 8; ++j) agg_push(g, ~(ys[7 + j] ^ A));
      calm_pre = __ballot((~g.z1 & P0) != 0u) == 0ull;
    }
  }
  if (settled) {
#pragma unroll
    for (int j = 0; j < K; ++j) E[j] = 0u;
    c[3] = P0;
    applied = 8u * (uint32_t)__popc(P0);
  } else if (kAblatePhase && KLZ_ABLATE && (p.ablate_phase & 16u)) {  // diagnostics: no slot network
#pragma unroll
    for (int j = 0; j < K; ++j) E[j] = 0u;
    c[3] = P0;
    applied = 8u * (uint32_t)__popc(P0);
  } else {
    round_slots<K, SYM>(ys, ns, low3, nearfin, det, alive, A, E, c, F, applied);
  }
  // Calm tiles, second half: no record of the tile flipped in the slot network, so the bound taken
  // against A_in above holds against the round's final A.
  const bool calm = calm_pre && __ballot((F & P0) != 0u) == 0ull;
  // deferred count planes: every polled record agreed on all 8 votes (no flip,
  // c == 8) -> K stays as stored and the tile's pending +8 steps grow by one
  bool kdefer = false;
  uint32_t pend = 0u;
  if constexpr (KL) {
    if (klazy) {
      const uint32_t c8 = c[3] & ~(c[0] | c[1] | c[2]);
      const bool lane_uniform = !active || (((F & P0) | (~c8 & P0)) == 0u);
      kdefer = __ballot(!lane_uniform) == 0ull;
      pend = in.kw & 0xFFu;
      if (!kdefer) {
        if (kunread) {  // late load: the tile leaves the deferred state
          k0 = ld4<POL>(reinterpret_cast<const u32x4*>(tp) + lane + 128);
          k1 = in.kw & kHiVirt ? u32x4{0u, 0u, 0u, ~real_mask(p.tn, b)}
                               : ld4<POL>(reinterpret_cast<const u32x4*>(tp) + lane + 192);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            Kp[i] = k0[i];
            Kp[4 + i] = k1[i];
          }
        }
        // true count = K + 8 * pend on the polled records: add pend to planes 3..6
        uint32_t cy = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t bi = ((pend >> i) & 1u) ? P0 : 0u;
          const uint32_t t = Kp[3 + i] ^ bi;
          const uint32_t si = t ^ cy;
          cy = (t & cy) | (Kp[3 + i] & bi);
          Kp[3 + i] = si;
        }
      }
    }
  }
  // count_new = F ? c : count + c on planes 0..6 (survivors stay <= 127); deleted: count 128 (K7 set)
  const uint32_t died = P0 & ~alive;
  // StatusUpdate log reservation (k = 8) before this tile's plane and published-word stores, so that
  // reading the atomics' results waits for them alone, not for those stores (round_common.h)
  EmitRes er{};
  if constexpr (K == 8) er = emit_reserve_med<K>(p, acc.shard, lane, E, died, acc.updates);
  {
    uint32_t cy = 0u;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const uint32_t ci = i < 4 ? c[i] : 0u;
      const uint32_t t = Kp[i] ^ ci;
      const uint32_t si = t ^ cy;
      cy = (t & cy) | (Kp[i] & ci);
      Kp[i] = ((F & ci) | (~F & si)) & ~died;
    }
    Kp[7] |= died;
  }

  // klazy rounds: a tile whose A plane did not change does not rewrite it
  const bool astore = !klazy || __ballot(active && A != A_in) != 0ull;
  // the K4..K7 group stays virtual (kernels.h kHiVirt) while every count is < 16 and nothing was
  // deleted: set by the fresh round, kept by klazy rounds (deferred tiles leave K as it is)
  bool hv = false;
  if (K == 8 && p.hivirt && ((!WARM && p.fresh) || (klazy && (in.kw & kHiVirt))))
    hv = kdefer || __ballot(active && ((Kp[4] | Kp[5] | Kp[6] | died) != 0u)) == 0ull;
  if (active && !(kAblatePhase && KLZ_ABLATE && (p.ablate_phase & 4u))) {
    const bool known = kdefer && pend >= 2u;  // (publish)
    PubPre pre{0u, 0u, 0u, false};
    if (AVK_PUB_PRELOAD && CC && p.count_changed && !known) pre = publish_loads(p, node * p.PS + b, node - p.n0);
    if (!kdefer) {
      u32x4 o2, o3;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o2[i] = Kp[i];
        o3[i] = Kp[4 + i];
      }
      st4<POL>(tr, grp + 128, 2048u + lane * 16u, o2);
      if (!hv) st4<POL>(tr, grp + 192, 3072u + lane * 16u, o3);
    }
    if (astore) st1<POL>(tr, tp + 1536u + lane, (1536u + lane) * 4u, A);
    const uint32_t prow = node * p.PS + b;  // < N * PS < 2^31
    const uint32_t pub = nbyz ? byz_pattern(p.round + 1u) : A;
    if (p.uni_out) acc.umis |= pub != in.uref ? 1u : 0u;  // uniform rows (kernels.h)
    publish<POL, CC>(p, prow, pub, nbyz ? byz_pattern(p.round - 2u) : pub, acc, known, node - p.n0, acc.qslot, &pre);
    // a record deleted this round keeps the vote/consider planes stored
    // above: K7 marks it dead, every reader masks by K7 (k_read_records,
    // k_add_targets resets all planes) and the next round's store zeroes them
  }
  if (REF && p.rflag_out && settled) {  // reference-row flag of the row a settled tile just published
    ref_flag_store(p, lane, active, b, node, nbyz ? byz_pattern(p.round + 1u) : A,
                   p.pref_in[p.ref_node * p.PS + (active ? b : 0u)]);
    if (active) acc.lane_bytes += 4u + (b == 0u ? 1u : 0u);
  }
  if constexpr (VVM && !REPLAY && K == 8) {
    // a settled tile's 8 new votes all equal its accepted plane on the polled
    // records: its vote register is A next round (no regather)
    // (preset consider planes, kernels.h c_preset: memory already holds what kCAll stands for)
    const uint32_t nv = (virt ? (settled ? kVUniform : kVStale) : 0u) | (in.cflag & kCAll) |
                        (cvirt && !p.c_preset ? kCAll : 0u) | (calm ? kVCalm : 0u);
    if (p.vv && lane == 0 && nv != (in.stale | in.cflag)) p.vstale[tile] = nv;
  }
  if constexpr (KL) {
    if (klazy) {
      // live records == valid targets in every lane (no live-but-invalid record):
      // the next round need not read K to find the polled set
      const bool all_live = __ballot(active && live0 != vmask) == 0ull;
      const uint32_t kw = (kdefer ? pend + 1u : 0u) | (all_live ? kPendAllLive : 0u) | (hv ? kHiVirt : 0u);
      if (lane == 0 && kw != in.kw) p.kpend[tile] = kw;
      if (lane == 0) acc.lane_bytes += kw != in.kw ? 8u : 4u;  // kpend word read (+ written)
    } else if (kcons) {
      if (lane == 0 && in.kw) p.kpend[tile] = 0u;
      if (lane == 0) acc.lane_bytes += in.kw ? 8u : 4u;
    }
  }
  if constexpr (!WARM && !REPLAY && K == 8) {  // the fresh round starts the tile's virtual K4..K7 group
    if (hv && lane == 0) {
      p.kpend[tile] = kHiVirt;
      acc.lane_bytes += 4u;
    }
  }
  // k = 8: single words, medium and dense records, one contiguous entry per lane (round_common.h)
  uint32_t emitted;
  if constexpr (K == 8)
    emitted = emit_store_med<K>(p, acc.shard, lane, node, p.t0 + b * 32u, E, A, died, er, p.round_rel);
  else
    emitted = emit_updates<K>(p, tile, lane, node, p.t0 + b * 32u, E, A, died, acc.updates);

  // fresh (p.fresh, cold template): no plane is read but A (96 B fewer)
  constexpr uint32_t plane_bytes = WARM ? 2u * 17u * 4u : 2u * kPlanes * 4u;
  const uint32_t lane_bytes = plane_bytes + (REPLAY ? 8u : 4u) * K + 4u - (!WARM && p.fresh ? 96u : 0u);
  acc.applied += applied;
  acc.died += (uint32_t)__popc(died);
  // stale: 7 regathered words instead of the 8 V planes read; virt: V planes not written
  // push: + the 4-B read of the word being overwritten
  // kl: K planes neither read (kunread and deferred) nor written (deferred); A not rewritten
  const uint32_t kbytes = (kunread && kdefer ? 32u : 0u) + (kdefer ? 32u : 0u) +
                          // virtual K4..K7 group (kHiVirt): not read (if K was read), not written
                          (WARM && (in.kw & kHiVirt) && !(kunread && kdefer) ? 16u : 0u) + (hv && !kdefer ? 16u : 0u);
  // V read: 32 B stored, 28 B regathered (stale), 0 B uniform
  // uflags: one 4-B reference word read instead of the K gathered votes / the 7 regathered ones
  acc.lane_bytes += active ? lane_bytes + extra_bytes - (in.stale == kVStale ? 4u : in.stale == kVUniform ? 32u : 0u) -
                                 (virt ? 32u : 0u) - (cvirt ? 32u : 0u) + (p.count_changed ? 4u : 0u) -
                                 kbytes - (astore ? 0u : 4u) - ((uflags & kUniVotes) ? 4u * K - 4u : 0u) -
                                 (in.stale == kVStale && (uflags & kUniPrev) ? 24u : 0u)
                           : 0u;
  acc.emitted_bytes += emitted;
  // sim rounds gather 8 peer words per lane (each word of the round-start snapshot is gathered by
  // ~k lanes: 28 of the 32 B re-read), stale tiles 7 more from the previous snapshot (24 B re-read)
  if constexpr (!REPLAY)
    acc.reread += active ? ((uflags & kUniVotes) ? 4u : 4u * K - 4u) +
                               (in.stale == kVStale ? ((uflags & kUniPrev) ? 4u : 24u) : 0u)
                         : 0u;
}

}  // namespace
}  // namespace avk
