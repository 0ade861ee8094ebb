// The persistent streaming round kernel k_round_sweep (the header comment of round_sweep.hip describes
// it), its modes, its launchers by mode, store policy and grid, and its occupancy query: templates on k,
// instantiated for k = 8 by round_sweep.hip and for k = 1..7 by round_sweep_lowk.hip.
// Build knobs read here: AVK_WARM_WPE, AVK_FRESH_WPE (below); the headers it includes read the others.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "round_common.h"
#include "round_plan.h"
#include "round_slots.h"
#include "sweep_publish.h"
#include "sweep_tile.h"
#include "sweep_settled.h"

namespace avk {
namespace {

enum : int { kModeWarm = 0, kModeCheck = 1, kModeReplay = 2, kModeAblate = 3, kModeWarmPipe = 4, kModeFresh = 5 };

// MODE: kModeWarm (sim, every consider plane all-ones), kModeCheck (sim, per
// tile: the oldest consider plane decides), kModeReplay (replayed votes),
// kModeAblate (kModeCheck with the peer gather replaced by a coalesced read of
// the node's own row: timing diagnostics only, results invalid), kModeWarmPipe
// (kModeWarm for a resident grid: the next tile's loads are issued before the
// current tile is computed; 93 VGPRs, 5 waves per SIMD).
// A/B build knob (Makefile variant libraries): the warm modes' waves per SIMD. Round 3: 6 (80 VGPRs,
// 7 spilled to scratch in cold paths) beat 5 (87 VGPRs) by 4 % (profiles/r03/ab_waves_per_simd.log).
// Round 4 (slot records, non-temporal log): 5 (92 VGPRs, none spilled) beats 6 (80, 8-9 spilled):
// C4p epoch -2.8 / -2.9 %, C4 -0.9 / -1.4 %, C4pb -1.1 %; 7 is 1.3x slower
// (profiles/r04/session13/abwpe.log; 4 compiles to the same code as 5)
#ifndef AVK_WARM_WPE
#define AVK_WARM_WPE 5
#endif
// (the fresh mode at 5 instead: round 0 -1 %, epochs within noise, profiles/r04/session15/abf5.log)
#ifndef AVK_FRESH_WPE
#define AVK_FRESH_WPE 6
#endif
template <int K, int MODE, int POL, bool REF = false, bool CC = true>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MODE == kModeWarmPipe ? 5 : MODE == kModeWarm ? AVK_WARM_WPE : MODE == kModeFresh ? AVK_FRESH_WPE : MODE == kModeReplay ? 6 : 7))) void k_round_sweep(const RoundParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = uni(blockIdx.x * 4u + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * 4u;
  const uint32_t tiles = p.Lpad >> 6;
  SweepAcc acc;
  acc.shard = wave0 & (p.log_shards - 1u);  // a power of two (engine.cpp set_log_layout)
  if constexpr (CC) {  // deferred pushes: the wave's queue (dynamic LDS, launched only with p.push_q)
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    const uint32_t w = threadIdx.x >> 6;
    acc.qpub = reinterpret_cast<uint32_t*>(s_dyn) + w * (kPushQ * 64u);
    acc.qpm = s_dyn + 4u * 4u * kPushQ * 64u + w * (kPushQ * 64u);
  }
  // the network-quiet word of the round before (kernels.h nq_in), requested with the uniform slots
  const uint32_t nqw = p.nq_in ? *p.nq_in : p.round;
  // uniform rows (kernels.h): no rank's slot of pref_in carries this round's tag
  bool uniform = p.uni_in != nullptr;
  if (uniform)
    for (uint32_t r = 0; r < p.uni_world; ++r) uniform = uniform && p.uni_in[r] != p.round;
  // (and of pref_prev: its slots carry round - 1's tag if a row of it differed)
  // prev_uni: whatever the uni_votes option says (the quiescent tiles need it too)
  bool prev_uni = uniform && p.uni_prev != nullptr && K == 8 && ((p.uni_votes && p.vv) || (!CC && p.quiet_tiles));
  if (prev_uni)
    for (uint32_t r = 0; r < p.uni_world; ++r) prev_uni = prev_uni && p.uni_prev[r] != p.round - 1u;
  const bool uniform_prev = prev_uni && p.uni_votes && p.vv;
  const uint32_t uflags = (K == 8 && uniform && p.uni_votes && p.vv ? kUniVotes : 0u) | (uniform_prev ? kUniPrev : 0u);
  // nq_tag: this wave owns tiles and some of them were not quiescent (kernels.h nq_out)
  bool nq_tag = wave0 < tiles;
  bool nq_taken = false;
  if constexpr (MODE == kModeWarm && K == 8 && !CC) {
    // Network-quiet round (sweep_settled.h "Network-quiet rounds"): every tile of the network is quiescent
    if (nqw != p.round && prev_uni && p.tpw && p.quiet_tiles && p.lean && p.settled_fast && p.klazy && p.vv) {
      const uint32_t G = min(max(p.nq_group, 1u), 16u), tpw = min(p.tpw, 16u);
      // the leaders: every G-th wave, or (p.nq_front) the grid's first waves, which are dispatched first
      // and work while the rest of the grid is dispatched and ends
      if (!p.nq_front && wave0 % G) return;
      const uint32_t t0 = (p.nq_front ? wave0 * G : wave0) * tpw;
      if (t0 >= tiles) return;
      net_quiet_run(p, lane, t0, min(t0 + G * tpw, tiles), acc);
      if (wave0 == 0u && lane == 0u) atomicAdd(p.nq_rounds, 1u);
      nq_taken = true;
      nq_tag = false;
    }
  }
  if constexpr (MODE == kModeWarmPipe) {
    // software-pipelined: tile t + nwaves's loads (state, peer draw, gathers)
    // are in flight while tile t is computed
    TileIn<K, false, true> cur, nxt;
    uint32_t tile = wave0;
    if (tile < tiles) load_tile<K, false, true, POL, false, true>(p, tile, lane, cur);
    for (; tile < tiles; tile += nwaves) {
      const uint32_t next = tile + nwaves;
      if (next < tiles) load_tile<K, false, true, POL, false, true>(p, next, lane, nxt);
      process_tile<K, false, true, POL, true>(p, tile, lane, cur, 0u, acc);
      cur = nxt;
    }
  } else if (!nq_taken) {
    uint32_t tile = wave0, tile_end = tiles, stride = nwaves;
    WaveDraw wd;
    wd.ok = false;
    wd.pair = false;
    wd.nlA = 0u;
    wd.nn = 0u;
    wd.flagok = 0ull;
    wd.t0 = 0u;
    wd.meta = 0u;
    wd.badc = wd.badp = 0ull;
    wd.sdc = wd.sdp = nullptr;
    wd.fofs = 0u;
    uint32_t uni_done = 0u;  // uniform rows: run tiles settled with no draw (settled_run_uni)
    bool uni_ran = false;
    __shared__ __attribute__((aligned(16))) uint32_t s_draw[4][512];
    uint32_t* const sd = s_draw[threadIdx.x >> 6];
    if constexpr (MODE == kModeWarm && K == 8) {
      if (p.tpw) {
        // a run of p.tpw consecutive tiles per wave; one Philox pass draws the
        // peers of all its nodes (round - 1's too if a tile is kVStale)
        tile = wave0 * p.tpw;
        tile_end = min(tile + p.tpw, tiles);
        stride = 1u;
        if (p.uni_merge > 1u && p.lean && p.settled_fast && p.klazy && p.vv && p.tpw * p.uni_merge <= kUniRun &&
            uniform) {
          // uniform input: most tiles settle with no draw, and what is left per wave is its set-up,
          // so every uni_merge-th wave takes its neighbours' runs too and the others end here
          if (wave0 % p.uni_merge) tile = tile_end = tiles;
          else tile_end = min(tile + p.tpw * p.uni_merge, tiles);
        }
        nq_tag = tile < tiles;
        if (tile < tiles) {
          const uint32_t nlA = uni(div_bl(p, tile * 64u));
          const uint32_t nlB = uni(div_bl(p, min(tile_end * 64u, p.L) - 1u));
          const uint32_t nn = nlB - nlA + 1u;
          // uniform rows: settled_run_uni's loads (UniPre)
          UniPre upre;
          const bool uni_ok = p.uni_in && p.lean && p.settled_fast && p.klazy && p.vv && nn <= 256u &&
                              tile_end - tile <= kUniRun;
          // the run's per-tile words, one lane per tile (tpw <= 16)
          const uint32_t ti = tile + lane;
          const uint32_t st = p.vv && ti < tile_end ? p.vstale[ti] : 0u;
          const uint32_t kw = (p.klazy || p.kconsume) && ti < tile_end ? p.kpend[ti] : 0u;
          if constexpr (!CC) {  // (the counting build requests them where it always did, below)
            if (uni_ok) uni_early(p, lane, nlA, upre);
          }
          wd.meta = (st << 8) | (kw & (kPendAllLive | kHiVirt | 0xFFu));
          wd.t0 = tile;
          wd.nlA = nlA;
          wd.nn = nn;
          // uniform rows: the run's settled candidates first, with no draw; the draw only if a tile is left
          const uint32_t all_tiles = run_mask(tile_end - tile);
          if (uni_ok && uniform) {
            // the run's quiescent tiles (sweep_settled.h "Quiescent tiles"): settled candidates with two deferred rounds behind them,
            // both input snapshots uniform (a Byzantine node in the run: settled_run_uni drops them)
            const bool qt = !CC && prev_uni && p.quiet_tiles;
            if constexpr (CC) uni_early(p, lane, nlA, upre);
            const uint32_t quiet = uni_prefetch<POL>(p, lane, tile, tile_end, nn, wd.meta, qt, upre);
            uni_done = settled_run_uni<POL, CC>(p, lane, tile, tile_end, wd.meta, nlA, nn, upre, quiet, acc);
            uni_ran = true;
            // (a run holding a Byzantine node comes back with no tile done)
            if (quiet == all_tiles && uni_done == all_tiles) nq_tag = false;
          }
          // (the tiles the uniform walk settled, calm ones among them, need no regather; a run holds
          // at most 16 tiles, lane i its tile i: st is 0 past them, uni_done a 32-bit mask)
          const bool any_stale = __ballot((st & kVMask) == kVStale && lane < 32u && !((uni_done >> lane) & 1u)) != 0ull;
          if (uni_done != all_tiles) {
            wd.pair = any_stale;
            wd.flagok = 0ull;
            if (any_stale && nn * 2u > 32u) {
              // both rounds' draws for up to 32 nodes: two passes over all 64 lanes, parked side by side
              const PairDraw dp = single_draw(p, p.round - 1u, nlA, nn, lane);
              const PairDraw dc = single_draw(p, p.round, nlA, nn, lane);
              wd.ok = !dp.fallback && !dc.fallback;
              if (wd.ok) {
                park_draw(dp, sd, lane, p.PS * 4u);
                park_draw(dc, sd + 256, lane, p.PS * 4u);
              }
              wd.sdp = sd;
              wd.sdc = sd + 256;
              wd.badp = dp.bad;
              wd.badc = dc.bad;
            } else {
              // one pass: lanes 0-31 round - 1 and 32-63 this round (pair), or all 64 this round
              const PairDraw d = any_stale ? pair_draw(p, p.round, nlA, nn, lane) : single_draw(p, p.round, nlA, nn, lane);
              wd.ok = !d.fallback;
              if (wd.ok) park_draw(d, sd, lane, p.PS * 4u);
              wd.sdp = sd;
              wd.sdc = any_stale ? sd + 128 : sd;
              wd.badp = d.bad & 0xFFFFFFFFull;
              wd.badc = any_stale ? d.bad >> 32 : d.bad;
              wd.fofs = any_stale ? 32u : 0u;
              if constexpr (REF) {
                if (wd.ok && p.rflag_in && p.klazy) {  // the run's peer flags in 4 loads (settled_run)
                  const uint8_t tag = ref_tag(p.round);
                  uint32_t ok = 1u;
#pragma unroll
                  for (int i = 0; i < 4; ++i) ok &= p.rflag_in[d.prod[i]] == tag ? 1u : 0u;
                  wd.flagok = __ballot(ok != 0u);
                }
              }
            }
          }
        }
      }
    }
    uint32_t lean_done = uni_done;  // run tiles the lean settled loop completed (bit i: tile wd.t0 + i)
    bool lean_ran = uni_ran;        // the run's settled candidates were all tested by it
    if constexpr (MODE == kModeWarm && K == 8) {
      if (!uni_ran && wd.ok && wd.badc == 0ull && p.lean && p.settled_fast && p.klazy && p.vv && tile < tile_end) {
        lean_done = settled_run<POL, REF, CC>(p, lane, tile_end, wd, acc);
        lean_ran = true;
      }
    }
    const uint32_t qfirst = tile, qstep = stride;  // deferred pushes: slot s = tile qfirst + s * qstep
    uint32_t qn = 0;
    if constexpr (MODE == kModeWarm && K == 8) {
      // every tile of the run settled in the lean loops (the settled rounds): no tile loop at all, whose
      // per-tile skip test cost a settled wave ~8 scalar instructions per tile (the settled rounds are
      // bound by the CU's scalar issue); the queued pushes of those tiles are still flushed below
      if (lean_ran && stride == 1u && tile < tile_end &&
          lean_done == run_mask(tile_end - tile)) {
        qn = tile_end - tile;
        tile = tile_end;
      }
    }
    // tile draws (p.tile_draw): a run whose nodes overflow the run's draw (narrow rows: at BL <= 16 a
    // 16-tile run holds 64-256 nodes) still shares one Philox pass per tile, 2 producer lanes per
    // node (a tile's 64 / BL nodes fit: BL >= 2, or >= 4 with a stale tile's paired draw), instead of
    // every lane drawing its node's 8 peers alone (4-16 lanes per node repeating the same draw)
    const bool tdraw = MODE == kModeWarm && K == 8 && p.tile_draw && p.tpw && !wd.ok && tile < tile_end;
    for (; tile < tile_end; tile += stride) {
      constexpr bool AB = MODE == kModeAblate;
      if constexpr (CC) acc.qslot = qn++;
      if constexpr (MODE == kModeWarm) {
        if constexpr (K == 8) {
          if (lean_done && ((lean_done >> (tile - wd.t0)) & 1u)) continue;
          if (tdraw) {
            const uint32_t tnlA = uni(div_bl(p, tile * 64u));
            const uint32_t tnn = uni(div_bl(p, min(tile * 64u + 64u, p.L) - 1u)) - tnlA + 1u;
            const bool tst = ((meta_of(wd, tile) >> 8) & kVMask) == kVStale;  // wave-uniform
            const PairDraw d = tst ? pair_draw(p, p.round, tnlA, tnn, lane) : single_draw(p, p.round, tnlA, tnn, lane);
            wd.ok = !d.fallback;
            if (wd.ok) {
              park_draw(d, sd, lane, p.PS * 4u);
              wd.nlA = tnlA;
              wd.nn = tnn;
              wd.pair = tst;
              wd.sdp = sd;
              wd.sdc = tst ? sd + 128 : sd;
              wd.badp = d.bad & 0xFFFFFFFFull;
              wd.badc = tst ? d.bad >> 32 : d.bad;
              wd.fofs = tst ? 32u : 0u;
              wd.flagok = 0ull;
            }
          }
          if (wd.ok && p.settled_fast && p.klazy && p.vv && !lean_ran) {
            const uint32_t m = meta_of(wd, tile);
            // (calm tiles only in a run with no Byzantine node, as in settled_run)
            const bool cok = p.calm && ((m >> 8) & kVCalm) &&
                             __ballot(lane < wd.nn && is_byz(p.byz, p.n0 + wd.nlA + lane)) == 0ull;
            if (settled_cand(m, cok ? 1u : 0u) &&
                settled_tile<POL, REF, CC>(p, tile, lane, m & (kPendAllLive | kHiVirt | 0xFFu), wd, acc, m >> 8))
              continue;
          }
        }
        TileIn<K, false, true> in;
        load_tile<K, false, true, POL, false, true, false, CC>(p, tile, lane, in, &wd, uflags);
        process_tile<K, false, true, POL, true, REF, CC, true>(p, tile, lane, in, 0u, acc, uflags);
      } else if constexpr (MODE == kModeFresh) {
        TileIn<K, false, false> in;
        load_tile<K, false, false, POL, false, true, true>(p, tile, lane, in);
        process_tile<K, false, false, POL, true>(p, tile, lane, in, 0u, acc);
      } else if constexpr (MODE == kModeReplay) {
        TileIn<K, true, false> in;
        load_tile<K, true, false, POL, false>(p, tile, lane, in);
        process_tile<K, true, false, POL>(p, tile, lane, in, 0u, acc);
      } else {
        bool warm = false;
        if (p.warm_skip) {
          // all-ones oldest consider plane <=> all consider planes all-ones (monotone sim votes)
          const uint32_t g = tile * 64u + lane;
          const uint32_t c7 = g < p.L ? p.planes[(size_t)tile * (kPlanes * 64u) + 1024u + 7u * 64u + lane] : ~0u;
          warm = __all(c7 == ~0u);
        }
        if (warm) {
          TileIn<K, false, true> in;
          load_tile<K, false, true, POL, AB>(p, tile, lane, in);
          process_tile<K, false, true, POL>(p, tile, lane, in, 4u, acc);
        } else {
          TileIn<K, false, false> in;
          load_tile<K, false, false, POL, AB>(p, tile, lane, in);
          process_tile<K, false, false, POL>(p, tile, lane, in, 0u, acc);
        }
      }
    }
    if constexpr (CC) {
      if (p.push_q && qn) acc.pushed += (uint32_t)wave_sum(flush_pushes(p, lane, qfirst, qstep, qn, acc.qpub, acc.qpm));
    }
  }
  // one flush per wave (shard = wave index); 32-bit sums: a wave's lanes
  // accumulate < 2^32 over the tiles a grid gives it (the engine's grids
  // walk <= 16 tiles per wave by default, 2^32 / (64 * 32 * 8) = 262k at most)
  const unsigned long long s = wave_sum(acc.applied);
  const unsigned long long f = __ballot(acc.died != 0u) ? wave_sum(acc.died) : 0ull;
  const unsigned long long by = (unsigned long long)wave_sum(acc.lane_bytes) + acc.emitted_bytes;
  const unsigned long long rr = wave_sum(acc.reread);
  if (lane == 0) {
    const uint32_t shard = acc.shard;
    if (s) atomicAdd(&p.applied[shard], s);
    if (f) atomicAdd(&p.finalized[shard], f);
    if (by) atomicAdd(&p.bytes[shard], by);
    if (rr) atomicAdd(&p.bytes[kLogShards + shard], rr);
    if (acc.updates) atomicAdd(&p.upd_count[shard], acc.updates);
  }
  if (p.count_changed && lane == 0 && acc.changed) {
    atomicAdd(&p.changed[acc.shard], (unsigned long long)acc.changed);
    atomicAdd(&p.changed[kLogShards + acc.shard], (unsigned long long)acc.changed_segs);
  }
  if (p.count_changed && lane == 0 && acc.pushed) atomicAdd(&p.changed[2 * kLogShards + acc.shard], (unsigned long long)acc.pushed);
  if (p.nq_out && nq_tag && lane == 0) *p.nq_out = p.round + 1u;  // not a quiescent wave (kernels.h nq_out)
  if (p.uni_out && __ballot(acc.umis != 0u) != 0ull && lane == 0) {
    // some word this wave published differs from the reference row: tag the output snapshot's slot
    // of this rank in every replica (read by the next round, after the barrier in a peer exchange)
    // (p.uni_post: the engine copies the slot to the peers once after the round, in the barrier
    // kernel: every wave of a storm round tags, and 7 system-scope stores per wave into the same 7
    // words serialised the whole round, 0.13 -> 0.6 ms per rank at 8 ranks)
    const uint32_t tag = p.round + 1u;
    p.uni_out[p.uni_rank] = tag;
    if (!p.uni_post)
      for (uint32_t r = 0; r < p.push_n; ++r)
        __hip_atomic_store(peer_ptr(p.push_dst, r) + p.uni_off + p.uni_rank, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// dynamic LDS of a sweep launch: the deferred-push queue of its 4 waves (p.push_q)
constexpr uint32_t kPushQBytes = 4u * kPushQ * 64u * 5u;

template <int K, int MODE, bool CC>
hipError_t launch_mode_cc(const RoundParams& p, uint32_t grid, hipStream_t s) {
  const uint32_t shm = CC && p.push_q ? kPushQBytes : 0u;
  // write-through store policies are built for k = 8 only (the measured workloads)
  const uint32_t pol = (K == 8 && p.store_policy >= 2) ? p.store_policy : (p.plane_nt ? 1u : 0u);
  if constexpr (K == 8 && MODE == kModeWarm) {
    // reference rows (kernels.h): the walking warm mode writes the flags and settled tiles read them
    if (p.rflag_out) {
      if (pol == 1)
        hipLaunchKernelGGL((k_round_sweep<K, MODE, 1, true, CC>), dim3(grid), dim3(256), shm, s, p);
      else
        hipLaunchKernelGGL((k_round_sweep<K, MODE, 0, true, CC>), dim3(grid), dim3(256), shm, s, p);
      return hipGetLastError();
    }
  }
  switch (pol) {
    case 0: hipLaunchKernelGGL((k_round_sweep<K, MODE, 0, false, CC>), dim3(grid), dim3(256), shm, s, p); break;
    case 1: hipLaunchKernelGGL((k_round_sweep<K, MODE, 1, false, CC>), dim3(grid), dim3(256), shm, s, p); break;
    default:
      if constexpr (K == 8) {
        if (pol == 2)
          hipLaunchKernelGGL((k_round_sweep<K, MODE, 2, false, CC>), dim3(grid), dim3(256), shm, s, p);
        else
          hipLaunchKernelGGL((k_round_sweep<K, MODE, 3, false, CC>), dim3(grid), dim3(256), shm, s, p);
      }
  }
  return hipGetLastError();
}

// CC (changed-word counting and peer pushes, p.count_changed): the walking warm mode at k = 8 (the
// hot path) has a separate build without it, so that its single-GPU rounds carry none of the
// prefetched overwritten words' registers; every other mode keeps the runtime switch
template <int K, int MODE>
hipError_t launch_mode(const RoundParams& p, uint32_t grid, hipStream_t s) {
  if constexpr (K == 8 && MODE == kModeWarm) {
    if (!p.count_changed) return launch_mode_cc<K, MODE, false>(p, grid, s);
  }
  return launch_mode_cc<K, MODE, true>(p, grid, s);
}

// mode: the round plan's (round_plan.h); what depends on the grid alone is decided here.
template <int K>
hipError_t launch_sweep_k(const RoundParams& p_in, SweepMode mode, uint32_t blocks, hipStream_t s, bool* ref_written) {
  if (ref_written) *ref_written = false;
  const uint32_t tiles = p_in.Lpad / 64u;
  const SweepGrid g = sweep_grid(tiles, blocks);
  RoundParams p = p_in;
  p.tpw = 0u;
  // deferred pushes: every wave of the grid takes at most kPushQ tiles (a run, or a grid stride over
  // <= kPushQ tiles) and at most 8 peers (the queue's byte per lane); the resident pipelined grid and
  // larger worlds push from the tile loop
  p.push_q = p.push_defer && p.push_n && p.push_n <= 8u && g.run <= kPushQ ? 1u : 0u;
  // p_in.tpw = enabled: each wave takes a run of consecutive tiles
  // (long runs: grid stride; their nodes overflow the shared draw anyway)
  if (mode == SweepMode::Warm && p_in.tpw && K == 8 && g.run && g.run <= 16u) {
    p.tpw = g.run;
    if (ref_written) *ref_written = p.rflag_out != nullptr;
    return launch_mode<K, kModeWarm>(p, g.grid, s);
  }
  p.rflag_out = nullptr;  // only the walking warm mode writes reference-row flags
  p.rflag_in = nullptr;
  switch (mode) {
    case SweepMode::Replay: return launch_mode<K, kModeReplay>(p, g.grid, s);
    case SweepMode::Ablate: return launch_mode<K, kModeAblate>(p, g.grid, s);
    case SweepMode::Fresh: return launch_mode<K, kModeFresh>(p, g.grid, s);
    case SweepMode::Warm:  // a resident grid walks several tiles per wave: pipeline them
      if (blocks && g.grid < (tiles + 3u) / 4u && !p.nopipe) {
        p.push_q = 0u;
        return launch_mode<K, kModeWarmPipe>(p, g.grid, s);
      }
      return launch_mode<K, kModeWarm>(p, g.grid, s);
    case SweepMode::Check: break;
  }
  return launch_mode<K, kModeCheck>(p, g.grid, s);
}

template <int K>
hipError_t occupancy_k(bool replay, int* bpc) {
  return replay ? hipOccupancyMaxActiveBlocksPerMultiprocessor(bpc, k_round_sweep<K, kModeReplay, 1>, 256, 0)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(bpc, k_round_sweep<K, kModeWarmPipe, 1>, 256, 0);
}

}  // namespace
}  // namespace avk
