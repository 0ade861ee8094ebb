// Persistent streaming round kernel (uncapped path, k <= 8): the hot path of
// the engine. One round of go-avalanche's poll loop for every simulated node
// (processor.go:92-117 driven by main.go:110-136, rules R1-R4 of SURVEY.md
// §8): peer draw (processor.go:173-182 replaced by a Philox k-peer draw),
// gather of each peer's published IsAccepted word (main.go:168-192 responder),
// k regsiterVote steps (vote.go:54-75) on 32 bit-sliced VoteRecords per lane,
// StatusUpdate emission (processor.go:111) and deletion on finalization
// (:114-116).
//
// Same HBM layout, outputs and counters as k_round_fast (round_firstgen.hip); what
// differs is how the work maps onto CDNA4:
//  * the Philox peer draw runs once per (node, Philox block) across the
//    wave's lanes and is handed to the node's lanes with ds_bpermute, instead
//    of every lane of a node redrawing the same peers (round_slots.h);
//  * per slot, the ">6 of 8" thresholds of vote.go:58,61 are "at most one
//    zero" over the 8-vote window of [old planes | new votes]: a prefix of the
//    new votes carried from slot to slot plus the shrinking old part,
//    combined in 2 ops (round_slots.h); on warm planes with sim votes the no
//    side runs on the complement of the same registers;
//  * the confidence update is deferred: a 4-plane counter of agreements since
//    the last flip, added once at the end (count = flipped ? c : count + c);
//    a wave holding a record with count >= 120 also detects, per slot, the
//    vote that takes a record from 127 to 128 (finalization and deletion);
//  * once every consider plane is known to be all-ones (sim votes only, the
//    engine tracks it), the consider planes are neither read nor written and
//    the per-tile warmth probe disappears;
//  * 72 VGPRs at k = 8 (7 waves per SIMD); one wave per tile, or a resident
//    grid walking the tiles when tiles are few (the per-wave counters are
//    then flushed once per wave, and each wave issues its next tile's loads
//    before computing the current one).
// The kernel and its launchers are templates on k in sweep_kernel.h; this unit compiles k = 8 (32 kernels),
// round_sweep_lowk.hip k = 1..7 (84). The tile, settled and publish paths are in sweep_tile.h,
// sweep_settled.h and sweep_publish.h. The write-back kernel k_materialize stays in this unit, in the code
// object of the k = 8 kernels whose deferred forms it writes back: in an object of its own, with the same
// device code, bench.py measured 2-3 % slower (supposed: the extra code object is first loaded
// by the first write-back, inside the timed window).

// Build knob: compile the per-phase ablation diagnostics (option "ablate_phase") into the warm
// path (1: the Makefile's "ablate" variant library only; the product kernel is built without them)
#ifndef AVK_ABLATE_PHASE
#define AVK_ABLATE_PHASE 0
#endif
// A/B build knob: the storm path's publish loads (overwritten word, stale and need bytes) issued
// before the tile's plane stores (1) or by publish itself, after them (0, default: measured 3 % faster
// on masked C4p node shards at 8 ranks, profiles/r06/ab_pub_preload.log)
// (decided, but kept: taking its losing side out changes the counting k = 8 kernels' register
// allocation, so it goes with the next change to publish)
// (as sensitive: k_round_sweep's run prologue out of line, a __forceinline__ function taking references, was
// tried, changed the twelve warm k = 8 kernels, and was left out)
#ifndef AVK_PUB_PRELOAD
#define AVK_PUB_PRELOAD 0
#endif

#include "sweep_kernel.h"

namespace avk {
namespace {

// The write-back's stores non-temporal (a write-only stream; the next round streams the planes back
// with non-temporal loads of its own), which also leaves L2 / MALL to the stale tiles' regathered
// rows. A/B (tools/wb_probe.py, three alternations on one box, profiles/r05/s18/ab_matnt.log):
// C4 0.80 -> 0.74 ms, C4p 0.65 -> 0.455, C5 1.56 -> 1.42 per segment end.
// k_materialize writes back both deferred forms in one pass, before anything other than a warm k = 8
// sim round reads or writes the records (do_v: stale vote planes, whose vote register is the last
// round's 8 gathered votes, V_i = slot 7 - i, and unstored consider planes; do_k: pending count steps
// (kernels.h klazy: + 8 * pending on the polled records) and virtual K4..K7 groups).
// Per tile every load (A for a uniform vote register, the K groups, a stale tile's peer rows) is issued
// before any store: vmcnt counts loads and stores in issue order, so a load issued after the tile's
// consider-plane stores waited for their write acknowledgements too (round 5's walking version paid
// that per tile, 16 tiles in a row per wave: ~5 TB/s at C4's segment end). A wave takes `run`
// consecutive tiles (default 1: the memory system hides each tile's round trip behind other waves').
__device__ __forceinline__ void materialize_tile(const RoundParams& p, uint32_t tile, uint32_t lane, uint32_t raw,
                                                 uint32_t kw) {
  const LaneIdx x = lane_idx(p, tile, lane);
  uint32_t* const tp = p.planes + (size_t)tile * (kPlanes * 64u);
  u32x4* const grp = reinterpret_cast<u32x4*>(tp) + lane;
  const uint32_t st = raw & kVMask;
  const uint32_t pend = kw & 0xFFu;
  const bool dok = (pend || (kw & kHiVirt)) && x.active;
  // + 8 * pend reaches the K0..K3 group only through K3, by pend's bit 0, and the carry into K4 then
  // starts from zero: for an even pend the group is neither loaded nor stored
  const bool klo = dok && (pend & 1u);
  // ---- loads
  u32x4 o0, o1, k0 = u32x4{0u, 0u, 0u, 0u}, k1;
  if (st == kVUniform) {  // V_i = A on every polled record
    const uint32_t A = tp[1536u + lane];
    o0 = o1 = u32x4{A, A, A, A};
  } else if (st) {  // the last round's 8 gathered votes, V_i = slot 7 - i
    const uint32_t nlA = uni(x.nl), nn = (uint32_t)__builtin_amdgcn_readlane((int)x.nl, 63) - nlA + 1u;
    uint32_t pp[8];
    draw_peers<8>(p, p.round - 1u, x.node, x.nl, nlA, nn, lane, pp);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      o0[c] = p.pref_prev[pp[7 - c] * p.PS + x.b];
      o1[c] = p.pref_prev[pp[3 - c] * p.PS + x.b];
    }
  }
  uint32_t vb = 0u;
  if (dok) {
    if (klo) k0 = grp[128];
    k1 = kw & kHiVirt ? u32x4{0u, 0u, 0u, ~real_mask(p.tn, x.b)} : grp[192];  // kernels.h kHiVirt
    vb = p.valid[x.b];
  }
  // ---- stores
  if ((raw & kCAll) && x.active) {  // consider planes: all-ones
#pragma unroll
    for (int c = 0; c < 8; ++c) pst<true>(tp + 1024u + (uint32_t)c * 64u + lane, ~0u);
  }
  if (st && x.active) {
    pst4<true>(grp, o0);
    pst4<true>(grp + 64, o1);
  }
  if (dok) {  // + 8 * pend on the polled records' counts
    uint32_t Kp[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      Kp[c] = k0[c];
      Kp[4 + c] = k1[c];
    }
    const uint32_t P0 = ~Kp[7] & vb;
    uint32_t cy = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // + pend on count bits 3..6
      const uint32_t bi = ((pend >> c) & 1u) ? P0 : 0u;
      const uint32_t t = Kp[3 + c] ^ bi;
      const uint32_t si = t ^ cy;
      cy = (t & cy) | (Kp[3 + c] & bi);
      Kp[3 + c] = si;
    }
    u32x4 o2, o3;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      o2[c] = Kp[c];
      o3[c] = Kp[4 + c];
    }
    if (klo) pst4<true>(grp + 128, o2);
    pst4<true>(grp + 192, o3);
  }
}

__global__ __launch_bounds__(256) void k_materialize(const RoundParams p, uint32_t run, uint32_t do_v, uint32_t do_k) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uni(blockIdx.x * 4u + (threadIdx.x >> 6));
  const uint32_t tiles = p.Lpad >> 6;
  if (run == 1u) {  // the tile words as scalar loads (the tile index is wave-uniform)
    if (wave >= tiles) return;
    const uint32_t raw = do_v ? uni(p.vstale[wave]) : 0u;
    const uint32_t kw = do_k ? uni(p.kpend[wave]) : 0u;
    if (raw == 0u && kw == 0u) return;
    materialize_tile(p, wave, lane, raw, kw);
    if (lane == 0) {
      if (raw) p.vstale[wave] = 0u;
      if (kw) p.kpend[wave] = 0u;
    }
    return;
  }
  const uint32_t t0 = wave * run;
  if (t0 >= tiles) return;
  const uint32_t n = min(run, tiles - t0);
  const uint32_t ti = t0 + lane;
  const uint32_t stw = do_v && lane < n ? p.vstale[ti] : 0u;
  const uint32_t kww = do_k && lane < n ? p.kpend[ti] : 0u;
  if (__ballot(stw != 0u || kww != 0u) == 0ull) return;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t raw = (uint32_t)__builtin_amdgcn_readlane((int)stw, (int)i);
    const uint32_t kw = (uint32_t)__builtin_amdgcn_readlane((int)kww, (int)i);
    if (raw == 0u && kw == 0u) continue;
    materialize_tile(p, t0 + i, lane, raw, kw);
  }
  if (lane < n) {
    if (stw) p.vstale[ti] = 0u;
    if (kww) p.kpend[ti] = 0u;
  }
}

}  // namespace

hipError_t launch_round_sweep(const RoundParams& p, int k, SweepMode mode, uint32_t blocks, hipStream_t s,
                              bool* ref_written) {
  if (k != 8) return launch_round_sweep_lowk(p, k, mode, blocks, s, ref_written);
  return launch_sweep_k<8>(p, mode, blocks, s, ref_written);
}

hipError_t launch_materialize(const RoundParams& p, bool do_v, bool do_k, hipStream_t s) {
  if ((do_v && (!p.vstale || !p.pref_prev)) || (do_k && !p.kpend)) return hipErrorInvalidValue;
  if (!do_v && !do_k) return hipSuccess;
  const uint32_t run = p.mat_run ? p.mat_run : 1u;
  const uint32_t tiles = p.Lpad / 64u;
  const uint32_t waves = (tiles + run - 1u) / run;
  hipLaunchKernelGGL(k_materialize, dim3((waves + 3u) / 4u), dim3(256), 0, s, p, run, do_v ? 1u : 0u, do_k ? 1u : 0u);
  return hipGetLastError();
}

hipError_t round_sweep_occupancy(int k, bool replay, int* blocks_per_cu, int* cus) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  if (k != 8) return round_sweep_occupancy_lowk(k, replay, blocks_per_cu);
  return occupancy_k<8>(replay, blocks_per_cu);
}

}  // namespace avk
