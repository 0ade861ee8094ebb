// The sweep kernel's settled paths (k_round_sweep, sweep_kernel.h; kModeWarm, k = 8, klazy rounds), each
// with less work per tile than the one before: settled_tile, settled_run, settled_run_uni and its
// quiescent tiles, net_quiet_run; and the written invariants the last two rest on ("Quiescent tiles",
// "Network-quiet rounds"). Included by the sweep translation units only; reads no build knob.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "round_common.h"
#include "round_slots.h"
#include "sweep_publish.h"
#include "sweep_tile.h"

namespace avk {
namespace {

// A settled candidate by its meta word (WaveDraw::meta): every live record of the tile is valid
// (kPendAllLive), and its vote register is uniform (kVUniform), or stale with at most one stray
// vote per polled record (kVStale | kVCalm, kernels.h calm; `calm` = p.calm).
__device__ __forceinline__ bool settled_cand(uint32_t m, uint32_t calm) {
  const uint32_t v = (m >> 8) & (kVMask | kVCalm);
  return (m & kPendAllLive) && (v == kVUniform || (calm && v == (kVStale | kVCalm)));
}
// A calm tile that settled (m: its meta word): its 8 new votes all equal A, so its vote register is
// uniform from here on. Called by the one lane that owns the tile's words; returns the bytes written.
__device__ __forceinline__ uint32_t calm_settle(const RoundParams& p, uint32_t tile, uint32_t m) {
  if (!((m >> 8) & kVCalm)) return 0u;
  p.vstale[tile] = kVUniform | ((m >> 8) & kCAll);
  return 4u;
}
// A settled tile's kpend word (m: the word it had, or its meta word): one more deferred +8 step, every
// live record still valid, the virtual K4..K7 group kept.
__device__ __forceinline__ uint32_t pend_next(uint32_t m) { return ((m & 0xFFu) + 1u) | kPendAllLive | (m & kHiVirt); }
// Bit i for each of a run's n <= 32 tiles (tile t0 + i).
__device__ __forceinline__ uint32_t run_mask(uint32_t n) { return (uint32_t)((1ull << n) - 1ull); }

// Settled-tile fast path (kModeWarm, k = 8, klazy round, the wave's parked
// draw): a tile whose vote register is uniform (kVUniform: V = A on every
// polled record) and whose count planes are deferred with every live record
// valid (kPendAllLive) is settled this round iff every polled record's 8
// gathered votes equal its accepted bit. process_tile would then store only
// the published words and the tile's pending count (+8 steps deferred once
// more): no flip, no StatusUpdate, no deletion, V stays uniform, A and K
// unchanged. This reads A, the validity word and the 8 votes and does exactly
// that; any other tile returns false and takes the general load + step.
// A stale tile flagged kVCalm (kernels.h calm) is a candidate too, here and in settled_run /
// settled_run_uni: at most one of its old votes differs from A on any polled record, so with 8 new
// votes equal to A every window of the round is still a conclusive agreement. It is tested with no
// regather; when it settles its tile word becomes kVUniform (vst: the word as stored, 4 B written),
// when it does not it takes the general path as the stale tile it is.
template <int POL, bool REF, bool CC>
__device__ __forceinline__ bool settled_tile(const RoundParams& p, uint32_t tile, uint32_t lane, uint32_t kw,
                                             const WaveDraw& wd, SweepAcc& acc, uint32_t vst) {
  const uint32_t g = tile * 64u + lane;
  const bool active = g < p.L;
  const uint32_t gc = active ? g : p.L - 1u;
  const uint32_t nl = div_bl(p, gc);
  const uint32_t b = gc - nl * p.BL;
  // A plane: a buffer resource on the tile (SGPRs) + the lane's constant byte
  // offset, so no 64-bit per-lane address is kept live across the tile loop
  // (the flat form was hoisted into a VGPR pair that spilled and was reloaded
  // from scratch, with a full vmcnt wait, at every settled tile)
  const __amdgpu_buffer_rsrc_t ta =
      __builtin_amdgcn_make_buffer_rsrc(p.planes + (size_t)tile * (kPlanes * 64u), 0, kPlanes * 64 * 4, kRsrcWord3);
  const uint32_t A = __builtin_amdgcn_raw_buffer_load_b32(ta, (1536u + lane) * 4u, 0, POL > 0 ? 2 : 0);
  const uint32_t P0 = active ? at_byte(p.valid, b * 4u) : 0u;  // polled = live (kPendAllLive) and valid
  const uint32_t uref = p.uni_out ? p.pref_in[p.ref_node * p.PS + b] : 0u;  // uniform rows (kernels.h)
  uint32_t rows[8];
  pick_parked(p, wd.sdc, wd.badc, (nl - wd.nlA) * 2u, p.n0 + nl, p.round, p.PS * 4u, rows);
  const uint32_t bo = b * 4u;
  uint32_t dis = 0u, all = ~0u;
  bool gather = true;
  uint32_t rbytes = 0u;  // reference-row reads
  if (REF && p.rflag_in) {
    // peers whose published row is the reference row (kernels.h rflag_in):
    // when all 8 are, each of the 8 votes is that row's word (the reference
    // word is loaded beside the flags, not after them)
    const uint32_t rw = p.pref_prev[p.ref_node * p.PS + b];
    uint32_t fl = 1u;
#pragma unroll
    for (int j = 0; j < 8; ++j) fl &= p.rflag_in[rows[j] >> p.ps_shift] == ref_tag(p.round) ? 1u : 0u;
    rbytes = 4u + (b == 0u ? 8u : 0u);
    if (fl) {
      dis = all = rw;
      gather = false;
    }
  }
  if (gather) {
#pragma unroll
    for (int j = 0; j < 8; ++j) dis |= at_byte(p.pref_in, rows[j] + bo);
#pragma unroll
    for (int j = 0; j < 8; ++j) all &= at_byte(p.pref_in, rows[j] + bo);
  }
  // every vote equals A  <=>  (OR of votes) == A == (AND of votes) on P0
  if (__ballot(((dis ^ A) | (all ^ A)) & P0) != 0ull) return false;
  const uint32_t node = p.n0 + nl;
  const uint32_t pub = is_byz(p.byz, node) ? byz_pattern(p.round + 1u) : A;
  if (active) {
    if (p.uni_out) acc.umis |= pub != uref ? 1u : 0u;
    const uint32_t prow = node * p.PS + b;  // < N * PS < 2^30 (sweep gate)
    const bool known = (kw & 0xFFu) >= 2u;  // (publish)
    publish<POL, CC>(p, prow, pub, is_byz(p.byz, node) ? byz_pattern(p.round - 2u) : pub, acc, known, nl, acc.qslot);
  }
  if (REF && p.rflag_out) ref_flag_store(p, lane, active, b, node, pub, p.pref_in[p.ref_node * p.PS + (active ? b : 0u)]);
  if (lane == 0) p.kpend[tile] = pend_next(kw);
  const uint32_t cbytes = lane == 0 ? calm_settle(p, tile, vst << 8) : 0u;
  acc.applied += 8u * (uint32_t)__popc(P0);
  // process_tile's accounting for this case: 17 plane words + 8 vote words +
  // valid read, minus V (uniform), V store (virtual), K read + store (deferred),
  // A store (unchanged) = 40 B per lane (+ 4 B push read); kpend read + write
  // reference rows: 8 flag bytes per node read, the reference word instead of
  // the 32 B of gathered votes, the next reference word + the flag written
  acc.reread += active && gather ? 28u : 0u;
  acc.lane_bytes += (active ? 40u + (p.count_changed ? 4u : 0u) + rbytes - (gather ? 0u : 32u) +
                                  (REF && p.rflag_out ? 4u + (b == 0u ? 1u : 0u) : 0u)
                            : 0u) +
                    (lane == 0 ? 8u : 0u) + cbytes;
  return true;
}

// The settled candidates of a wave's run in one lean loop (p.lean: kModeWarm,
// k = 8, klazy round, BL dividing 64, the run's draw parked with no repeated
// candidate). Same test and outputs as settled_tile, with everything that does
// not depend on the tile hoisted out of the loop: a lane's block b = lane % BL
// and its validity word, the run's Byzantine bits (one ballot), the A-plane
// buffer resource (the tile moves the scalar offset only), the node index
// (shift, no division); the kpend words of the settled tiles are written by one
// store per run (lane i: tile t0 + i) and the counters accumulated per tile
// without a branch. Per settled tile: the A load, 8 gathers, 2 LDS reads, one
// ballot, the published-word store. Returns the run's settled tiles (bit i =
// tile t0 + i); the others take the general load + step afterwards.
//
// REF (reference rows, kernels.h rflag_*): a tile whose 8 peers' rows are all
// flagged equal to the reference row takes the reference word (one hoisted
// load per run) for all 8 votes instead of gathering them. The run's flags are
// read in the prologue next to the draw (4 byte loads per producer lane, from
// 1 MB at C4: L2-resident where the 128 MB of rows are not) and kept as one
// ballot. Every settled tile writes its nodes' flags for the row it published.
template <int POL, bool REF, bool CC>
__device__ __forceinline__ uint32_t settled_run(const RoundParams& p, uint32_t lane, uint32_t tile_end,
                                                const WaveDraw& wd, SweepAcc& acc) {
  const uint32_t t0 = wd.t0, ntiles = tile_end - t0;
  const uint32_t b = lane & (p.BL - 1u), bo = b * 4u;
  const uint32_t vw = at_byte(p.valid, bo);
  // Byzantine bits of the run's nodes (local nodes nlA .. nlA + nn - 1, nn <= 64)
  const unsigned long long byzm = __ballot(lane < wd.nn && is_byz(p.byz, p.n0 + wd.nlA + lane));
  const uint32_t bpat = byz_pattern(p.round + 1u);
  const __amdgpu_buffer_rsrc_t ta =
      __builtin_amdgcn_make_buffer_rsrc(p.planes + (size_t)t0 * (kPlanes * 64u), 0, (int)(ntiles * kPlanes * 64u * 4u),
                                        kRsrcWord3);
  const uint32_t aoff = (1536u + lane) * 4u;
  // reference words of this lane's block: the snapshot being written is flagged against rin, the
  // flags of the snapshot being read (prefetched for the run's nodes: wd.flagok) against rprev
  const bool rd = REF && p.rflag_in && wd.flagok != 0ull;
  const uint32_t rprev = rd ? at_byte(p.pref_prev, p.ref_node * p.PS * 4u + bo) : 0u;
  const uint32_t rin = (REF && p.rflag_out) || p.uni_out ? at_byte(p.pref_in, p.ref_node * p.PS * 4u + bo) : 0u;
  uint32_t done = 0u, umis = 0u;
  uint32_t applied = 0u, bytes = 0u, reread = 0u;  // per lane
  for (uint32_t i = 0; i < ntiles; ++i) {
    const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)wd.meta, (int)i);
    // (a run holding a Byzantine node leaves its calm tiles to the general path, as settled_run_uni
    // leaves all of its tiles: existing byte pins of small Byzantine networks rest on their regather)
    if (!settled_cand(m, byzm ? 0u : p.calm)) continue;
    const uint32_t tile = t0 + i;
    const uint32_t A = __builtin_amdgcn_raw_buffer_load_b32(ta, aoff + i * (kPlanes * 64u * 4u), 0, POL > 0 ? 2 : 0);
    const uint32_t g = tile * 64u + lane;
    const bool active = g < p.L;
    const uint32_t nl = (active ? g : p.L - 1u) >> p.bl_log2;
    const uint32_t P0 = active ? vw : 0u;  // polled = live (kPendAllLive) and valid
    const uint32_t rel = nl - wd.nlA;
    uint32_t rows[8];
    {
      const uint32_t* q = wd.sdc + rel * 8u;
      const u32x4 lo = *reinterpret_cast<const u32x4*>(q);
      const u32x4 hi = *reinterpret_cast<const u32x4*>(q + 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        rows[c] = lo[c];
        rows[c + 4] = hi[c];
      }
    }
    uint32_t dis = 0u, all = ~0u;
    bool gather = true;
    if (rd) {
      const uint32_t base = rel * 2u + wd.fofs;  // the node's producer lanes
      const bool fl = ((wd.flagok >> base) & 3ull) == 3ull;
      if (__ballot(active && !fl) == 0ull) {
        dis = all = rprev;
        gather = false;
      }
    }
    if (gather) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w = at_byte(p.pref_in, rows[j] + bo);
        dis |= w;
        all &= w;
      }
    }
    // every vote equals A  <=>  (OR of votes) == A == (AND of votes) on P0
    if (__ballot(((dis ^ A) | (all ^ A)) & P0) != 0ull) continue;
    const uint32_t node = p.n0 + nl;
    const uint32_t pub = ((byzm >> rel) & 1ull) ? bpat : A;
    if (active) {
      umis |= pub != rin ? 1u : 0u;
      const uint32_t prow = node * p.PS + b;  // < N * PS < 2^30 (sweep gate)
      const bool known = (m & 0xFFu) >= 2u;  // (publish)
      publish<POL, CC>(p, prow, pub, ((byzm >> rel) & 1ull) ? byz_pattern(p.round - 2u) : pub, acc, known, nl, i);
    }
    if (REF && p.rflag_out) ref_flag_store(p, lane, active, b, node, pub, rin);
    done |= 1u << i;
    applied += 8u * (uint32_t)__popc(P0);
    // settled_tile's accounting: 40 B per active lane (+ 4 B push read), 28 of the 32 gathered re-read;
    // reference rows: the 8 flag bytes per node instead of the 32 B of votes, the flag byte written
    bytes += active ? 40u + (p.count_changed ? 4u : 0u) - (gather ? 0u : 32u) +
                          (REF && p.rflag_out ? (b == 0u ? 1u : 0u) : 0u)
                    : 0u;
    reread += active && gather ? 28u : 0u;
  }
  // the settled tiles' pending count steps: +1 deferred +8 step each (lane i: tile t0 + i)
  if (lane < ntiles && ((done >> lane) & 1u)) {
    p.kpend[t0 + lane] = pend_next(wd.meta);
    bytes += 8u;  // kpend read (prologue) + written
    bytes += calm_settle(p, t0 + lane, wd.meta);
  }
  acc.applied += applied;
  acc.lane_bytes += bytes;
  acc.reread += reread;
  if (p.uni_out) acc.umis |= umis;
  return done;
}

// The settled candidates of a wave's run when every row of pref_in is ref_node's row of pref_prev
// (uniform rows, kernels.h uni_in): each of a lane's 8 gathered votes would be that row's word
// `refp`, whoever the peers are, so the settled test of settled_run needs no peer draw and no
// gather: every polled record's accepted bit equals refp. Same outputs and accounting as
// settled_run otherwise (the published word, the deferred +8 step); the votes' 32 B per lane are
// not read. Bit i of the result = tile t0 + i settled; the other tiles take the draw and the
// general path.
constexpr uint32_t kUniRun = 16;  // longest run settled_run_uni takes (p.tpw <= 16)

// Everything settled_run_uni reads that depends on no other load (the run's A planes, the validity
// word, the reference row's words, the Byzantine bits), requested in two parts (uni_early,
// uni_prefetch) once the run is known to take the uniform path. (Requested at the start of the wave's
// run, before the uniform test, it measured no faster: 4.24 vs 4.19-4.22 ms per C4 epoch,
// profiles/r05/s14/ab_pre.log: the settled waves are not waiting on that chain.)
struct UniPre {
  uint32_t Av[kUniRun];
  uint32_t vw, refp, rin;
  uint32_t bz[4];  // per lane: node nlA + lane + 64 j is Byzantine (uni_early)
  unsigned long long byzm[4];
};

// The part that depends on no tile word and on no slot word (the validity word, the Byzantine words of
// the run's nodes): requested with the run's tile words, before the uniform test's slot words are
// waited for, so that a quiescent wave, which does little else, waits for two memory latencies (the
// kernel arguments, then everything it reads) and not for three in a row.
__device__ __forceinline__ void uni_early(const RoundParams& p, uint32_t lane, uint32_t nlA, UniPre& u) {
  u.vw = at_byte(p.valid, (lane & (p.BL - 1u)) * 4u);
  // lanes past the run's nodes read the network's last node's word and drop it (uni_prefetch)
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j)
    u.bz[j] = is_byz(p.byz, min(p.n0 + nlA + lane + 64u * j, p.n_nodes - 1u)) ? 1u : 0u;
}

// `qt`: the kernel-uniform part of the quiescent test holds (below, "Quiescent tiles"); the result is
// the run's quiescent tiles (bit i: tile t0 + i), whose A words are not requested (an offset past the
// resource, as for the tiles past the run); a run that is quiescent throughout does not read the
// reference words either. After uni_early.
template <int POL>
__device__ __forceinline__ uint32_t uni_prefetch(const RoundParams& p, uint32_t lane, uint32_t t0, uint32_t tile_end,
                                                 uint32_t nn, uint32_t meta, bool qt, UniPre& u) {
  const uint32_t ntiles = tile_end - t0;
  const uint32_t bo = (lane & (p.BL - 1u)) * 4u;
  uint32_t quiet = 0u;
  if (qt)  // (lanes past the run hold meta = 0)
    quiet = (uint32_t)__ballot((meta & (kPendAllLive | (kVMask << 8))) == (kPendAllLive | (kVUniform << 8)) &&
                               (meta & 0xFFu) >= 2u);
  const __amdgpu_buffer_rsrc_t ta =
      __builtin_amdgcn_make_buffer_rsrc(p.planes + (size_t)t0 * (kPlanes * 64u), 0, (int)(ntiles * kPlanes * 64u * 4u),
                                        kRsrcWord3);
  const uint32_t aoff = (1536u + lane) * 4u;
#pragma unroll
  for (uint32_t i = 0; i < kUniRun; ++i)  // tiles past the run: offset past the resource (reads 0, no access)
    u.Av[i] = __builtin_amdgcn_raw_buffer_load_b32(
        ta, i < ntiles && !((quiet >> i) & 1u) ? aoff + i * (kPlanes * 64u * 4u) : 0x80000000u, 0, POL > 0 ? 2 : 0);
  const bool walk = quiet != run_mask(ntiles);  // wave-uniform: some tile is left to the walk
  u.refp = walk ? at_byte(p.pref_prev, p.ref_node * p.PS * 4u + bo) : 0u;  // every vote word this round
  u.rin = walk && p.uni_out ? at_byte(p.pref_in, p.ref_node * p.PS * 4u + bo) : 0u;
  // the run's Byzantine bits, node nlA + rel at bit rel & 63 of byzm[rel >> 6]: up to 256 nodes (runs of
  // 16 tiles at BL >= 4, the merged runs of uni_merge on target shards)
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) u.byzm[j] = __ballot(lane + 64u * j < nn && u.bz[j] != 0u);
  return quiet;
}

template <int POL, bool CC>
__device__ __forceinline__ uint32_t settled_run_uni(const RoundParams& p, uint32_t lane, uint32_t t0,
                                                    uint32_t tile_end, uint32_t meta, uint32_t nlA, uint32_t nn,
                                                    const UniPre& u, uint32_t quiet, SweepAcc& acc) {
  const uint32_t ntiles = tile_end - t0;
  const uint32_t b = lane & (p.BL - 1u);
  const uint32_t vw = u.vw, refp = u.refp, rin = u.rin;
  // a run holding a Byzantine node is left to the general path (a uniform input with Byzantine voters
  // needs every honest row equal to their flip-flop pattern: rare), so that every settled word here
  // is the tile's A plane, with no per-lane Byzantine-bit lookup per tile
  if ((u.byzm[0] | u.byzm[1] | u.byzm[2] | u.byzm[3]) != 0ull) return 0u;
  if constexpr (!CC) {
    if (quiet) {
      // Quiescent tiles (the essay below): one more deferred +8 step (lane i: tile t0 + i) and the
      // counters; no A word, no published word. 8 B per tile: its kpend word read and written. Every
      // lane is active in every tile but the network's last, which may be partial.
      const bool mine = lane < ntiles && ((quiet >> lane) & 1u);
      if (mine) p.kpend[t0 + lane] = pend_next(meta);
      const uint32_t last = (p.Lpad >> 6) - 1u;  // < t0 + 32 where it is tested (ntiles <= kUniRun)
      const bool cut = last < tile_end && ((quiet >> (last - t0)) & 1u) && last * 64u + lane >= p.L;
      acc.applied += 8u * (uint32_t)__popc(vw) * ((uint32_t)__popc(quiet) - (cut ? 1u : 0u));
      acc.lane_bytes += mine ? 8u : 0u;
      if (quiet == run_mask(ntiles)) return quiet;  // (before the walk over the tile words)
    }
  }
  uint32_t cand = 0u;
  for (uint32_t i = 0; i < ntiles; ++i) {
    const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)meta, (int)i);
    if (settled_cand(m, p.calm)) cand |= 1u << i;
  }
  cand &= ~quiet;
  uint32_t Av[kUniRun];
#pragma unroll
  for (uint32_t i = 0; i < kUniRun; ++i) Av[i] = u.Av[i];
  if constexpr (!CC) {
    // The single-GPU (non-counting) build walks the run with no per-tile branch: a tile is settled iff
    // it is a candidate and no polled record's A differs from the reference word (one ballot, a
    // scalar bit); its published words are stored through a resource bounded to the snapshot, with
    // an out-of-range offset for the lanes that must not store (the store is dropped), and the
    // counters take the settled bit as a factor. Per tile: ~half the scalar instructions of the
    // branching walk (the settled rounds are bound by the CU's scalar issue).
    const __amdgpu_buffer_rsrc_t prb =
        __builtin_amdgcn_make_buffer_rsrc(p.pref_out, 0, (int)(p.n_nodes * p.PS * 4u), kRsrcWord3);
    uint32_t done = 0u, applied = 0u, bytes = 0u, umis = 0u;
    // a tile holds 64 / BL nodes: the lane's node and row advance by constants from tile to tile
    // (lanes past the last lane compute a row they never store)
    const uint32_t npt = 64u >> p.bl_log2;
    const uint32_t rel0 = ((t0 * 64u + lane) >> p.bl_log2) - nlA;
    uint32_t prow = (p.n0 + nlA + rel0) * p.PS + b;  // < N * PS < 2^30 (sweep gate)
#pragma unroll
    for (uint32_t i = 0; i < kUniRun; ++i) {
      const uint32_t g = (t0 + i) * 64u + lane;
      const bool active = g < p.L;
      const uint32_t P0 = active ? vw : 0u;  // polled = live (kPendAllLive) and valid
      const uint32_t A = Av[i];
      const uint32_t mis = __ballot((refp ^ A) & P0) != 0ull ? 1u : 0u;  // always evaluated: no branch
      const bool ok = (((cand >> i) & 1u) & (mis ^ 1u)) != 0u;             // wave-uniform
      const uint32_t pub = A;
      const bool st = ok && active;
      __builtin_amdgcn_raw_buffer_store_b32(pub, prb, st ? prow * 4u : 0xFFFFFFFCu, 0, POL == 1 ? 2 : 0);  // (table < 4 GiB: 0xFFFFFFFC is past it)
      umis |= (st & (pub != rin)) ? 1u : 0u;
      done |= ok ? 1u << i : 0u;
      applied += st ? 8u * (uint32_t)__popc(P0) : 0u;
      bytes += st ? 8u : 0u;  // settled_run's accounting without the 32 B of gathered votes
      prow += npt * p.PS;
    }
    if (lane < ntiles && ((done >> lane) & 1u)) {
      p.kpend[t0 + lane] = pend_next(meta);
      bytes += 8u;  // kpend read (prologue) + written
      bytes += calm_settle(p, t0 + lane, meta);
    }
    acc.applied += applied;
    acc.lane_bytes += bytes;
    if (p.uni_out) acc.umis |= umis;
    return done | quiet;
  }
  uint32_t done = 0u, applied = 0u, bytes = 0u, umis = 0u;
#pragma unroll
  for (uint32_t i = 0; i < kUniRun; ++i) {
    if (!((cand >> i) & 1u)) continue;
    const uint32_t tile = t0 + i;
    const uint32_t A = Av[i];
    const uint32_t g = tile * 64u + lane;
    const bool active = g < p.L;
    const uint32_t nl = (active ? g : p.L - 1u) >> p.bl_log2;
    const uint32_t P0 = active ? vw : 0u;  // polled = live (kPendAllLive) and valid
    if (__ballot((refp ^ A) & P0) != 0ull) continue;
    const uint32_t node = p.n0 + nl;
    const uint32_t pub = A;
    if (active) {
      umis |= pub != rin ? 1u : 0u;
      const uint32_t prow = node * p.PS + b;  // < N * PS < 2^30 (sweep gate)
      // kpend >= 2: this settled tile's accepted plane is unchanged since the snapshot being
      // overwritten (publish): honest rows publish that word again, Byzantine rows its pattern's
      const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)meta, (int)i);
      const bool known = (m & 0xFFu) >= 2u;
      publish<POL, CC>(p, prow, pub, pub, acc, known, nl, i);
    }
    done |= 1u << i;
    applied += 8u * (uint32_t)__popc(P0);
    // settled_run's accounting without the 32 B of gathered votes: A read, valid, published word
    bytes += active ? 8u + (p.count_changed ? 4u : 0u) : 0u;
  }
  if (lane < ntiles && ((done >> lane) & 1u)) {
    p.kpend[t0 + lane] = pend_next(meta);
    bytes += 8u;  // kpend read (prologue) + written
    bytes += calm_settle(p, t0 + lane, meta);
  }
  acc.applied += applied;
  acc.lane_bytes += bytes;
  if (p.uni_out) acc.umis |= umis;
  return done;
}

// Quiescent tiles (p.quiet_tiles, option "quiet_tiles", default 1; the single-engine build, CC ==
// false; 0 restores the walk of every settled tile). A tile of a wave's run is quiescent in round r
// when
//  * it is a settled candidate as settled_run_uni tests it (kPendAllLive, kVUniform),
//  * its incoming pend (kpend low byte) is >= 2: it deferred its count step in rounds r - 1 and r - 2,
//  * `uniform` and `prev_uni` hold: every row of pref_in is the reference row of pref_prev, and every
//    row of pref_prev the reference row of the snapshot before it (whatever option uni_votes says),
//  * its run holds no Byzantine node (settled_run_uni's own gate).
// Then (1) the reference node's row of pref_prev is one of "every row" of it, so this round's vote
// word w is last round's w'; (2) the tile deferred in r - 1, which process_tile, settled_run and
// settled_run_uni grant only when every polled record agreed with all 8 votes and nothing flipped
// (a calm tile, kernels.h calm, that settles is no exception: all 8 votes equalled A, A is unchanged
// and the tile deferred; it becomes kVUniform then, with pend as any other tile's, so it reaches the
// pend >= 2 asked for here two rounds after it first settles, and is no candidate here before):
// A & P0 == w' & P0 at the end of r - 1, and A has not changed since, so the settled test of round r
// holds before A is loaded; (3) pref_out is the ring buffer that held the snapshot of round r - 2's
// input: every row of it is the row's A plane at the start of r - 2 (published by round r - 3, or by
// the call that rewrote the records since), and a tile that deferred in r - 2 and r - 1 still has
// that A: the store would rewrite the word already there (the fact `known` in process_tile and the
// need-masked peer pushes are built on). More: the tile's own row of pref_in, published in r - 1, is
// its A and is a uniform row, so A equals the reference word of pref_in on the whole word: no
// mismatch to tag (umis). A quiescent tile's one effect is pend + 1 and the applied / byte counters
// (8 B: its kpend word read and written); rows, V, A, K, the log and the uniform tag stay.
// Threshold: pend >= 2, the least for (3); (2) alone needs pend >= 1.
//
// Reference-row flags (REF): the settled tiles of a uniform round write none already
// (settled_run_uni does not), and a flag byte carries its snapshot's tag (ref_tag), so the byte a
// quiescent tile leaves in pref_out's flags is three rounds old and reads as "unflagged": gather.
//
// Everything else that writes kpend, a record plane, the validity words or a snapshot row, and why
// no tile is taken as quiescent afterwards while its row of pref_out or its A differs from what
// the walk would publish. Two guards: a write-back clears pend (k_materialize, launched by
// materialize in engine.cpp, zeroes every kpend word), so two deferred
// rounds must follow it; facts.snapshot_written drops uni_ok of all three buffers, so `uniform` is false in
// the next round and prev_uni in the next two.
//  * av_register_votes(_batch), av_add_targets(_batch), av_admit_targets, av_write_records: materialize_votes first (pend = 0,
//    kPendAllLive gone) and facts.snapshot_written; they republish the rows they change into the current
//    snapshot (k_register_votes, k_add_lanes, k_admit_blocks / k_admit_lanes, refresh_pref), which is pref_out three rounds later:
//    (3) holds with "the call that rewrote the records".
//  * av_set_valid: materialize_votes (pend = 0) and facts.snapshot_written; A and the rows are untouched, and
//    the new polled set is first seen by the general path (kPendAllLive cleared).
//  * av_init_records: kpend zeroed, facts.snapshot_written, every plane and the current snapshot rewritten;
//    the fresh round after it defers nothing (klazy needs a warm round).
//  * av_materialize and every other write-back: pend = 0. av_read_records, av_census, av_read_pref
//    read through the deferred forms and write nothing.
//  * av_set_option (every option, this one too): facts.snapshot_written; count_lazy and k_hi_virtual write
//    back first; responder republishes and leaves the sweep.
//  * the replay, capped and first-generation round kernels, and a sweep round that is not klazy:
//    launch_one_round / launch_replay_fused write the counts back first (pend = 0) and leave
//    uni_ok of the buffer they write false (replay, capped: uni is false) or run the kconsume round,
//    which clears kpend itself.
//  * peer pushes, the barrier's slot copy and RCCL gathers write snapshot buffers of node-sharded
//    engines only: those run the CC build, which has no quiescent path.
//
// Network-quiet rounds (p.nq_in, option "net_quiet", default 1; the single-engine build of the walking
// warm mode with runs, as the quiescent tiles). The induction: let every wave that owns tiles in round
// r - 1 find its whole run quiescent (or round r - 1 take this path). Then round r - 1 stored no
// snapshot row, no uniform tag, no plane, no validity word and no vstale word; every kpend word kept
// kPendAllLive and its pend grew by one (>= 3 now). If round r is again a klazy round of the same
// engine and nothing but reads happened in between, then in round r
//  * the run geometry, the Byzantine words and the validity words are those of round r - 1: every run is
//    free of Byzantine nodes and every tile a settled candidate (kVUniform, kPendAllLive), pend >= 2;
//  * pref_in was not written by round r - 1: its rows are what pref_prev held (points (1)-(3) of the
//    quiescent tiles say a quiescent tile would have stored the word already there), and the kernel
//    still tests both uniform slots, which no round since has tagged;
// so every tile is quiescent in round r by the three points above, and its one effect is pend + 1, the
// applied votes and its 8 B. The word: a wave that owns tiles and is not quiescent throughout (general
// tiles, the settled walk, settled_run, a Byzantine node in the run, a non-uniform snapshot, every
// other mode of this kernel) stores the tag p.round + 1 into p.nq_out at its end; a quiescent wave and a
// wave of this path store nothing. Round r reads round r - 1's word (the other of two, by round parity:
// a wave of round r tagging the word that round r still reads would hide round r - 1's tag); a tag
// from an older round is smaller than p.round (rounds only grow) and never reads as this one.
// Who may invalidate the induction between two rounds, and where nq_ok (round_plan.h) is cleared:
//  * every caller of facts.snapshot_written: av_set_valid, av_add_targets(_batch), av_admit_targets, av_register_votes(_batch),
//    av_write_records, av_init_records (facts.init), av_set_option (every option: the run geometry, the
//    path's own switches), av_set_polling, responder and exchange set-up, the replay launches;
//  * every write-back (materialize in engine.cpp: av_materialize, and what any reader or writer of
//    counts asks for first): kpend = 0, and this path does not test pend >= 2;
//  * after_round of any round that did not maintain the word: non-klazy (the kconsume round, rounds
//    near finalization), fresh, replay, capped and first-generation rounds, engines with an exchange
//    or with count_changed (the CC build);
//  * av_read_records, av_read_pref, av_census, the log readers and av_discard_updates write none of
//    the above and leave nq_ok as it is.
// The leader waves (G = p.nq_group; p.nq_front: the grid's first waves, else wave0 % G == 0) take G
// consecutive runs: up to 256 kpend words, one lane per tile, all chunks requested before the first is
// waited for. Counters as the per-run quiescent
// path of settled_run_uni: 8 B per tile; 8 votes per polled record, every lane of every tile but the
// network's last (possibly partial) tile being active.
constexpr uint32_t kNqChunks = 4;  // 64 tiles each: G <= 16 runs of <= 16 tiles
__device__ __forceinline__ void net_quiet_run(const RoundParams& p, uint32_t lane, uint32_t t0, uint32_t tile_end,
                                              SweepAcc& acc) {
  const uint32_t n = tile_end - t0;  // <= 256
  const uint32_t vw = at_byte(p.valid, (lane & (p.BL - 1u)) * 4u);
  uint32_t kw[kNqChunks];
#pragma unroll
  for (uint32_t c = 0; c < kNqChunks; ++c) kw[c] = c * 64u + lane < n ? p.kpend[t0 + c * 64u + lane] : 0u;
  uint32_t mine = 0u;
#pragma unroll
  for (uint32_t c = 0; c < kNqChunks; ++c) {
    if (c * 64u + lane < n) {
      p.kpend[t0 + c * 64u + lane] = pend_next(kw[c]);
      ++mine;
    }
  }
  const uint32_t last = (p.Lpad >> 6) - 1u;
  const bool cut = last < tile_end && last * 64u + lane >= p.L;  // (t0 <= last: the wave owns a tile)
  acc.applied += 8u * (uint32_t)__popc(vw) * (n - (cut ? 1u : 0u));
  acc.lane_bytes += 8u * mine;
}

}  // namespace
}  // namespace avk
