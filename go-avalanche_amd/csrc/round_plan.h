// Host-side round planning: what the engine knows about its records (RecordFacts), the decision a
// round derives from it (plan_round) and the sweep grid's arithmetic (sweep_grid). Pure C++17, no HIP
// include: host/round_plan_test.cpp checks it without a GPU. A round that plans klazy, vv or fresh on
// a wrong fact corrupts records silently, so every fact changes only through the transitions below.
#pragma once

#include <algorithm>
#include <cstdint>

namespace avk {

enum class RoundKernel : int {
  Sweep,     // k_round_sweep (uncapped, k <= 8)
  Node,      // k_round_node (capped, k <= 8)
  FirstGen,  // k_round_fast / k_round_capped (any k; responder variants, non-polling nodes, A/B)
  Lossy,     // k_round_lossy (uncapped, any k): lost Responses and unresponsive nodes (rule R5)
  Listed,    // k_round_listed (uncapped, any k): per-node peer lists (rule R6), with or without R5
};

// The sweep kernel's build, as far as the records decide it. The launcher (sweep_kernel.h
// launch_sweep_k) adds what depends on the grid alone: Warm runs as the walking kModeWarm or, on a
// resident grid smaller than the tile count, as kModeWarmPipe.
enum class SweepMode : int { Replay, Ablate, Fresh, Warm, Check };

struct PlanShape {
  int k;
  uint32_t BL;
  int64_t N;
  uint32_t NL, PS;
  bool capped;
  int peer_world;
  bool has_comm;  // an RCCL communicator exchanges the rows
  int32_t pub_mode;
  bool any_nopoll;
  // rule R5 (av_set_loss, av_set_responding): some Response of a sim round may be lost (a loss
  // threshold above 0 or a node marked not responding); loss_neutral: a lost Response arrives with
  // neutral votes (AV_LOSS_NEUTRAL) instead of not at all
  bool lossy = false, loss_neutral = false;
  // rule R6 (av_set_peer_lists): every local node polls from its own peer list
  bool listed = false;
};

// the options the decision reads (av_set_option)
struct PlanKnobs {
  int kernel;
  bool virtual_votes;
  uint32_t vv_min_bl;
  bool count_lazy, k_hi_virtual, ref_rows, uni_rows, ablate_gather, unsynced_shard;
  // the network-quiet word (kernels.h nq_*): options "quiet_tiles" and "net_quiet"; count_changed: the
  // sweep's counting build runs (option "count_changed"), which has no quiescent path
  bool quiet_tiles = true, net_quiet = true, count_changed = false;
  bool calm_tiles = true;  // option "calm_tiles" (kernels.h RoundParams::calm)
};

struct RoundPlan {
  // responder variant 2 or non-polling nodes on a capped engine, or a lossy (R5) or listed (R6) round
  // of a capped engine, of responder variant 2 or of a peer-push engine: no kernel runs them
  bool unsupported;
  RoundKernel kernel;
  SweepMode mode;  // kernel == Sweep
  int k;
  bool replay, capped;
  bool fresh;       // planes known to be zero are not read (kernels.h fresh)
  bool warm;        // every consider plane all-ones: the sweep's warm sim modes
  bool vv;          // vote planes left unstored (kernels.h vv)
  bool vv_uniform;  // below vv_min_bl only the uniform form (a settled tile's V = A: nothing to regather)
  bool klazy;       // count planes deferred (kernels.h klazy)
  bool kconsume;    // the first warm round that can finalize applies the pending steps itself
  bool hivirt;      // kernels.h kHiVirt
  bool exact_pass;  // capped: a count may have reached 120
  // deferred state the round cannot read through, written back before the launch
  bool wb_votes, wb_counts;
  // the stored consider planes still stand for ~real_mask (RecordFacts::c_preset) and the round is
  // not the fresh sweep round that makes them true: they are stored explicitly before the launch
  bool wb_cpreset;
  // reference rows / uniform rows may be used; the caller clears these when no honest reference
  // node exists (ref_pick reads the device)
  bool ref_rows, uni_rows;
  // the network-quiet word (kernels.h nq_*). net_quiet_out: the round maintains this round's word (a
  // klazy sweep round of a single engine with quiet_tiles on); net_quiet_in: the word the round before
  // wrote may be trusted (facts.nq_ok)
  bool net_quiet_out, net_quiet_in;
  // calm tiles (kernels.h calm): a klazy sweep round at k = 8 whose tiles may be left stale (vv, not
  // the uniform-only form) flags them kVCalm and takes flagged tiles as settled candidates
  bool calm;
  // a sim round under R5 (kernel == Lossy); loss_neutral: its lost Responses shift in consider = 0
  bool lossy, loss_neutral;
  // a sim round over peer lists (kernel == Listed); lossy / loss_neutral then say whether R5 applies
  // to its non-empty slots and how
  bool listed;
};

struct RecordFacts {
  // every consider bit ever shifted in was 1 (no replay, no neutral drop-in
  // vote, no write_records): an all-ones oldest consider plane implies all
  // consider planes are all-ones (lets k_round_fast skip them)
  bool c_monotone = true;
  // every consider plane of every lane is all-ones: set after a sim round with k >= 8 in which every
  // live record was polled (all targets valid, uncapped); cleared by anything that can write a 0
  // consider bit (init, add, write_records, drop-in votes, replay)
  bool warm_all = false;
  // every record is a NewVoteRecord from av_init_records (votes = consider =
  // count = 0): the next sweep round reads only the A plane (kernels.h fresh)
  bool fresh = false;
  // upper bound on any live record's count (confidence >> 1) at the start of the next round: a
  // round adds at most k, init/add start at 0, anything else sets it to 127. While it is < 120 no
  // record can finalize in the next round (k <= 8), so the capped path skips its exact pass.
  int count_bound = 127;
  // every lane's stored consider planes are all-ones and stand for ~real_mask (consider = 0 on every
  // existing record): av_init_records stored what the fresh sweep round would leave behind (after 8
  // sim votes every consider bit is 1), so that neither that round nor the first write-back stores
  // them. Implies fresh. Set by init alone; cleared by after_round and by c_unpreset, which goes with
  // the pass that stores the planes explicitly. Every other transition that clears fresh (adds,
  // drop-in votes, writes, option "fresh" = 0) is entered only after that pass.
  bool c_preset = false;
  bool v_stale = false;  // some tile may be stale
  bool k_pend = false;   // some tile may hold pending steps or flags
  // rflag_ok[b]: the reference-row flags of snapshot buffer b were written by the round that wrote
  // its rows, against ref_node's row of the buffer that round read, and nothing has written either
  // buffer since
  bool rflag_ok[3] = {false, false, false};
  // uni_ok[b]: buffer b was written by a sweep round that tagged its uniform-row slots
  bool uni_ok[3] = {false, false, false};
  // the network-quiet word of the last round (kernels.h nq_in) says whether some run of that round was
  // not quiescent, and nothing has written a record plane, a tile word, a validity word, a snapshot
  // row or an option since: set by after_round of a klazy sweep round that maintained the word,
  // cleared by everything else listed in sweep_settled.h ("Network-quiet rounds")
  bool nq_ok = false;

  // Anything but a reference-row sweep round that writes a snapshot buffer
  // (drop-in votes, adds, writes, init, validity/publish-rule refreshes, peer
  // and RCCL set-up, other round kernels) leaves its flags stale.
  void snapshot_written() {
    rflag_ok[0] = rflag_ok[1] = rflag_ok[2] = false;
    uni_ok[0] = uni_ok[1] = uni_ok[2] = false;
    nq_ok = false;
  }
  // av_init_records: every plane is rewritten (the caller clears the tile words of what was deferred).
  // Every record starts at count 0 with no considered vote (NewVoteRecord, vote.go:33-35), and a
  // count step needs > 6 considered votes in the 8-vote window (vote.go:58-61): the first 6 votes
  // of a fresh record cannot step it, so after v votes every count is <= v - 6
  // preset: the consider planes were stored as all-ones (c_preset; only with records, and only where
  // the next sim round plans as a fresh sweep round: plans_c_preset below)
  void init(bool records_created, bool preset = false) {
    snapshot_written();
    warm_all = false;
    count_bound = -6;
    v_stale = k_pend = false;
    fresh = records_created;
    c_preset = records_created && preset;
  }
  // the consider planes were stored explicitly (C = ~real_mask on every lane)
  void c_unpreset() {
    c_preset = false;
    nq_ok = false;
  }
  void add_targets() {
    warm_all = false;
    fresh = false;
    nq_ok = false;
  }
  // drop-in votes: at most one confidence step per vote, so the most votes one node gets bound the
  // counts; a neutral vote shifts in consider = 0
  void dropin_votes(int64_t max_node_votes, bool any_neutral) {
    fresh = false;
    count_bound = (int)std::min<int64_t>(127, count_bound + max_node_votes);
    if (any_neutral) c_monotone = false;
    nq_ok = false;
  }
  void write_records() {
    nq_ok = false;
    c_monotone = false;
    fresh = false;
    count_bound = 127;  // arbitrary counts written
  }
  void replay_call() {  // replayed votes may be neutral
    c_monotone = false;
    nq_ok = false;
  }
  // a write-back zeroes the tile words (pend = 0), which the network-quiet path does not look at
  void votes_written_back() {
    v_stale = false;
    nq_ok = false;
  }
  void counts_written_back() {
    k_pend = false;
    nq_ok = false;
  }
  // the responders' re-adds (pub_mode 2) create records after the round's votes
  void responder_readds() {
    nq_ok = false;
    warm_all = false;
    count_bound = 127;
  }
  void option_fresh_off() { fresh = false; }          // option "fresh" = 0
  void option_warm_skip_off() { c_monotone = false; }  // option "warm_skip" = 0: may only be switched off
  // A round ran by `p` and published snapshot buffer out_buf. all_valid: every target of the shard is
  // valid; refw: the launch wrote reference-row flags for the snapshot it published.
  void after_round(const RoundPlan& p, bool all_valid, bool refw, int out_buf) {
    if (p.vv) v_stale = true;
    if (p.klazy) k_pend = true;
    if (p.kconsume) k_pend = false;
    if (p.fresh && p.hivirt) k_pend = true;  // the fresh round flags its tiles kHiVirt
    count_bound = std::min(127, count_bound + p.k);
    fresh = false;
    c_preset = false;  // a fresh sweep round made the stored planes true; any other was preceded by c_unpreset
    rflag_ok[out_buf] = p.ref_rows && refw;
    uni_ok[out_buf] = p.uni_rows;
    // (every other kind of round: non-klazy, replay, capped, first-generation, an engine with an exchange)
    nq_ok = p.net_quiet_out;
    if (p.lossy || p.listed) {
      // a skipped Response or an empty slot leaves a record short of 8 new votes, a neutral Response
      // shifts in consider = 0 (vote.go:56); the round tags no snapshot buffer
      snapshot_written();
      warm_all = false;
      if (p.loss_neutral) c_monotone = false;
    } else if (p.replay)
      warm_all = false;
    else if (c_monotone && p.k >= 8 && !p.capped && all_valid)
      warm_all = true;  // every live record was polled and shifted in 8 considered votes
  }
};

// The whole per-round decision, a pure function of its arguments.
inline RoundPlan plan_round(const RecordFacts& f, const PlanShape& s, const PlanKnobs& o, bool replay) {
  RoundPlan r{};
  r.k = s.k;
  r.replay = replay;
  r.capped = s.capped;
  // responder variants and non-polling nodes run the first-generation kernels
  const bool compat = s.pub_mode != 0 || s.any_nopoll;
  r.unsupported = compat && s.capped && (s.pub_mode == 2 || s.any_nopoll);
  // the sweep addresses the preference table by 32-bit byte offsets
  const bool sweep = o.kernel == 2 && s.k <= 8 && !s.capped && !compat && (uint64_t)s.N * s.PS < (1ull << 30);
  r.kernel = sweep                                             ? RoundKernel::Sweep
             : o.kernel == 2 && s.k <= 8 && s.capped && !compat ? RoundKernel::Node
                                                                : RoundKernel::FirstGen;
  const bool ones = f.c_monotone && f.warm_all;
  // the round after av_init_records: planes known to be zero are not read
  r.fresh = f.fresh && sweep && !replay && !o.ablate_gather;
  r.warm = sweep && !replay && ones && !o.ablate_gather && !r.fresh;
  r.mode = replay            ? SweepMode::Replay
           : o.ablate_gather ? SweepMode::Ablate
           : r.fresh         ? SweepMode::Fresh
           : ones            ? SweepMode::Warm
                             : SweepMode::Check;
  // vote planes may be left unstored: warm (or fresh) k = 8 sim rounds
  r.vv = o.virtual_votes && s.k == 8 && (r.warm || r.fresh);
  r.vv_uniform = r.vv && s.BL < o.vv_min_bl;
  // count planes may be deferred: warm k = 8 sim rounds while no record can
  // finalize (every true count < 120 at round start)
  r.klazy = o.count_lazy && r.warm && s.k == 8 && f.count_bound < 120;
  r.kconsume = !r.klazy && f.k_pend && r.warm && s.k == 8;
  r.hivirt = o.k_hi_virtual && s.k == 8;
  r.exact_pass = f.count_bound >= 120;
  r.wb_votes = !r.vv && f.v_stale;
  r.wb_counts = !r.klazy && !r.kconsume && f.k_pend;
  r.wb_cpreset = f.c_preset && !r.fresh;
  // reference rows: sweep rounds at k = 8 with a node's lanes inside one wave
  const bool tagged = sweep && s.k == 8 && !replay && !s.has_comm && !o.ablate_gather;
  r.ref_rows = o.ref_rows && tagged && 64 % s.BL == 0;
  // uniform rows: a node-sharded engine sees every row only through the peer exchange, whose pushes
  // carry the slots (unsynced_shard, diagnostics: a rank's share alone, on its own slot)
  r.uni_rows = o.uni_rows && tagged && (s.NL == (uint32_t)s.N || s.peer_world > 1 || o.unsynced_shard);
  // the network-quiet word: the single-engine build of the klazy sweep (no exchange, no counting); a
  // round that cannot be uniform (no uniform rows) still maintains it, by tagging it in every wave
  r.net_quiet_out = o.quiet_tiles && o.net_quiet && r.klazy && sweep && !o.count_changed && s.peer_world <= 1 && !s.has_comm;
  r.net_quiet_in = r.net_quiet_out && f.nq_ok;
  r.calm = o.calm_tiles && r.klazy && r.vv && !r.vv_uniform && s.k == 8 && sweep;
  // R5: a sim round with lost Responses runs k_round_lossy on the stored planes alone; it neither
  // reads nor leaves a deferred form, so the write-back rules above see none of them planned. Replay
  // rounds ignore the setting (their stream carries its own neutral votes).
  if (s.lossy && !replay) {
    r.lossy = true;
    r.loss_neutral = s.loss_neutral;
    r.unsupported = r.unsupported || s.capped || s.pub_mode == 2 || s.peer_world > 1;
    r.kernel = RoundKernel::Lossy;
    r.mode = SweepMode::Check;
    r.fresh = r.warm = r.vv = r.vv_uniform = r.klazy = r.kconsume = r.calm = false;
    r.ref_rows = r.uni_rows = r.net_quiet_out = r.net_quiet_in = false;
    r.wb_votes = f.v_stale;
    r.wb_counts = f.k_pend;
    r.wb_cpreset = f.c_preset;
  }
  // R6: a sim round over peer lists runs k_round_listed, planned as R5's round is: on the stored
  // planes alone, whether or not a Response can be lost as well (loss_neutral only where one can).
  // Replay rounds ignore the lists.
  if (s.listed && !replay) {
    r.listed = true;
    r.lossy = s.lossy;
    r.loss_neutral = s.lossy && s.loss_neutral;
    r.unsupported = r.unsupported || s.capped || s.pub_mode == 2 || s.peer_world > 1;
    r.kernel = RoundKernel::Listed;
    r.mode = SweepMode::Check;
    r.fresh = r.warm = r.vv = r.vv_uniform = r.klazy = r.kconsume = r.calm = false;
    r.ref_rows = r.uni_rows = r.net_quiet_out = r.net_quiet_in = false;
    r.wb_votes = f.v_stale;
    r.wb_counts = f.k_pend;
    r.wb_cpreset = f.c_preset;
  }
  return r;
}

// av_init_records may preset the consider planes (RecordFacts::c_preset) iff the next sim round of
// the newly created records would plan as a fresh sweep round: never on capped engines, responder
// variants, non-polling networks, kernel 1 or ablate_gather.
inline bool plans_c_preset(const PlanShape& s, const PlanKnobs& o) {
  RecordFacts f;
  f.init(true);
  const RoundPlan r = plan_round(f, s, o, false);
  return r.fresh && !r.unsupported;
}

// The sweep grid over `tiles` 64-lane tiles: `blocks` resident workgroups of 4 waves (0 = one wave
// per tile), never more than the tiles need; each wave owns a run of `run` consecutive tiles (or, for
// runs the kernel does not take, walks the same number with the grid's stride).
struct SweepGrid {
  uint32_t grid, run;
};
inline SweepGrid sweep_grid(uint32_t tiles, uint32_t blocks) {
  const uint32_t need = (uint32_t)(((uint64_t)tiles + 3u) / 4u);
  const uint32_t grid = std::max(1u, blocks ? std::min(blocks, need) : need);
  const uint64_t waves = (uint64_t)grid * 4u;
  return {grid, (uint32_t)((tiles + waves - 1u) / waves)};
}
// waves of that grid that own a run (the fewest that write the StatusUpdate log)
inline uint64_t sweep_run_waves(uint32_t tiles, uint32_t blocks) {
  const uint64_t run = std::max(1u, sweep_grid(tiles, blocks).run);
  return std::max<uint64_t>(1, (tiles + run - 1u) / run);
}

}  // namespace avk
