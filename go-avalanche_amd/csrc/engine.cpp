// libavhip.so — C ABI (include/avhip.h) over the CDNA4 kernels (csrc/*.hip, kernels.h).
//
// The engine owns all device memory: the bit-sliced VoteRecord planes, the two
// published-preference snapshots, validity / Byzantine bitsets, the sharded
// StatusUpdate log and the applied-vote counters. Host buffers passed in are
// only read or written for the duration of the call.
//
// This file: what a round launches (the plan, the parameters, the grids, the log layout), engine
// creation and destruction, and the option table. The other host files are listed in engine.h.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "engine.h"

using namespace aveng;

namespace aveng {

static thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int set_device(av_engine* e) {
  AV_CHECK(e, AV_ERR_INVALID_ARG, "null engine");
  AV_HIP(hipSetDevice(e->cfg.device));
  return AV_OK;
}

avk::RoundParams round_params(const av_engine* e, const uint32_t* replay) {
  avk::RoundParams p{};
  p.planes = e->planes;
  p.pref_in = e->pref[e->cur];
  p.pref_out = e->pref[av_engine::nxt(e->cur)];
  p.pref_prev = e->pref[av_engine::prv(e->cur)];
  p.vstale = e->vstale;
  p.valid = e->valid;
  p.byz = e->byz;
  p.replay = replay;
  p.log = e->log;
  p.log_count = e->log_count;
  p.dlog = e->dlog;
  p.dlog_count = e->dlog_count;
  p.upd_count = e->upd_count;
  p.dlog_cap = e->dlog_cap;
  p.mlog = e->mlog;
  p.mlog_count = e->mlog_count;
  p.mlog_cap = e->mlog_cap;
  p.log_overflow = e->log_overflow;
  p.applied = e->applied;
  p.bytes = e->bytes;
  p.finalized = e->finalized;
  p.warm_skip = e->facts.c_monotone ? 1u : 0u;
  p.plane_nt = e->plane_nt ? 1u : 0u;
  p.ablate_gather = e->ablate_gather ? 1u : 0u;
  p.ablate_emit = (uint32_t)e->ablate_emit;
  p.ablate_phase = e->ablate_phase;
  p.ablate_node = e->ablate_node;
  p.mat_run = e->mat_run;
  p.tile_draw = e->tile_draw;
  p.seed = e->cfg.seed;
  p.log_cap = e->log_cap;
  p.log_shards = e->log_shards;  // a power of two (set_log_layout): the sweep kernel masks by it
  p.n_nodes = (uint32_t)e->N;
  p.n0 = (uint32_t)e->n0;
  p.NL = e->NL;
  p.BL = e->BL;
  p.PS = e->PS;
  p.L = e->L;
  p.Lpad = e->Lpad;
  p.t0 = (uint32_t)e->t0;
  p.round = (uint32_t)e->round;
  p.round_rel = (uint32_t)(e->round - e->log_base);
  p.round_shift = e->round_shift;
  p.peer_mode = e->cfg.peer_mode;
  p.warm_all = e->facts.warm_all ? 1u : 0u;
  p.store_policy = e->store_policy;
  p.bl_magic = e->bl_magic;
  p.bl_sh1 = e->bl_sh1;
  p.bl_sh2 = e->bl_sh2;
  p.kpend = e->kpend;
  p.tn = (uint32_t)(e->t1 - e->t0);
  p.nopipe = e->sweep_nopipe ? 1u : 0u;
  p.tpw = e->wave_runs && e->sweep_blocks ? 1u : 0u;
  p.settled_fast = e->settled_fast ? 1u : 0u;
  p.lean = e->settled_lean && 64 % e->BL == 0 ? 1u : 0u;
  p.bl_log2 = (uint32_t)__builtin_ctz(e->BL);
  p.pub_mode = (uint32_t)e->pub_mode;
  p.readd = e->pub_mode == 2 ? e->readd : nullptr;
  p.died_out = e->pub_mode == 2 ? e->died_out : nullptr;
  p.nopoll = e->any_nopoll ? e->nopoll : nullptr;
  p.dense_min = e->dense_min;
  p.wave_dense = e->wave_dense;
  p.uni_votes = e->uni_votes;
  p.quiet_tiles = e->quiet_tiles;
  return p;
}

// Write back deferred state, one k_materialize pass. votes: the vote planes of tiles the last warm
// k = 8 sim round left stale (kernels.h vv); every path that reads or writes records other than such
// a round asks for them first. counts: the pending +8 steps of deferred count planes (kernels.h
// klazy); every path that reads or writes counts other than a klazy round asks for them first.
int materialize(av_engine* e, bool votes, bool counts) {
  // preset consider planes (kernels.h c_preset) go with the votes: stored explicitly, in a pass of
  // their own (no round has run since av_init_records, so nothing else is deferred)
  if (votes && e->facts.c_preset) {
    AV_HIP(avk::launch_c_unpreset(e->planes, e->BL, e->L, (uint32_t)(e->t1 - e->t0), e->stream));
    e->facts.c_unpreset();
  }
  votes = votes && e->facts.v_stale;
  counts = counts && e->facts.k_pend;
  if (!votes && !counts) return AV_OK;
  AV_HIP(avk::launch_materialize(round_params(e, nullptr), votes, counts, e->stream));
  if (votes) e->facts.votes_written_back();
  if (counts) e->facts.counts_written_back();
  return AV_OK;
}
int materialize_votes(av_engine* e) { return materialize(e, true, true); }

// Growable device scratch owned by the engine.
int engine_scratch(av_engine* e, size_t bytes, void** out) {
  const hipError_t he = e->fetch_scratch.reserve(bytes);
  AV_CHECK(he == hipSuccess, oom_or_hip(he), "scratch (%zu B): %s", bytes, hipGetErrorString(he));
  *out = e->fetch_scratch;
  return AV_OK;
}

// The reference node: the first honest node (a Byzantine row changes every
// round and would never match).
int ref_pick(av_engine* e) {
  if (e->ref_node != -1) return AV_OK;
  e->ref_node = -2;
  const size_t words = std::min<size_t>((e->N + 31) / 32, 1024);
  std::vector<uint32_t> w(words);
  AV_HIP(hipMemcpyAsync(w.data(), e->byz, words * 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < words && e->ref_node < 0; ++i)
    if (~w[i]) {
      const int64_t n = (int64_t)i * 32 + __builtin_ctz(~w[i]);
      if (n < e->N) e->ref_node = n;
    }
  return AV_OK;
}

// Sweep grid (0 = one wave per tile). Each wave walks `tiles_per_wave`
// tiles (grid stride, no next-tile prefetch): the wave's prologue — kernel
// parameters, the loop-invariant Philox key schedule and the SGPR spills the
// compiler parks in VGPR lanes, ~150 SALU and ~100 VALU instructions — is then
// paid once per 4 tiles instead of per tile. Measured on MI355X
// (tools/round_probe.py, C4 epoch): one wave per tile 9.37 ms, 4 tiles per
// wave 8.37 ms, 17 per wave 8.39 ms; the prefetching resident grid
// (kModeWarmPipe, 5 waves per SIMD) 9.5-10.2 ms. force: the resident grid (A/B).
uint32_t default_sweep_blocks(const av_engine* e, bool force) {
  if (e->k > 8 || e->capped) return 0;
  const uint64_t tiles = e->Lpad / 64;
  if (force) {
    int bpc = 0, cus = 0;
    if (avk::round_sweep_occupancy(e->k, false, &bpc, &cus) != hipSuccess || bpc <= 0 || cus <= 0) return 0;
    return (uint32_t)(bpc * cus);
  }
  // (by size: a run's nodes must fit the shared draw, 2 producer lanes each: 8 tiles need BL >= 16)
  // (a run's nodes must fit the run's peer draw: 2 producer lanes per node and round, 64 lanes; runs
  // of 16 tiles at BL >= 32 draw both rounds in two passes: C4 epoch 5.14 -> 4.95 ms, the settled
  // rounds 0.112 -> 0.088 ms, storm rounds +2 %, profiles/r03/ab_tiles_per_wave.log)
  // Default: the longest run (16, 8 or 4 tiles) whose nodes fit one 64-lane draw (tiles_per_wave <= BL:
  // 64 * tpw / BL nodes per run) while the grid keeps >= 15000 waves. Target shards of C4
  // (tools/shard_model.py, profiles/r04/tshard_c4_*.json, rank 0's settled rounds): BL 16 (G = 2)
  // 0.083 ms at 4 tiles per wave, 0.038 at 16; BL 8 (G = 4) 0.046 at 4, 0.031 at 8, 0.166 at 16 (the
  // run's nodes overflow the draw); BL 4 (G = 8) 0.027 at 4, 0.124 at 8.
  // Narrow rows (BL <= 8: C5, the target shards of C4 at 4 and 8 ranks): a run's nodes overflow the
  // draw at any length >= BL / 2, so every tile draws its own peers whatever the run, and the longest
  // run pays the per-wave set-up least; the uniform settled runs take up to 256 nodes (settled_run_uni).
  // Round 5 (tools/group_model.py, profiles/r05/s11/gm_td16_*.log; tools/round_probe.py, ab_c5td.log):
  // C4 rank 0 at G = 8 window 1.545 -> 1.309 ms, G = 4 2.078 -> 1.955, C5 epoch 17.2 -> 16.2 ms, C4p /
  // C4pb within 1 %.
  uint64_t tpw = e->tiles_per_wave;
  if (!tpw && e->BL <= 8) tpw = 16;
  if (!tpw) {
    tpw = 16;
    while (tpw > 4 && (tpw > (uint64_t)e->BL || tiles / tpw < 15000)) tpw /= 2;
  }
  const uint64_t waves = (tiles + tpw - 1) / tpw;
  return (uint32_t)std::max<uint64_t>(1, (waves + 3) / 4);
}

// Waves that write the StatusUpdate log in the fewest-wave round kernel the engine may launch: every
// writer picks shard wave % log_shards, so with more shards than writers the rest would sit empty and
// the usable capacity shrink by that factor. Capped engines: k_round_node (one wave per node per 64
// blocks); uncapped: the sweep grid's waves that own a run of tiles (round_plan.h sweep_grid, shared
// with launch_sweep_k), never more than the tiles (the first-generation kernels: one per tile).
uint64_t log_writer_waves(const av_engine* e) {
  if (e->capped) return (uint64_t)e->NL * ((e->BL + 63) / 64);
  return avk::sweep_run_waves(e->Lpad / 64, e->sweep_blocks);
}

// Shard count and per-shard capacities of the (empty) log from the allocation and the writers: a
// power of two with >= 4 writers per shard in every kernel, so that the modulo's uneven wrap (W
// writers over S shards: some get ceil(W / S)) loads no shard more than 1.25x the mean.
uint64_t log_shards_for(uint64_t w) {
  uint64_t sh = 1;
  while (sh * 2 <= avk::kLogShards && sh * 2 * 4 <= w) sh *= 2;
  return sh;
}

void set_log_layout(av_engine* e) {
  e->log_shards = (uint32_t)log_shards_for(log_writer_waves(e));
  e->log_cap = (uint32_t)std::min<size_t>(e->log_alloc / e->log_shards, 0xFFFFFFFFu);
  e->mlog_cap = (uint32_t)std::min<size_t>(e->mlog_alloc / e->log_shards, 0xFFFFFFFFu);
  e->dlog_cap = (uint32_t)std::min<size_t>(e->dlog_alloc / e->log_shards, 0xFFFFFFFFu);
}

int refresh_pref(av_engine* e) {
  e->facts.snapshot_written();
  AV_HIP(avk::launch_refresh_pref((uint32_t)e->pub_mode, e->planes, e->pref[e->cur], e->byz, (uint32_t)e->n0, e->NL,
                                  e->BL, e->PS, (uint32_t)e->round, e->stream));
  return AV_OK;
}

}  // namespace aveng

namespace {

avk::PlanShape plan_shape(const av_engine* e) {
  return {e->k,      e->BL,         e->N,               e->NL,       e->PS,
          e->capped, e->peer_world, e->comm != nullptr, e->pub_mode, e->any_nopoll,
          e->lossy(), e->loss_neutral, e->listed};
}
avk::PlanKnobs plan_knobs(const av_engine* e) {
  return {e->kernel,   e->virtual_votes, e->vv_min_bl,     e->count_lazy,     e->k_hi_virtual,
          e->ref_rows, e->uni_rows,      e->ablate_gather, e->unsynced_shard, e->quiet_tiles != 0,
          e->net_quiet != 0, e->count_changed, e->calm_tiles != 0};
}
avk::RoundPlan plan_for(const av_engine* e, bool replay) {
  return avk::plan_round(e->facts, plan_shape(e), plan_knobs(e), replay);
}

int round_checks(const av_engine* e, int64_t rounds) {
  AV_CHECK(e->round + rounds - 1 - e->log_base < e->max_log_rounds(), AV_ERR_OVERFLOW,
           "StatusUpdate log spans %lld rounds: call av_fetch_updates more often", (long long)e->max_log_rounds());
  if (e->group) {
    // serial group: round r of rank i is enqueued after round r of every lower rank and before
    // round r of every higher one (the stream order is the exchange's barrier)
    AV_TRY(group_alive(e));
    for (const av_engine* m : e->group->members)
      if (m != e)
        AV_CHECK(m->round == e->round + (m->peer_rank < e->peer_rank ? 1 : 0), AV_ERR_UNSUPPORTED,
                 "peer group: rank %d at round %lld, rank %d at round %lld: run one round of every rank in rank "
                 "order", e->peer_rank, (long long)e->round, m->peer_rank, (long long)m->round);
  }
  AV_CHECK(e->NL == (uint32_t)e->N || e->comm != nullptr || e->peer_world > 1 || e->N == e->n1 - e->n0 ||
               e->unsynced_shard,
           AV_ERR_UNSUPPORTED,
           "node-sharded engine needs av_comm_init before running rounds");
  return AV_OK;
}

bool all_targets_valid(const av_engine* e) {
  for (uint32_t b = 0; b < e->BL; ++b)
    if (e->valid_host[b] != avk::real_mask((uint32_t)(e->t1 - e->t0), b)) return false;
  return true;
}

// peer-push exchange: the sweep kernel's sim rounds push changed words into buffer nb's replicas; any
// other round is followed by a full push of this rank's rows (uniform across
// ranks: it depends only on the engine configuration and the call)
void fill_push_params(const av_engine* e, bool sweep_sim, int nb, avk::RoundParams& p) {
  if (e->peer_world > 1 && sweep_sim) {
    p.push_n = (uint32_t)e->peer_world - 1u;
    p.push_dst = e->push_tbl + (size_t)nb * avk::kMaxPeers;
    if (e->masked) {  // need-masked pushes: this round's row masks (window of push round e->round)
      const int64_t w = e->round / avk::kNeedWin;  // combined before the launch (need_combine) if not yet
      const bool have = e->need_ready == w || e->need_pushed == w;
      p.need = have ? e->needmask + (size_t)(e->round % avk::kNeedWin) * e->NL : nullptr;
      p.stale = e->stale + (size_t)nb * e->NL * e->segs;
      p.segs = e->segs;
    }
    p.peer_all = (1u << std::min<uint32_t>(p.push_n, 31u)) - 1u;
    p.push_defer = e->push_defer ? 1u : 0u;
    p.push_store = e->push_store;
  }
  p.count_changed = (p.push_n || e->count_changed) && sweep_sim ? 1u : 0u;
  p.changed = e->changed;
}

// Reference rows and uniform rows where the plan allows them and an honest reference node exists
// (the plan's two flags are cleared where none does).
int fill_row_params(av_engine* e, avk::RoundPlan& plan, int nb, avk::RoundParams& p) {
  if (plan.ref_rows || plan.uni_rows) {
    AV_TRY(ref_pick(e));
    plan.ref_rows = plan.ref_rows && e->ref_node >= 0;
    plan.uni_rows = plan.uni_rows && e->ref_node >= 0;
  }
  if (plan.ref_rows && e->round - e->rflag_clear_round >= 120) {
    // flag bytes carry a 7-bit snapshot tag (sweep_publish.h ref_tag): every buffer's flags are
    // cleared before 128 rounds have passed since the last clear, whatever kind of round ran in
    // between (replay, capped, non-refr), so no byte outlives its tag's period
    for (int b = 0; b < 3; ++b)
      AV_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(e->pref[b].get()) + e->rflag_off, 0, (size_t)e->N, e->stream));
    e->rflag_clear_round = e->round;
    e->facts.snapshot_written();
  }
  if (plan.ref_rows) {
    p.ref_node = (uint32_t)e->ref_node;
    p.ps_shift = (uint32_t)__builtin_ctz(e->PS * 4u);
    p.rflag_off = (uint32_t)e->rflag_off;
    p.rflag_out = reinterpret_cast<uint8_t*>(e->pref[nb].get()) + e->rflag_off;
    p.rflag_in =
        e->facts.rflag_ok[e->cur] ? reinterpret_cast<const uint8_t*>(e->pref[e->cur].get()) + e->rflag_off : nullptr;
  }
  // uniform rows: sweep rounds at k = 8 tag the snapshot they write; a round whose input snapshot
  // is known uniform tests settled tiles with no peer draw and no gather (kernels.h uni_*)
  if (plan.uni_rows) {
    p.ref_node = (uint32_t)e->ref_node;
    p.uni_off = (uint32_t)e->uni_off;
    p.uni_world = (uint32_t)std::max(1, e->peer_world);
    p.uni_rank = (uint32_t)std::max(0, e->peer_rank);
    p.uni_out = e->pref[nb] + e->uni_off;
    p.uni_in = e->facts.uni_ok[e->cur] ? e->pref[e->cur] + e->uni_off : nullptr;
    const int pv = av_engine::prv(e->cur);
    p.uni_prev = e->facts.uni_ok[pv] ? e->pref[pv] + e->uni_off : nullptr;
    p.uni_merge = e->uni_merge;
    p.uni_post = p.push_n ? 1u : 0u;  // the slot reaches the peers in the barrier kernel
  }
  return AV_OK;
}

// The pair of events around one timed launch (av_set_timing; av_kernel_stats sums them).
int timing_begin(av_engine* e, hipEvent_t* ev0, hipEvent_t* ev1) {
  if (!e->timing) return AV_OK;
  AV_HIP(hipEventCreate(ev0));
  AV_HIP(hipEventCreate(ev1));
  AV_HIP(hipEventRecord(*ev0, e->stream));
  return AV_OK;
}

int timing_end(av_engine* e, hipEvent_t ev0, hipEvent_t ev1) {
  AV_HIP(hipEventRecord(ev1, e->stream));
  e->events.emplace_back(avmem::Event(ev0), avmem::Event(ev1));  // owned from here on
  return AV_OK;
}

// What follows a round's kernel: the next window's need masks (inside the round's timing), then this
// rank's rows of buffer nb to the peers where the kernel did not push them, the barrier, the RCCL
// all-gather.
int exchange_tail(av_engine* e, const avk::RoundParams& p, int nb, hipEvent_t ev0, hipEvent_t ev1) {
  const bool peer = e->peer_world > 1;
  if (peer) {
    // the next push round's window drawn and pushed before the barrier (combined after it)
    AV_TRY(need_gen(e, (e->round + 1) / avk::kNeedWin));
  }
  if (ev0) {
    AV_TRY(timing_end(e, ev0, ev1));
  } else if (e->round_marker) {  // diagnostics: a timing-free event after every round
    if (!e->marker) AV_HIP(e->marker.create(hipEventDisableTiming));
    AV_HIP(hipEventRecord(e->marker, e->stream));
  }
  if (peer) {
    if (!p.push_n) {
      AV_TRY(push_own_rows(e, nb));
      AV_TRY(stale_clear(e, nb));
    }
    AV_TRY(peer_barrier(e, p.uni_post ? nb : -1));
  } else if (e->solo_barrier) {
    AV_TRY(peer_barrier(e));
  }
  if (e->comm) {
    const size_t count = (size_t)e->NL * e->PS;
    uint32_t* out = e->pref[nb];
    ncclResult_t r = ncclAllGather(out + (size_t)e->n0 * e->PS, out, count, ncclUint32, e->comm, e->stream);
    AV_CHECK(r == ncclSuccess, AV_ERR_RCCL, "ncclAllGather: %s", ncclGetErrorString(r));
  }
  return AV_OK;
}

// Why no kernel runs a lossy (R5) or listed (R6) sim round of this engine; `what` names the rule.
int refuse_round(const av_engine* e, const char* what) {
  AV_CHECK(!e->capped, AV_ERR_UNSUPPORTED, "%s need M <= 4096 (uncapped)", what);
  AV_CHECK(e->pub_mode != 2, AV_ERR_UNSUPPORTED, "%s: not with the example responder (responder 2)", what);
  AV_CHECK(e->peer_world <= 1, AV_ERR_UNSUPPORTED, "%s: not on a peer-push engine", what);
  return AV_OK;
}

int launch_one_round(av_engine* e, const uint32_t* replay) {
  AV_TRY(round_checks(e, 1));
  avk::RoundPlan plan = plan_for(e, replay != nullptr);
  // rules R6 and R5: no kernel runs these rounds, until the lists are cleared or the loss is off
  if (plan.unsupported && plan.listed) AV_TRY(refuse_round(e, "rounds over peer lists (av_set_peer_lists)"));
  if (plan.unsupported && plan.lossy)
    AV_TRY(refuse_round(e, "rounds with lost Responses or unresponsive nodes (av_set_loss, av_set_responding)"));
  AV_CHECK(!plan.unsupported, AV_ERR_UNSUPPORTED,
           "the example responder and av_set_polling need M <= 4096 (uncapped)");
  AV_TRY(materialize(e, plan.wb_votes || plan.wb_cpreset, false));  // (two passes, votes first)
  AV_TRY(materialize(e, false, plan.wb_counts));
  avk::RoundParams p = round_params(e, replay);
  p.c_preset = e->facts.c_preset ? 1u : 0u;  // (left only before a fresh sweep round: plan.wb_cpreset)
  p.vv = plan.vv ? 1u : 0u;
  p.vv_uniform = plan.vv_uniform ? 1u : 0u;
  p.fresh = plan.fresh ? 1u : 0u;
  p.klazy = plan.klazy ? 1u : 0u;
  p.calm = plan.calm ? 1u : 0u;
  p.kconsume = plan.kconsume ? 1u : 0u;
  p.hivirt = plan.hivirt ? 1u : 0u;
  const bool sweep = plan.kernel == avk::RoundKernel::Sweep;
  const int nb = av_engine::nxt(e->cur);
  fill_push_params(e, sweep && !replay, nb, p);
  AV_TRY(fill_row_params(e, plan, nb, p));
  if (plan.net_quiet_out) {  // the network-quiet word: this round's, and the last round's if it holds
    p.nq_out = e->nq + (e->round & 1);
    p.nq_in = plan.net_quiet_in ? e->nq + ((e->round & 1) ^ 1) : nullptr;
    p.nq_rounds = e->nq + 2;
    p.nq_group = e->nq_group;
    p.nq_front = e->nq_front;
  }
  if (e->warm_pref && sweep) {  // diagnostics (untimed): the round's gather sources, read once
    if (!e->touch_sink) AV_HIP(e->touch_sink.alloc(16));
    AV_HIP(avk::launch_touch(p.pref_prev, (size_t)e->N * e->PS * 4u, e->touch_sink, e->stream));
    AV_HIP(avk::launch_touch(p.pref_in, (size_t)e->N * e->PS * 4u, e->touch_sink, e->stream));
  }
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  AV_TRY(timing_begin(e, &ev0, &ev1));
  if (p.push_n && e->masked) {  // (inside the round's timing: the exchange's own work)
    AV_TRY(need_combine(e, e->round / avk::kNeedWin));
    AV_TRY(need_draw_ahead(e, e->round / avk::kNeedWin + 1));
  }
  bool refw = false;  // the round wrote reference-row flags for the snapshot it published
  switch (plan.kernel) {
    case avk::RoundKernel::Sweep:
      AV_HIP(avk::launch_round_sweep(p, e->k, plan.mode, e->sweep_blocks, e->stream, &refw));
      break;
    case avk::RoundKernel::Node:
      p.node_flags = e->node_flags;
      AV_HIP(avk::launch_round_node(p, e->k, plan.replay, plan.exact_pass, e->stream));
      break;
    case avk::RoundKernel::FirstGen:
      AV_HIP(avk::launch_round(p, e->k, plan.replay, e->capped, e->stream));
      break;
    case avk::RoundKernel::Lossy: {
      avk::LossyParams lp{};
      lp.r = p;
      lp.responding = e->any_down ? e->responding.get() : nullptr;
      lp.lost = e->lost;
      lp.loss_threshold = e->loss_threshold;
      AV_HIP(avk::launch_round_lossy(lp, e->k, plan.loss_neutral, e->stream));
      break;
    }
    case avk::RoundKernel::Listed: {
      avk::ListedParams q{};
      q.l.r = p;
      q.l.responding = e->any_down ? e->responding.get() : nullptr;
      q.l.lost = e->lost;
      q.l.loss_threshold = e->loss_threshold;
      q.offsets = e->list_offsets;
      q.list = e->list_peers;
      q.unsent = e->unsent;
      AV_HIP(avk::launch_round_listed(q, e->k, plan.loss_neutral, e->stream));
      break;
    }
  }
  if (e->pub_mode == 2) {  // the responders' re-adds (main.go:175-177)
    AV_HIP(avk::launch_readd(p, e->stream));
    e->facts.responder_readds();
  }
  e->facts.after_round(plan, all_targets_valid(e), refw, nb);
  AV_TRY(exchange_tail(e, p, nb, ev0, ev1));
  e->cur = nb;
  e->round++;
  return AV_OK;
}

// Replay rounds [round, round + R) of a capped engine in one k_replay_node
// launch, followed per round by the exact pass over the nodes it left at that
// round (count >= 120). Host-side round bookkeeping as launch_one_round.
int launch_replay_fused(av_engine* e, const uint32_t* replay0, int32_t R) {
  e->facts.snapshot_written();
  AV_TRY(round_checks(e, R));
  AV_TRY(materialize(e, true, false));
  AV_TRY(materialize(e, false, true));
  const size_t per = e->round_replay_words();
  avk::RoundParams p = round_params(e, replay0);
  p.node_flags = e->node_flags;
  p.fuse_rounds = (uint32_t)R;
  p.replay_fast = e->replay_fast && e->BL >= avk::kMaxPoll / 32 ? 1u : 0u;
  p.replay_stride = per;
  p.ring_next = (uint32_t)av_engine::nxt(e->cur);
  for (int i = 0; i < 3; ++i) p.pref_ring[i] = e->pref[i];
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  AV_TRY(timing_begin(e, &ev0, &ev1));
  AV_HIP(avk::launch_replay_node(p, e->k, e->stream));
  for (int32_t r = 0; r < R; ++r) {
    const avk::RoundPlan plan = plan_for(e, true);
    if (plan.exact_pass) {  // a node may have reached count 120 by this round
      avk::RoundParams q = round_params(e, replay0 + per * (size_t)r);
      q.node_flags = e->node_flags;
      q.exact_rel = (uint32_t)r;
      q.exact_keep = r + 1 < R ? 1u : 0u;
      AV_HIP(avk::launch_round(q, e->k, /*replay=*/true, /*capped=*/true, e->stream));
    }
    e->cur = av_engine::nxt(e->cur);
    e->facts.after_round(plan, /*all_valid: not read after a replay round*/ false, false, e->cur);
    e->round++;
  }
  if (ev0) return timing_end(e, ev0, ev1);
  return AV_OK;
}


// A step of av_create: AV_ERR_OOM where the device has no memory left, else AV_ERR_HIP.
int created(hipError_t he, const char* what) {
  AV_CHECK(he == hipSuccess, oom_or_hip(he), "%s: %s", what, hipGetErrorString(he));
  return AV_OK;
}

}  // namespace

extern "C" {

int av_abi_version(void) { return AVHIP_ABI_VERSION; }

void av_config_init(av_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->k = 8;
  c->seed = 0xA7A1A9C4ull;
}

const char* av_strerror(int code) {
  switch (code) {
    case AV_OK: return "ok";
    case AV_ERR_INVALID_ARG: return "invalid argument";
    case AV_ERR_HIP: return "HIP runtime error";
    case AV_ERR_OOM: return "out of device memory";
    case AV_ERR_NOT_FOUND: return "VoteRecord not found";
    case AV_ERR_OVERFLOW: return "buffer overflow";
    case AV_ERR_UNSUPPORTED: return "unsupported configuration";
    case AV_ERR_RCCL: return "RCCL error";
    case AV_ERR_PEER: return "peer exchange failed";
    default: return "unknown error";
  }
}

const char* av_last_error(void) { return g_last_error.c_str(); }

// Only what has an order is written out; everything else the engine owns is released by its members'
// destructors (engine.h), the buffers and events before the engine's stream.
int av_destroy(av_engine* e) {
  if (!e) return AV_OK;
  std::unique_ptr<av_engine> rest(e);
  if (!e->stream) return AV_OK;  // av_create stopped before its first device call
  (void)hipSetDevice(e->cfg.device);
  (void)hipStreamSynchronize(e->stream);
  if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
  if (e->need_stream) (void)hipStreamSynchronize(e->need_stream);
  if (e->comm) (void)ncclCommDestroy(e->comm);
  for (void* m : e->peer_opened) (void)hipIpcCloseMemHandle(m);
  if (PeerGroup* g = e->group) {  // the group's stream is destroyed with its last member
    g->members[(size_t)e->peer_rank] = nullptr;
    if (--g->alive == 0) delete g;
  }
  return AV_OK;
}

int av_create(const av_config* cfg, av_engine** out) {
  AV_CHECK(cfg && out, AV_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const av_config& c = *cfg;
  // node ids are 32-bit in the kernels; the update word's node field widens past 24 bits by taking
  // bits from its round field (pack_update), which keeps >= 2^6 rounds between fetches below 2^30
  AV_CHECK(c.n_nodes >= 2 && c.n_nodes < (1ll << 30), AV_ERR_INVALID_ARG, "n_nodes must be in [2, 2^30)");
  AV_CHECK(c.n_targets >= 1 && c.n_targets < (1ll << 22), AV_ERR_INVALID_ARG, "n_targets must be in [1, 2^22)");
  AV_CHECK(c.k >= 1 && c.k <= avk::kMaxK, AV_ERR_INVALID_ARG, "k must be in [1, 16]");
  AV_CHECK(c.peer_mode == AV_PEERS_RANDOM || c.peer_mode == AV_PEERS_ROUND_ROBIN, AV_ERR_INVALID_ARG,
           "bad peer_mode");
  // destroyed on every return but the last (av_destroy: before the stream exists, a plain delete)
  std::unique_ptr<av_engine, int (*)(av_engine*)> guard(new av_engine(), av_destroy);
  av_engine* e = guard.get();
  e->cfg = c;
  e->N = c.n_nodes;
  e->M = c.n_targets;
  e->n0 = c.node_begin;
  e->n1 = c.node_end;
  if (e->n0 == 0 && e->n1 == 0) e->n1 = e->N;
  e->t0 = c.target_begin;
  e->t1 = c.target_end;
  if (e->t0 == 0 && e->t1 == 0) e->t1 = e->M;
  e->k = c.k;
  {
    uint32_t nb = 24;
    while (nb < 32 && (1ll << nb) < e->N) ++nb;
    e->round_shift = 28 + nb;
  }
  AV_CHECK(e->n0 >= 0 && e->n0 < e->n1 && e->n1 <= e->N, AV_ERR_INVALID_ARG, "bad node shard");
  AV_CHECK(e->t0 >= 0 && e->t0 < e->t1 && e->t1 <= e->M && e->t0 % 32 == 0, AV_ERR_INVALID_ARG, "bad target shard");
  e->capped = e->M > (int64_t)avk::kMaxPoll;
  AV_CHECK(!e->capped || (e->t0 == 0 && e->t1 == e->M), AV_ERR_UNSUPPORTED,
           "target sharding needs M <= 4096: the 4096 poll cap couples targets (processor.go:165-167)");
  e->NL = (uint32_t)(e->n1 - e->n0);
  e->BL = (uint32_t)((e->t1 - e->t0 + 31) / 32);
  e->PS = avk::pref_stride(e->BL);
  AV_CHECK(!e->capped || e->BL <= 1024, AV_ERR_INVALID_ARG, "capped path supports M <= 32768");
  const uint64_t L = (uint64_t)e->NL * e->BL;
  AV_CHECK(L < (1ull << 31), AV_ERR_INVALID_ARG, "too many lanes for one engine: shard further");
  // the round kernels index the published-preference table (all N nodes x PS words) in 32 bits
  AV_CHECK((uint64_t)e->N * e->PS < (1ull << 31), AV_ERR_INVALID_ARG,
           "preference table over 2^31 words: shard targets further");
  e->L = (uint32_t)L;
  e->Lpad = (uint32_t)((L + 63) / 64 * 64);
  avk::bl_divider(e->BL, e->bl_magic, e->bl_sh1, e->bl_sh2);

  AV_TRY(created(hipSetDevice(c.device), "hipSetDevice"));
  AV_TRY(created(e->own_stream.create(hipStreamNonBlocking), "hipStreamCreate"));
  e->stream = e->own_stream;
  hipStream_t s = e->stream;
  const size_t plane_words = (size_t)(e->Lpad / 64) * avk::kPlanes * 64;
  const size_t pref_words = (size_t)e->N * e->PS;
  int64_t cap = c.update_log_capacity;
  if (cap <= 0) cap = std::min<int64_t>(std::max<int64_t>((int64_t)L * 8, 1 << 20), 1ll << 28);
  // one shard per wave up to kLogShards: waves of the round kernel that runs
  const uint64_t waves = e->capped ? (uint64_t)e->NL * ((e->BL + 63) / 64) : (uint64_t)(e->Lpad / 64);
  e->log_shards = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(waves, avk::kLogShards));
  e->log_cap = (uint32_t)std::max<int64_t>((cap + e->log_shards - 1) / e->log_shards, 64);
  AV_TRY(created(e->planes.alloc(plane_words), "alloc planes"));
  // whole 2-MiB units: each snapshot buffer is an allocation of its own (IPC export, av_peer_handles)
  e->rflag_off = (pref_words * 4 + 255) / 256 * 256;
  e->uni_off = (e->rflag_off + (size_t)e->N + 255) / 256 * 256 / 4;  // uniform-rows slots (kernels.h)
  e->pref_alloc_words =
      ((e->uni_off * 4 + (avk::kMaxPeers + 1) * 4 + (2u << 20) - 1) / (2u << 20)) * (2u << 20) / 4;
  for (auto& pref : e->pref) AV_TRY(created(pref.alloc_zeroed(e->pref_alloc_words, s), "alloc pref"));
  AV_TRY(created(e->vstale.alloc_zeroed(e->Lpad / 64, s), "alloc planes"));
  AV_TRY(created(e->kpend.alloc_zeroed(e->Lpad / 64, s), "alloc planes"));
  AV_TRY(created(e->valid.alloc(e->BL), "alloc valid"));
  AV_TRY(created(e->byz.alloc((e->N + 31) / 32), "alloc byz"));
  AV_TRY(created(e->log.alloc((size_t)e->log_cap * e->log_shards), "alloc log"));
  AV_TRY(created(e->log_count.alloc_zeroed(3 * avk::kLogShards * avk::kCtrStride, s), "alloc log"));
  e->mlog_count = e->log_count + avk::kLogShards * avk::kCtrStride;
  e->dlog_count = e->log_count + 2 * avk::kLogShards * avk::kCtrStride;
  // a dense record holds >= dense_min(k) updates: log_cap / dense_min records
  // take any log_cap updates that go dense (8 B of capacity per update)
  const uint32_t dw = avk::dense_words((uint32_t)e->k);
  e->dense_min = avk::dense_min((uint32_t)e->k);
  // k = 8 (slot records, kernels.h): a lane goes dense from 4 slots with updates on
  const uint32_t dense_least = e->k == 8 ? 4u : e->dense_min;
  e->dlog_cap = std::max<uint32_t>(e->log_cap / dense_least, 16);
  AV_TRY(created(e->dlog.alloc((size_t)e->dlog_cap * e->log_shards * dw), "alloc log"));
  AV_TRY(created(e->upd_count.alloc_zeroed(avk::kLogShards, s), "alloc log"));
  // a medium record holds >= 2 updates: log_cap / 2 records per shard (kernels.h med_rec_words: 32 B
  // slot records, 16 B per update of capacity). Only k = 8 kernels emit them (round_common.h
  // emit_store_med: the sweep, k_replay_fast): other engines keep a token 16 records per shard.
  e->mlog_cap = e->k == 8 ? std::max<uint32_t>(e->log_cap / 2, 16) : 16u;
  AV_TRY(created(e->mlog.alloc((size_t)e->mlog_cap * e->log_shards * avk::med_rec_words()), "alloc log"));
  e->log_alloc = (size_t)e->log_cap * e->log_shards;
  e->mlog_alloc = (size_t)e->mlog_cap * e->log_shards;
  e->dlog_alloc = (size_t)e->dlog_cap * e->log_shards;
  AV_TRY(created(e->log_overflow.alloc_zeroed(1, s), "alloc log"));
  if (e->capped) AV_TRY(created(e->node_flags.alloc_zeroed(e->NL, s), "alloc node flags"));
  AV_TRY(created(e->applied.alloc_zeroed(avk::kLogShards, s), "alloc counters"));
  AV_TRY(created(e->bytes.alloc_zeroed(2 * avk::kLogShards, s), "alloc counters"));
  AV_TRY(created(e->finalized.alloc_zeroed(avk::kLogShards, s), "alloc counters"));
  AV_TRY(created(e->scratch_count.alloc(1), "alloc counters"));
  AV_TRY(created(e->changed.alloc_zeroed(3 * avk::kLogShards, s), "alloc counters"));
  AV_TRY(created(e->nq.alloc_zeroed(4, s), "alloc counters"));
  // every real target starts valid
  e->valid_host.assign(e->BL, 0u);
  for (uint32_t b = 0; b < e->BL; ++b) {
    const int64_t tb = e->t0 + 32ll * b;
    const int64_t r = std::min<int64_t>(e->t1 - tb, 32);
    e->valid_host[b] = r >= 32 ? ~0u : ((1u << r) - 1u);
  }
  AV_TRY(created(hipMemcpyAsync(e->valid, e->valid_host.data(), e->BL * 4, hipMemcpyHostToDevice, s), "upload valid"));
  AV_TRY(created(avk::launch_byz(e->byz, (uint32_t)e->N, c.seed, c.byz_threshold, s), "byz kernel"));
  e->sweep_blocks = default_sweep_blocks(e);
  set_log_layout(e);  // shards = the sweep grid's writers (a wave takes a run of tiles), not the tiles
  AV_TRY(av_init_records(e, AV_INIT_NONE, 0));
  *out = guard.release();
  return AV_OK;
}

int av_init_records(av_engine* e, int32_t init_mode, uint32_t init_param) {
  AV_ENTER(e);
  AV_CHECK(init_mode >= AV_INIT_NONE && init_mode <= AV_INIT_PAIRS, AV_ERR_INVALID_ARG, "bad init_mode");
  // every plane is rewritten: nothing deferred survives
  if (e->facts.v_stale) AV_HIP(hipMemsetAsync(e->vstale, 0, (size_t)(e->Lpad / 64) * 4, e->stream));
  if (e->facts.k_pend) AV_HIP(hipMemsetAsync(e->kpend, 0, (size_t)(e->Lpad / 64) * 4, e->stream));
  // the consider planes preset (kernels.h c_preset) where the new records' next sim round would plan
  // as a fresh sweep round, with this engine's shape and options as they stand
  const bool created = init_mode != AV_INIT_NONE;
  const bool preset = created && e->c_preset && avk::plans_c_preset(plan_shape(e), plan_knobs(e));
  e->facts.init(created, preset);
  avk::InitParams p{};
  p.c_preset = preset ? 1u : 0u;
  p.planes = e->planes;
  p.pref = e->pref[e->cur];
  p.byz = e->byz;
  p.seed = e->cfg.seed;
  p.n_nodes = (uint32_t)e->N;
  p.n0 = (uint32_t)e->n0;
  p.NL = e->NL;
  p.BL = e->BL;
  p.PS = e->PS;
  p.L = e->L;
  p.Lpad = e->Lpad;
  p.t0 = (uint32_t)e->t0;
  p.n_targets = (uint32_t)e->t1;  // targets >= t1 belong to another shard (or do not exist)
  p.round = (uint32_t)e->round;
  p.mode = init_mode;
  p.pub_mode = (uint32_t)e->pub_mode;
  p.param = init_param;
  AV_HIP(avk::launch_init(p, e->stream));
  if (e->peer_world > 1) {
    // peer-push engine: this rank's new rows of the current snapshot go to every peer replica, and
    // no rank's next round may read them before all ranks have pushed (collective: every rank
    // re-initialises). The other two buffers are untouched, so their replicas stay identical.
    AV_TRY(push_own_rows(e, e->cur));
    AV_TRY(stale_clear(e, e->cur));
    AV_TRY(need_gen(e, e->round / avk::kNeedWin));
    AV_TRY(peer_barrier(e));
  }
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_run_rounds(av_engine* e, int32_t rounds) {
  AV_ENTER(e);
  AV_PEER_CHECK(e);
  AV_CHECK(rounds >= 0, AV_ERR_INVALID_ARG, "rounds < 0");
  for (int32_t r = 0; r < rounds; ++r) {
    AV_TRY(launch_one_round(e, nullptr));
  }
  return AV_OK;
}

int av_replay_round_errs(av_engine* e, const uint32_t* errs) {
  AV_ENTER(e);
  AV_PEER_CHECK(e);
  AV_CHECK(errs, AV_ERR_INVALID_ARG, "null argument");
  e->facts.replay_call();
  const int64_t TL = e->t1 - e->t0;
  std::vector<uint32_t> planes(e->round_replay_words(), 0u);
  for (uint32_t nl = 0; nl < e->NL; ++nl)
    for (int s = 0; s < e->k; ++s) {
      const uint32_t* row = errs + ((size_t)nl * e->k + s) * TL;
      for (uint32_t b = 0; b < e->BL; ++b) {
        uint32_t y = 0, c = 0;
        for (uint32_t i = 0; i < 32; ++i) {
          const int64_t tl = 32ll * b + i;
          if (tl >= TL) break;
          const uint32_t err = row[tl];
          y |= (err == 0u ? 1u : 0u) << i;             // vote.go:55
          c |= ((int32_t)err >= 0 ? 1u : 0u) << i;     // vote.go:56
        }
        const size_t g = (size_t)nl * e->BL + b;
        planes[avk::replay_idx((uint32_t)g, e->k, s, 0)] = y;
        planes[avk::replay_idx((uint32_t)g, e->k, s, 1)] = c;
      }
    }
  avmem::DevBuf<uint32_t> s;
  AV_HIP(s.alloc(planes.size()));
  AV_HIP(hipMemcpyAsync(s, planes.data(), planes.size() * 4, hipMemcpyHostToDevice, e->stream));
  AV_TRY(launch_one_round(e, s));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_replay_prepare(av_engine* e, int32_t rounds) {
  AV_ENTER(e);
  AV_CHECK(rounds >= 1, AV_ERR_INVALID_ARG, "rounds < 1");
  const size_t per = e->round_replay_words();
  const hipError_t he = e->replay.reserve(per * rounds);
  AV_CHECK(he == hipSuccess, oom_or_hip(he), "alloc replay: %s", hipGetErrorString(he));
  for (int32_t r = 0; r < rounds; ++r)
    AV_HIP(avk::launch_gen_replay(e->cfg.seed, (uint32_t)e->n0, e->NL, e->BL, e->L, e->Lpad, (uint32_t)e->t0,
                                  (uint32_t)e->t1, (uint32_t)(e->round + r), e->k, e->replay + per * r, e->stream));
  e->replay_first = e->round;
  e->replay_ready = rounds;
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_replay_rounds(av_engine* e, int32_t rounds) {
  AV_ENTER(e);
  AV_PEER_CHECK(e);
  AV_CHECK(rounds >= 0, AV_ERR_INVALID_ARG, "rounds < 0");
  AV_CHECK(e->round >= e->replay_first && e->round + rounds <= e->replay_first + e->replay_ready,
           AV_ERR_INVALID_ARG, "replay stream not prepared for these rounds");
  if (rounds > 0) e->facts.replay_call();
  const size_t per = e->round_replay_words();
  // capped engines (poll cap binds) fuse consecutive replay rounds: every node's
  // records depend only on its own stream (k_replay_node)
  const bool fuse = e->replay_fuse > 1 && e->kernel == 2 && e->k <= 8 && e->capped && e->pub_mode == 0 &&
                    !e->any_nopoll && e->peer_world <= 1 && !e->comm && e->NL == (uint32_t)e->N;
  for (int32_t r = 0; r < rounds;) {
    const uint32_t* rp = e->replay + per * (size_t)(e->round - e->replay_first);
    const int32_t n = fuse ? std::min<int32_t>(rounds - r, e->replay_fuse) : 1;
    AV_TRY(n > 1 ? launch_replay_fused(e, rp, n) : launch_one_round(e, rp));
    r += n;
  }
  return AV_OK;
}

int av_synchronize(av_engine* e) {
  AV_ENTER(e);
  AV_HIP(hipStreamSynchronize(e->stream));
  AV_PEER_CHECK(e);
  return AV_OK;
}

int av_round_index(av_engine* e, int64_t* out) {
  AV_CHECK(e && out, AV_ERR_INVALID_ARG, "null argument");
  *out = e->round;
  return AV_OK;
}

int av_get_round(av_engine* e, int64_t node, int64_t* out) {
  AV_CHECK(e && out, AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(local_node(e, node), AV_ERR_INVALID_ARG, "node %lld not in this shard", (long long)node);
  *out = e->proc_round.empty() ? 0 : e->proc_round[(size_t)(node - e->n0)];
  return AV_OK;
}

int av_set_round(av_engine* e, int64_t node, int64_t round) {
  AV_CHECK(e, AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(local_node(e, node), AV_ERR_INVALID_ARG, "node %lld not in this shard", (long long)node);
  if (e->proc_round.empty()) e->proc_round.assign(e->NL, 0);
  e->proc_round[(size_t)(node - e->n0)] = round;
  return AV_OK;
}

int av_materialize(av_engine* e) {
  AV_ENTER(e);
  AV_PEER_CHECK(e);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (e->facts.v_stale || e->facts.k_pend || e->facts.c_preset) AV_TRY(timing_begin(e, &ev0, &ev1));
  AV_TRY(materialize_votes(e));
  return ev0 ? timing_end(e, ev0, ev1) : AV_OK;
}

}  // extern "C"

namespace {

// ---- av_set_option (documented in include/avhip.h) ----
// Plain options only store a value: a bool (value != 0), or an integer in [lo, hi] that is rejected
// (AV_ERR_INVALID_ARG) or clamped outside it.
enum OptKind { kBool, kReject, kClamp };
struct PlainOption {
  const char* name;
  OptKind kind;
  int64_t lo, hi;
  bool av_engine::*b;  // the member: one of the three
  uint32_t av_engine::*u;
  int av_engine::*i;
};
constexpr PlainOption opt(const char* n, bool av_engine::*m) { return {n, kBool, 0, 1, m, nullptr, nullptr}; }
constexpr PlainOption opt(const char* n, uint32_t av_engine::*m, OptKind kd = kBool, int64_t lo = 0, int64_t hi = 1) {
  return {n, kd, lo, hi, nullptr, m, nullptr};
}
constexpr PlainOption opt(const char* n, int av_engine::*m, OptKind kd, int64_t lo, int64_t hi) {
  return {n, kd, lo, hi, nullptr, nullptr, m};
}

constexpr PlainOption kPlainOptions[] = {
    opt("plane_nt", &av_engine::plane_nt),              // non-temporal plane loads / stores
    opt("uniform_rows", &av_engine::uni_rows),          // A/B: uniform-row settled tests (kernels.h uni_*)
    opt("ref_rows", &av_engine::ref_rows),              // reference-row flags in converged sweep rounds (kernels.h)
    opt("virtual_votes", &av_engine::virtual_votes),    // 0: always store the vote planes (A/B)
    opt("vv_min_bl", &av_engine::vv_min_bl, kReject, 1, (1ll << 31) - 1),  // smallest BL with stale votes
    opt("kernel", &av_engine::kernel, kReject, 1, 2),  // 2 = k_round_sweep / k_round_node, 1 = k_round_fast
    opt("store_policy", &av_engine::store_policy, kReject, 0, 3),  // 2 = sc1 plane stores, 3 = nt sc1
    opt("settled_fast", &av_engine::settled_fast),      // settled warm tiles skip the round step's bookkeeping
    opt("settled_lean", &av_engine::settled_lean),      // a run's settled candidates tested in one lean loop
    opt("wave_runs", &av_engine::wave_runs),            // a wave takes a run of tiles and draws their peers once
    opt("sweep_nopipe", &av_engine::sweep_nopipe),      // 0 = the prefetching kModeWarmPipe on a resident grid (A/B)
    opt("uni_merge", &av_engine::uni_merge, kReject, 1, 16),  // runs per wave, uniform-input rounds
    opt("uni_votes", &av_engine::uni_votes),            // uniform input: the reference word as every tile's votes
    opt("quiet_tiles", &av_engine::quiet_tiles),        // A/B: quiescent settled tiles skip the A read and the republish
    opt("calm_tiles", &av_engine::calm_tiles),          // A/B: 0 = stale tiles with one stray old vote regather (kernels.h calm)
    opt("net_quiet", &av_engine::net_quiet),            // A/B: rounds after a fully quiescent round skip the per-run work
    opt("net_quiet_group", &av_engine::nq_group, kReject, 1, 16),  // runs per leader wave of such a round
    opt("net_quiet_front", &av_engine::nq_front),       // A/B: 0 = every net_quiet_group-th wave leads, not the grid's first
    opt("wave_dense", &av_engine::wave_dense, kReject, 0, 64),  // A/B: dense records per wave (0 off)
    opt("tile_draw", &av_engine::tile_draw, kReject, 0, 1),  // A/B: per-tile shared draws in overflowing runs
    opt("materialize_run", &av_engine::mat_run, kReject, 1, 64),  // A/B: tiles per wave of the write-back
    opt("c_preset", &av_engine::c_preset),              // A/B: 0 = av_init_records stores C = ~live (kCAll stays in use)
    opt("replay_fuse", &av_engine::replay_fuse, kReject, 0, 4096),  // replay rounds per launch (<= 1: off)
    opt("replay_fast", &av_engine::replay_fast),        // k_replay_fast where the poll set is the first 128 lanes
    opt("dropin_fast", &av_engine::dropin_fast),        // 0: drop-in batches always take the sort-grouped path
    opt("admit_map", &av_engine::admit_map, kReject, 0, 2),  // A/B: av_admit_targets' thread mapping (0 = by the touched blocks)
    opt("push_defer", &av_engine::push_defer),          // A/B: 0 = every push stored from the tile loop
    opt("push_store", &av_engine::push_store, kReject, 0, 2),  // A/B: 0 = system scope, 2 = none (invalid)
    opt("census_blocks", &av_engine::census_blocks, kReject, 0, 65536),  // av_census grid (0 = by size)
    opt("catalog_blocks", &av_engine::catalog_blocks, kReject, 0, 65535),  // hash lookup grid (0 = by size)
    opt("catalog_lds", &av_engine::catalog_lds),        // A/B: 0 = the hash table probed in global memory at any size
    opt("copy_blocks", &av_engine::copy_blocks, kReject, 0, 4096),  // stream copy kernel (0 = runtime copy)
    opt("enc_buckets", &av_engine::enc_buckets, kReject, 1, 1ll << 30),  // buckets per encoder pass
    opt("count_changed", &av_engine::count_changed),    // diagnostics: count changed published words in every sweep round
    opt("round_marker", &av_engine::round_marker),      // diagnostics: a timing-free event after every round
    opt("warm_pref", &av_engine::warm_pref),            // diagnostics: the gather sources read once before a timed round
    opt("unsynced_shard", &av_engine::unsynced_shard),  // diagnostics (invalid results): rounds with no exchange
    opt("ablate_gather", &av_engine::ablate_gather),    // diagnostics (invalid results)
    opt("ablate_phase", &av_engine::ablate_phase, kClamp, 0, 31),  // diagnostics (kernels.h; invalid results)
    opt("ablate_emit", &av_engine::ablate_emit, kClamp, 0, 3),     // diagnostics (invalid results)
    opt("ablate_node", &av_engine::ablate_node, kClamp, 0, 7),     // diagnostics (k_round_node)
};

int opt_range(const char* name, int64_t value, int64_t lo, int64_t hi) {
  AV_CHECK(value >= lo && value <= hi, AV_ERR_INVALID_ARG, "%s must be in [%lld, %lld]", name, (long long)lo,
           (long long)hi);
  return AV_OK;
}

int set_plain(av_engine* e, const PlainOption& o, int64_t value) {
  if (o.kind == kReject) AV_TRY(opt_range(o.name, value, o.lo, o.hi));
  value = o.kind == kBool ? value != 0 : std::max(o.lo, std::min(o.hi, value));
  if (o.b)
    e->*o.b = value != 0;
  else if (o.u)
    e->*o.u = (uint32_t)value;
  else
    e->*o.i = (int)value;
  return AV_OK;
}

// Options with side effects. Every handler that touches the device enters through AV_ENTER.
// 0 = one wave per tile, -1 = the default choice, -2 = resident grid
int opt_sweep_blocks(av_engine* e, int64_t value) {
  AV_TRY(opt_range("sweep_blocks", value, -2, (1ll << 31) - 1));
  AV_ENTER(e);
  e->sweep_blocks = value < 0 ? default_sweep_blocks(e, value == -2) : (uint32_t)value;
  e->sweep_blocks_explicit = value >= 0;
  return relayout_log_if_empty(e);
}

int opt_tiles_per_wave(av_engine* e, int64_t value) {
  AV_TRY(opt_range("tiles_per_wave", value, 0, 4096));
  AV_ENTER(e);
  e->tiles_per_wave = (uint32_t)value;
  // the default grid depends on the run length; an explicit sweep_blocks stays as set
  if (!e->sweep_blocks_explicit) e->sweep_blocks = default_sweep_blocks(e);
  return relayout_log_if_empty(e);
}

// diagnostics: a one-rank barrier after every round (exchange_cost.py)
int opt_solo_barrier(av_engine* e, int64_t value) {
  AV_CHECK(e->peer_world <= 1 && !e->comm, AV_ERR_UNSUPPORTED, "solo_barrier: engine has an exchange");
  if (value && !e->arrive) {
    AV_ENTER(e);
    AV_TRY(alloc_arrival(e));
    e->peer_arrive.p[0] = e->arrive;
  }
  e->solo_barrier = value != 0;
  e->solo_used = e->solo_used || e->solo_barrier;
  return AV_OK;
}

// "count_lazy" (0: always store the count planes) and "k_hi_virtual" (the virtual K4..K7 group, kernels.h
// kHiVirt), A/B: what is deferred under the old setting is written back
template <bool av_engine::*M>
int opt_count_planes(av_engine* e, int64_t value) {
  AV_ENTER(e);
  AV_TRY(materialize(e, false, true));
  e->*M = value != 0;
  return AV_OK;
}

// 0 = R2 decision, 1 = IsAccepted literally, 2 = the example's responder
int opt_responder(av_engine* e, int64_t value) {
  AV_ENTER(e);
  AV_CHECK(value >= 0 && value <= 2, AV_ERR_INVALID_ARG, "responder must be 0, 1 or 2");
  AV_CHECK(value != 2 || (e->NL == (uint32_t)e->N && e->t0 == 0 && e->t1 == e->M && e->peer_world <= 1 && !e->comm),
           AV_ERR_UNSUPPORTED, "the example responder (re-adds) needs an unsharded engine");
  AV_CHECK(value == 0 || e->peer_world <= 1, AV_ERR_UNSUPPORTED, "responder variants on a peer-push engine");
  if (value == 2 && !e->readd) {
    AV_HIP(e->readd.alloc_zeroed(e->L, e->stream));
    AV_HIP(e->died_out.alloc_zeroed(e->L, e->stream));
  }
  AV_TRY(materialize_votes(e));
  e->pub_mode = (int32_t)value;
  AV_TRY(refresh_pref(e));  // republish the current snapshot under the new rule
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

// A/B: the three snapshot buffers re-allocated uncached (hipDeviceMallocUncached: the L2 does not
// keep their lines, a gather reads the bytes it asks for instead of a 128-B line fill) or back
int opt_pref_uncached(av_engine* e, int64_t value) {
  AV_TRY(opt_range("pref_uncached", value, 0, 1));
  AV_CHECK(!e->arrive && !e->group, AV_ERR_UNSUPPORTED, "pref_uncached: not with a peer exchange");
  if ((value != 0) == e->pref_uncached) return AV_OK;
  AV_ENTER(e);
  AV_TRY(realloc_pref(e, value ? hipDeviceMallocUncached : hipDeviceMallocDefault));
  e->pref_uncached = value != 0;
  return AV_OK;
}

constexpr struct {
  const char* name;
  int (*set)(av_engine*, int64_t);
} kOptionHandlers[] = {
    {"sweep_blocks", opt_sweep_blocks},
    {"tiles_per_wave", opt_tiles_per_wave},
    {"solo_barrier", opt_solo_barrier},
    {"count_lazy", opt_count_planes<&av_engine::count_lazy>},
    {"k_hi_virtual", opt_count_planes<&av_engine::k_hi_virtual>},
    {"responder", opt_responder},
    {"pref_uncached", opt_pref_uncached},
    // 0: a round after init reads every plane (A/B only)
    {"fresh", [](av_engine* e, int64_t v) -> int {
       if (v) return AV_OK;
       if (e->facts.c_preset) {  // preset consider planes stand only while the records are fresh
         AV_ENTER(e);
         AV_TRY(materialize(e, true, false));
       }
       e->facts.option_fresh_off();
       return AV_OK;
     }},
    // may only be switched off (it is a proven invariant, not a hint)
    {"warm_skip", [](av_engine* e, int64_t v) -> int {
       if (!v) e->facts.option_warm_skip_off();
       return AV_OK;
     }},
    // before the exchange is set up: need-masked pushes (default 1)
    {"peer_mask", [](av_engine* e, int64_t v) -> int {
       AV_CHECK(e->peer_world == 0, AV_ERR_INVALID_ARG, "peer_mask must be set before the exchange is set up");
       e->peer_mask = v != 0;
       return AV_OK;
     }},
    // before av_peer_handles: fine-grained snapshot buffers (default 1)
    {"peer_fine", [](av_engine* e, int64_t v) -> int {
       AV_CHECK(!e->arrive, AV_ERR_INVALID_ARG, "peer_fine must be set before av_peer_handles");
       e->peer_fine = v != 0;
       return AV_OK;
     }},
    {"barrier_timeout_ms", [](av_engine* e, int64_t v) -> int {
       AV_TRY(opt_range("barrier_timeout_ms", v, 1, 3600000));
       e->barrier_timeout_ms = (uint32_t)v;
       e->barrier_ticks = 0;  // recomputed at the next barrier
       return AV_OK;
     }},
    // tuning (A/B): fewer updates per dense record; the dense log may fill sooner
    {"dense_min", [](av_engine* e, int64_t v) -> int {
       AV_TRY(opt_range("dense_min", v, 1, 32 * (int64_t)e->k + 1));
       e->dense_min = (uint32_t)v;
       return AV_OK;
     }},
};

}  // namespace

extern "C" {

int av_set_option(av_engine* e, const char* name, int64_t value) {
  if (e) e->facts.snapshot_written();
  AV_CHECK(e && name, AV_ERR_INVALID_ARG, "null argument");
  for (const PlainOption& o : kPlainOptions)
    if (!std::strcmp(name, o.name)) return set_plain(e, o, value);
  for (const auto& h : kOptionHandlers)
    if (!std::strcmp(name, h.name)) return h.set(e, value);
  return fail(AV_ERR_INVALID_ARG, "unknown option '%s'", name);
}

int av_set_timing(av_engine* e, int32_t enable) {
  AV_ENTER(e);
  e->timing = enable != 0;
  return AV_OK;
}

int av_kernel_stats(av_engine* e, double* total_ms, int64_t* launches) {
  AV_ENTER(e);
  AV_CHECK(total_ms && launches, AV_ERR_INVALID_ARG, "null argument");
  AV_HIP(hipStreamSynchronize(e->stream));
  for (auto& ev : e->events) {
    float ms = 0.f;
    AV_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
    e->timed_ms += ms;
    e->timed_launches++;
  }
  e->events.clear();  // destroys them
  *total_ms = e->timed_ms;
  *launches = e->timed_launches;
  e->timed_ms = 0.0;
  e->timed_launches = 0;
  return AV_OK;
}

int av_layout_info(av_engine* e, int64_t* lanes, int64_t* local_nodes, int64_t* local_blocks, int32_t* capped) {
  AV_CHECK(e, AV_ERR_INVALID_ARG, "null engine");
  if (lanes) *lanes = e->L;
  if (local_nodes) *local_nodes = e->NL;
  if (local_blocks) *local_blocks = e->BL;
  if (capped) *capped = e->capped ? 1 : 0;
  return AV_OK;
}

}  // extern "C"
