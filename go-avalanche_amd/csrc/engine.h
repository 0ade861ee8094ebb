// Internal to the host side of libavhip.so (engine*.cpp): the error macros, the engine's state and the
// helpers that cross its translation units. engine.cpp decides what a round launches and creates and
// destroys engines; engine_peer.cpp holds the peer exchange, engine_log.cpp StatusUpdate delivery,
// engine_records.cpp record I/O outside a round, engine_dropin.cpp the drop-in write batches (added
// targets and votes, laid out by batch_layout.h), engine_catalog.cpp the Hash catalog.
//
// The host objects are compiled with hidden visibility: only what include/avhip.h declares is exported.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <thread>
#include <utility>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/avhip.h"
#pragma GCC visibility pop
#include "engine_mem.h"
#include "kernels.h"
#include "round_plan.h"

namespace aveng {
// Record the calling thread's av_last_error text; returns code.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int oom_or_hip(hipError_t he) { return he == hipErrorOutOfMemory ? AV_ERR_OOM : AV_ERR_HIP; }
}  // namespace aveng

#define AV_HIP(call)                                                                                           \
  do {                                                                                                         \
    hipError_t _e = (call);                                                                                    \
    if (_e != hipSuccess) return aveng::fail(AV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                                             __FILE__, __LINE__);                                              \
  } while (0)

// propagate an AV_ERR_* code
#define AV_TRY(call)              \
  do {                            \
    int _rc = (call);             \
    if (_rc != AV_OK) return _rc; \
  } while (0)

#define AV_CHECK(cond, code, ...) \
  do {                            \
    if (!(cond)) return aveng::fail(code, __VA_ARGS__); \
  } while (0)

#define AV_ENTER(e) AV_TRY(aveng::set_device(e))

#define AV_PEER_CHECK(e) AV_TRY(aveng::peer_failed(e))

// For calls that return results: every round enqueued so far (and its
// barrier) completes first, then the flag decides.
#define AV_PEER_SYNC_CHECK(e)                                      \
  do {                                                             \
    if ((e)->peer_world > 1) AV_HIP(hipStreamSynchronize((e)->stream)); \
    AV_TRY(aveng::peer_failed(e));                                 \
  } while (0)

// An in-process peer group (av_peer_group_serial): the ranks of a node-sharded network as engines of
// one process on one device, sharing one stream; its order replaces the device barrier.
struct PeerGroup {
  std::vector<av_engine*> members;  // by rank; nullptr once destroyed
  avmem::Stream stream;             // destroyed with the group, by its last member (av_destroy)
  int alive = 0;
};

// Members are destroyed in reverse order of declaration: own_stream comes before every buffer and
// event, so they are all released before the engine's stream is destroyed (av_destroy has
// synchronized the streams by then).
struct av_engine {
  av_config cfg{};
  int64_t N = 0, M = 0, n0 = 0, n1 = 0, t0 = 0, t1 = 0;
  uint32_t NL = 0, BL = 0, L = 0, Lpad = 0;
  int k = 0;
  bool capped = false;
  // the stream created with the engine, and (not owning) the stream its work runs on: own_stream, or
  // the group's in an in-process peer group (av_peer_group_serial)
  avmem::Stream own_stream;
  hipStream_t stream = nullptr;
  avmem::DevBuf<uint32_t> planes;
  // published-preference snapshots, rotated by 3: round r reads pref[cur]
  // (S_r) and writes pref[nxt(cur)] (S_r+1); pref[prv(cur)] (S_r-1) is kept
  // for tiles whose vote planes are recomputed (vstale)
  avmem::DevBuf<uint32_t> pref[3];
  // words per node row of the preference tables: BL rounded up to a power of two (BL <= 32) or to a
  // multiple of 32 (BL > 32), so that a gathered row covers whole 128-B lines (avk::pref_stride)
  uint32_t PS = 0;
  // what the host knows about the records, and the one place each fact changes (round_plan.h)
  avk::RecordFacts facts;
  // reference rows (kernels.h ref_node / rflag_*): one flag byte per node after the preference words
  // of every snapshot buffer (so rotation, IPC export and peer pushes carry them; facts.rflag_ok)
  // option "ref_rows" (default off: measured slower): the flag loads, the reference
  // word and the writer's ballot + byte store cost more issue/latency than the 8 gathers they replace
  bool ref_rows = false;
  int64_t ref_node = -1;  // first honest node (chosen at the first round that can use it); -2: none
  size_t rflag_off = 0;   // byte offset of the flags in a snapshot buffer
  // option "uniform_rows" (default on; kernels.h uni_*): every snapshot buffer carries one mismatch
  // slot per rank at word uni_off (facts.uni_ok)
  bool uni_rows = true;
  uint32_t uni_merge = 1;  // option "uni_merge": runs per wave in a round with a uniform input (kernels.h)
  bool k_hi_virtual = true;  // option "k_hi_virtual": the K4..K7 group left unstored while counts are < 16 (kernels.h kHiVirt)
  size_t uni_off = 0;
  // option "c_preset" (default on, A/B): av_init_records stores the consider planes as all-ones where
  // the next sim round plans as a fresh sweep round (facts.c_preset, kernels.h c_preset)
  bool c_preset = true;

  int cur = 0;
  static int nxt(int c) { return c == 2 ? 0 : c + 1; }
  static int prv(int c) { return c == 0 ? 2 : c - 1; }
  // recomputed vote registers (kernels.h vv): option "virtual_votes" and the
  // smallest BL it is used at (option "vv_min_bl": below it the 7 extra
  // gathered rows cost more requests than the 64 B per lane of V planes save)
  avmem::DevBuf<uint32_t> vstale;  // [tiles]
  // deferred count planes (kernels.h klazy): option "count_lazy"
  avmem::DevBuf<uint32_t> kpend;   // [tiles]
  bool count_lazy = true;
  bool virtual_votes = true;
  uint32_t vv_min_bl = 16;
  avmem::DevBuf<uint32_t> valid;
  avmem::DevBuf<uint32_t> byz;
  avmem::DevBuf<uint64_t> log;
  // the singles', medium and dense records' per-shard counters: one array (round_common.h
  // emit_reserve_med indexes it by kind); mlog_count and dlog_count point into it (not owning)
  avmem::DevBuf<uint32_t> log_count;
  avmem::DevBuf<uint64_t> dlog;      // dense lane records (kernels.h dense_words(k) u64 each)
  uint32_t* dlog_count = nullptr;
  avmem::DevBuf<uint64_t> mlog;      // medium lane records (kernels.h med_rec_words: 4 u64 each)
  uint32_t* mlog_count = nullptr;
  uint32_t mlog_cap = 0;
  avmem::DevBuf<uint32_t> upd_count;  // StatusUpdates emitted per shard (singles + dense bits)
  uint32_t dlog_cap = 0;
  avmem::DevBuf<uint32_t> log_overflow;
  avmem::DevBuf<uint32_t> node_flags;  // capped engines: nodes k_round_node leaves to the exact pass
  uint32_t log_cap = 0;
  uint32_t log_shards = 1;
  // allocated entries of the three log kinds (all shards together); log_cap / mlog_cap / dlog_cap are
  // these divided by log_shards, which follows the round kernels' wave count (set_log_layout)
  size_t log_alloc = 0, mlog_alloc = 0, dlog_alloc = 0;
  avmem::DevBuf<unsigned long long> applied;
  // [0, kLogShards): model bytes moved; [kLogShards, 2 kLogShards): the part of them that re-reads a
  // preference word another lane of the same round already gathered (av_alg_bytes_reread)
  avmem::DevBuf<unsigned long long> bytes;
  avmem::DevBuf<unsigned long long> finalized;
  avmem::DevBuf<unsigned long long> scratch_count;
  int64_t round = 0, log_base = 0;
  // update words (kernels.h pack_update): the round field starts at bit round_shift = 28 + the node
  // field's width, max(24, bits of N); the log spans at most 2^(64 - round_shift) rounds
  uint32_t round_shift = 52;
  int64_t max_log_rounds() const { return (int64_t)1 << (64 - round_shift); }
  bool plane_nt = true;  // tuning option "plane_nt" (A/B on MI355X: -8 % kernel time warm, -16 % cold)
  bool ablate_gather = false;  // diagnostics option "ablate_gather" (invalid results)
  uint32_t ablate_node = 0;  // diagnostics option "ablate_node" (k_round_node, invalid results)
  int ablate_emit = 0;  // diagnostics option "ablate_emit": 1 = StatusUpdates counted, not stored; 2 = no reserving atomic; 3 = atomic issued, result unused
  uint32_t ablate_phase = 0;  // diagnostics option "ablate_phase" (kernels.h; results invalid)
  // diagnostics option "unsynced_shard": a node-sharded engine runs rounds with no exchange (other
  // shards' preference rows keep their initial values; per-rank kernel timing only, invalid results)
  bool unsynced_shard = false;
  // diagnostics option "warm_pref": before each timed round, read the snapshots the round gathers
  // from (untimed), as a GPU of the rank's own would hold them in its caches (tools/group_model.py:
  // the serial group runs every rank's kernel on one GPU, each after the others' traffic)
  bool warm_pref = false;
  avmem::DevBuf<uint32_t> touch_sink;
  // round kernels (option "kernel"): 2 = k_round_sweep (uncapped) / k_round_node (capped), k <= 8;
  // 1 = k_round_fast / k_round_capped (the first versions; any k, A/B baseline)
  int kernel = 2;
  uint32_t sweep_blocks = 0;  // resident workgroups of the sweep grid (option "sweep_blocks"; 0 = one wave per tile)
  bool sweep_blocks_explicit = false;  // "sweep_blocks" set to a value >= 0: "tiles_per_wave" leaves it alone
  // option "sweep_nopipe": a walking grid runs without next-tile prefetch
  // (kModeWarm; default); 0 = the prefetching kModeWarmPipe (A/B)
  bool sweep_nopipe = true;
  // option "wave_runs": a walking grid gives each wave a run of consecutive
  // tiles whose peers one Philox pass draws (sweep_tile.h WaveDraw)
  bool wave_runs = true;
  // option "settled_fast": settled warm tiles skip the round step's bookkeeping
  bool settled_fast = true;
  // option "settled_lean": with BL dividing 64, a wave tests its run's settled candidates in one
  // lean loop first (sweep_settled.h settled_run)
  bool settled_lean = true;
  // option "tiles_per_wave" (default grid, default_sweep_blocks); 0 = by size: up to 16, at most BL, with
  // >= 15000 waves (C4: 500k tiles, 16 per wave; C3's 98k tiles: 4 — 8 per wave leaves two generations
  // of waves and was 6 % slower)
  uint32_t tiles_per_wave = 0;
  uint32_t bl_magic = 1, bl_sh1 = 0, bl_sh2 = 0;
  uint32_t store_policy = 0;  // option "store_policy": 2 = sc1 (write-through) plane stores, 3 = nt sc1
  std::vector<uint32_t> valid_host;
  // replay stream (av_replay_prepare: replay_ready rounds from replay_first)
  avmem::DevBuf<uint32_t> replay;
  int64_t replay_first = 0, replay_ready = 0;
  int replay_fuse = 16;  // option "replay_fuse": replay rounds per k_replay_node launch (capped engines; <= 1: off)
  bool replay_fast = true;  // option "replay_fast": k_replay_fast for nodes whose poll set is their first 128 lanes
  // timing
  bool timing = false;
  bool round_marker = false;  // option "round_marker" (diagnostics)
  avmem::Event marker;
  std::vector<std::pair<avmem::Event, avmem::Event>> events;
  double timed_ms = 0.0;
  int64_t timed_launches = 0;
  // RCCL
  ncclComm_t comm = nullptr;
  // peer-push exchange (av_peer_init): every rank's three
  // snapshot buffers and arrival slots mapped into this process over IPC
  int peer_world = 0, peer_rank = 0;
  uint32_t* peer_pref[3][avk::kMaxPeers + 1] = {};  // [buffer][rank]; own rank = the local buffer
  avmem::DevBuf<uint32_t> arrive;                    // [kMaxPeers + 1] arrival slots (local)
  // barrier timeout flag in pinned host memory (the barrier kernel stores it
  // with system scope): the host reads it without synchronizing the stream
  avmem::PinnedBuf<volatile uint32_t> barrier_err_host;
  uint32_t* barrier_err = nullptr;                   // device view of barrier_err_host (not owning)
  bool failed = false;                               // sticky: a peer barrier timed out
  bool pref_uncached = false;  // option "pref_uncached": snapshot buffers in uncached device memory (A/B)
  bool peer_fine = true;  // option "peer_fine": snapshot buffers fine-grained once exported (xGMI coherence)
  size_t pref_alloc_words = 0;
  uint32_t barrier_seq = 0;
  uint32_t barrier_timeout_ms = 30000;
  std::vector<void*> peer_opened;                    // IPC mappings to close
  avk::PeerPtrs peer_arrive{};
  avmem::DevBuf<uint32_t*> push_tbl;                 // device [3][kMaxPeers]: peers' replicas of each buffer
  uint64_t barrier_ticks = 0;                        // barrier_timeout_ms in wall-clock ticks (peer_timeout_ticks)
  // diagnostics option "solo_barrier": a one-rank barrier (the same 1-wave kernel, world 1) after every
  // round of an engine without a peer exchange — the exchange's fixed cost per round without the
  // pushes and without other ranks (tools/exchange_cost.py)
  bool solo_barrier = false;
  // sticky: solo_barrier was enabled at some point (its arrival slots were allocated and its barrier
  // sequence advanced outside an exchange): this engine can no longer join a peer exchange
  bool solo_used = false;
  // in-process peer group (av_peer_group_serial): stream is the group's stream
  PeerGroup* group = nullptr;
  // need-masked exchange (option "peer_mask", default on; kernels.h RoundParams::need / stale,
  // DESIGN.md §5): a sweep round pushes a row segment only to the peers whose nodes draw that row in
  // the next round, and remembers per segment, buffer and peer the changes it withheld
  bool peer_mask = true;
  bool push_defer = true;          // option "push_defer": sweep pushes queued per wave (RoundParams::push_q)
  uint32_t push_store = 1;         // option "push_store" (RoundParams::push_store)
  uint32_t tile_draw = 0;          // option "tile_draw" (RoundParams::tile_draw, A/B)
  uint32_t mat_run = 1;            // option "materialize_run" (RoundParams::mat_run, A/B)
  uint32_t census_blocks = 0;      // option "census_blocks": workgroups of av_census's grid (0 = the engine's choice)
  bool masked = false;             // set up by the exchange's initialisation (mask_setup)
  uint32_t segs = 1;               // 32-word segments per row
  avmem::DevBuf<uint8_t> need_mine;  // [kNeedWin][N]: rows this rank's nodes draw in a window's rounds
  avmem::DevBuf<uint8_t> needmask;   // [kNeedWin][NL]: peers (push order) that draw each local row
  avmem::DevBuf<uint8_t> stale;      // [3][NL * segs]: per snapshot buffer, peers whose copy may differ
  // [2][world][kNeedWin][ceil(NL/32)]: the peers' drawn-row bits. Not owning in an IPC exchange, where
  // it lies inside the exported arrival allocation (arrive, at kNeedinOff); a serial group's engines
  // own theirs, in needin_own
  uint32_t* needin = nullptr;
  avmem::DevBuf<uint32_t> needin_own;
  avk::PeerPtrs peer_needin{};     // every rank's needin
  int64_t need_ready = -1;         // window whose needmask is combined
  int64_t need_pushed = -1;        // window whose drawn rows were pushed to the peers
  // the next window's rows are drawn on a side stream while the current window's rounds run
  // (need_draw_ahead): need_free = the last push that read need_mine, need_drawn = the draw done
  avmem::Stream need_stream;
  avmem::Event need_free, need_drawn;
  int64_t need_drawn_w = -1;       // window whose rows the side stream drew (or is drawing)
  // changed published words (kernels.h RoundParams::changed): counted in every peer-push round and,
  // with option "count_changed", in every sweep round
  avmem::DevBuf<unsigned long long> changed;
  bool count_changed = false;
  // the reference-row flag bytes of every buffer were cleared (or the engine created) at this round;
  // a flag byte carries a 7-bit round tag, so they are cleared again before 128 rounds have passed
  int64_t rflag_clear_round = 0;

  // responder variant (option "responder", kernels.h pub_mode) and the nodes
  // that no longer poll (av_set_polling); both run the first-generation kernel
  uint32_t dense_min = 0;  // option "dense_min" (kernels.h dense records; default dense_min(k))
  uint32_t wave_dense = 0;  // option "wave_dense" (kernels.h RoundParams::wave_dense; A/B)
  uint32_t uni_votes = 1;   // option "uni_votes" (kernels.h RoundParams::uni_votes)
  uint32_t quiet_tiles = 1; // option "quiet_tiles" (kernels.h RoundParams::quiet_tiles; 0: every settled tile is walked)
  uint32_t calm_tiles = 1;  // option "calm_tiles" (kernels.h RoundParams::calm; 0: such tiles regather)
  // network-quiet rounds (kernels.h nq_*): option "net_quiet" (0: every run tests its own tiles) and
  // "net_quiet_group", the runs a leader wave takes (A/B on MI355X, profiles/r09/ab_net_quiet.log)
  uint32_t net_quiet = 1;
  uint32_t nq_group = 16;
  uint32_t nq_front = 1;    // option "net_quiet_front" (kernels.h nq_front; 0: every nq_group-th wave leads, A/B)
  avmem::DevBuf<uint32_t> nq;  // [0], [1]: the word of even / odd rounds; [2]: rounds that took the path
  int32_t pub_mode = 0;
  avmem::DevBuf<uint32_t> readd;     // [L] pub_mode 2: re-add marks
  avmem::DevBuf<uint32_t> died_out;  // [L] pub_mode 2: records deleted this round
  std::vector<uint32_t> nopoll_host;
  avmem::DevBuf<uint32_t> nopoll;    // [ceil(NL/32)]
  bool any_nopoll = false;
  // lost Responses and unresponsive nodes (rule R5; av_set_loss, av_set_responding): sim rounds run
  // k_round_lossy while lossy() holds. responding: bit n = node n of the whole network answers
  // queries; allocated, like the counter, by the first call that needs it
  uint32_t loss_threshold = 0;
  bool loss_neutral = false;
  std::vector<uint32_t> responding_host;
  avmem::DevBuf<uint32_t> responding;           // [ceil(N/32)]
  bool any_down = false;
  avmem::DevBuf<unsigned long long> lost;       // [kLogShards] lost Responses (av_lost_responses)
  bool lossy() const { return loss_threshold != 0 || any_down; }
  // per-node peer lists (rule R6; av_set_peer_lists): while `listed` holds, sim rounds run
  // k_round_listed and the peer dumps draw from the lists. Both arrays are replaced as a pair, after
  // the stream has drained, so a round already enqueued keeps the lists it was enqueued under.
  bool listed = false;
  avmem::DevBuf<uint32_t> list_offsets;         // [NL + 1] into list_peers, by local node
  avmem::DevBuf<uint32_t> list_peers;           // global ids, strictly ascending per node
  avmem::DevBuf<unsigned long long> unsent;     // [kLogShards] empty slots (av_unsent_polls)
  // per-local-node Processor.round (processor.go:15,40-42): a field only the
  // caller changes (avalanche_test.go:302); allocated on the first set
  std::vector<int64_t> proc_round;
  // device scratch kept across calls (StatusUpdate delivery, digests)
  avmem::DevBuf<void> fetch_scratch;
  avmem::DevBuf<unsigned long long> digest;  // [3]
  // drop-in batches (av_register_votes_batch): pinned host staging; option "dropin_fast" (0: always the
  // sort-grouped general path, A/B and tests)
  avmem::PinnedBuf<void> dropin_host;
  // StatusUpdate delivery into pageable caller memory: two pinned staging chunks (copy_out)
  avmem::PinnedBuf<void> stage[2];
  avmem::Event stage_ev[2];
  bool dropin_fast = true;
  // option "admit_map" (A/B and tests): av_admit_targets' thread mapping, 0 = by the touched blocks,
  // 1 = a wave per 64 nodes of one block, 2 = lane-major (kernels.h launch_admit)
  uint32_t admit_map = 0;
  // StatusUpdate encoder (log_ops.hip launch_encode_log): error flags and per-pass totals (device)
  avmem::DevBuf<uint32_t> enc_err;
  avmem::DevBuf<uint64_t> enc_tot;  // [4]
  uint32_t enc_buckets = 1u << 26;  // option "enc_buckets": (round, node) buckets per encoder pass
  // option "copy_blocks": workgroups of the compact stream's device-to-host copy kernel (k_stream_out);
  // 0 = hipMemcpyAsync (the runtime's copy)
  uint32_t copy_blocks = 0;
  // compact stream delivery (av_fetch_compact_async / _wait): kSlots slots, each a device buffer
  // the encoder writes and a pinned host buffer its copy lands in, the copy on copy_stream (overlaps
  // the next rounds on the engine stream); ticket t uses slot t % kSlots
  static constexpr int kSlots = 3;
  avmem::Stream copy_stream;
  avmem::DevBuf<uint8_t> cdev[kSlots];
  avmem::PinnedBuf<uint8_t> chost[kSlots];
  avmem::Event cev[kSlots];
  av_compact_header chdr[kSlots] = {};
  int64_t cticket = 0;           // next ticket
  bool cpend[kSlots] = {};       // a copy was issued into the slot
  // high-water marks: a slot that grows grows to the largest stream seen, so a caller's warm-up pass
  // sizes every slot and later rounds never allocate (pinned allocations take tens of ms)
  size_t cdev_hwm = 0, chost_hwm = 0;
  // batched poll sets (av_get_invs_batch): host-mapped pinned output the fill kernel writes
  avmem::PinnedBuf<void> invs_host;
  // the Hash catalog over [t0, t1) (catalog.h; set up by the first call that needs it, so an engine
  // that never uses it pays nothing) and the device copy of its table image, brought up to date by
  // catalog_sync before a device lookup. cat_group: the grouping scratch of a hashed vote batch that
  // turns out to need the general path (the engine's scratch holds the batch by then).
  avcat::Catalog cat;
  avmem::DevBuf<avcat::Entry> cat_dev;
  avmem::DevBuf<uint32_t> cat_group;
  uint32_t catalog_blocks = 0;  // option "catalog_blocks": workgroups of the lookup kernel (0 = by size)
  bool catalog_lds = true;      // option "catalog_lds" (A/B and tests; 0: tables of any size probed in global memory)

  size_t round_replay_words() const { return avk::replay_words(Lpad, k); }
};

// Helpers that cross the engine's translation units, by the file that defines them.
namespace aveng {

// ---- engine.cpp
int set_device(av_engine* e);
avk::RoundParams round_params(const av_engine* e, const uint32_t* replay);
int materialize(av_engine* e, bool votes, bool counts);
int materialize_votes(av_engine* e);
int engine_scratch(av_engine* e, size_t bytes, void** out);
int ref_pick(av_engine* e);
uint32_t default_sweep_blocks(const av_engine* e, bool force = false);
uint64_t log_writer_waves(const av_engine* e);
uint64_t log_shards_for(uint64_t writers);
void set_log_layout(av_engine* e);
int refresh_pref(av_engine* e);

// ---- engine_peer.cpp
int group_alive(const av_engine* e);
int push_own_rows(av_engine* e, int b);
int peer_barrier(av_engine* e, int slot_buf = -1);
int stale_clear(av_engine* e, int b);
int need_gen(av_engine* e, int64_t w);
int need_draw_ahead(av_engine* e, int64_t w);
int need_combine(av_engine* e, int64_t w);
int peer_failed(av_engine* e);
int alloc_arrival(av_engine* e);
int realloc_pref(av_engine* e, unsigned flags);

// ---- engine_log.cpp
int relayout_log_if_empty(av_engine* e);

// ---- engine_catalog.cpp
// The device copy of the catalog's table image equals the host image (entry patches, or the whole
// image after a rebuild); the stream is synchronized, so the host image may change again at once.
int catalog_sync(av_engine* e);
// hashes[0 .. n) looked up on the device (dh: their 16-byte-aligned device copy) into packed words
// (dropin_word; errs / resp_off / unordered as CatalogPackParams); enqueued on the engine's stream.
int catalog_pack(av_engine* e, const int64_t* dh, const uint32_t* derr, const uint32_t* dresp_off, uint32_t n_resp,
                 uint32_t n, uint32_t* dpacked, uint32_t* dunordered);

// ---- defined here
// Host work of the drop-in path (packing the caller's votes, expanding the
// statuses) split over threads for large batches: the box's CPU share
// (OMP_NUM_THREADS, else up to 16 hardware threads).
inline int host_threads() {
  static const int n = [] {
    int t = 0;
    if (const char* s = std::getenv("OMP_NUM_THREADS")) t = std::atoi(s);
    if (t <= 0) t = (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    return std::max(1, std::min(t, 64));
  }();
  return n;
}

// How a query of counters starts: the rounds enqueued so far have finished, out is not null.
inline int counter_query(av_engine* e, const void* out) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(out, AV_ERR_INVALID_ARG, "null argument");
  return AV_OK;
}

// Peer-push engines keep every replica of a snapshot buffer identical; a
// write to this rank's rows outside a round would break that.
inline int peer_local_write_check(const av_engine* e) {
  AV_CHECK(e->peer_world <= 1, AV_ERR_UNSUPPORTED,
           "record writes outside a round are not supported on a peer-push node-sharded engine");
  return AV_OK;
}

inline bool local_node(const av_engine* e, int64_t node) { return node >= e->n0 && node < e->n1; }
inline bool local_target(const av_engine* e, int64_t t) { return t >= e->t0 && t < e->t1; }

// f(thread, begin, end) over [0, n) split into chunks of at least min_chunk, on up to host_threads()
// threads.
template <class F>
void parallel_chunks(int64_t n, int64_t min_chunk, F f) {
  const int t = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), n / std::max<int64_t>(1, min_chunk)));
  if (t <= 1) {
    f(0, (int64_t)0, n);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(t);
  for (int i = 0; i < t; ++i) th.emplace_back([&, i] { f(i, n * i / t, n * (i + 1) / t); });
  for (auto& x : th) x.join();
}

}  // namespace aveng
