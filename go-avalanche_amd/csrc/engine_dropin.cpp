// libavhip.so: the drop-in write batches. AddTargetToReconcile for many nodes' lists and for a node
// range, RegisterVotes for Responses given by slots or by the caller's hashes. Every batch lays its
// arrays out by batch_layout.h: one function gives the size and the pointers, in pinned and in device
// memory alike.
#include <cstring>

#include "engine.h"

using namespace aveng;

namespace {

// How the messages of a call name its requests and their entries.
struct TableWords {
  const char *requests, *entries, *call;
};

// What the batches check on the caller's request table before they look at an entry (n_req > 0);
// stale tiles are written back on the way out. have_arrays: the per-entry arrays are not null.
int check_table(av_engine* e, int64_t n_req, const int64_t* nodes, const int64_t* offsets, bool have_arrays,
                const TableWords& w, int64_t* n_out) {
  AV_CHECK(n_req < (1ll << 31), AV_ERR_INVALID_ARG, "too many %s in one call", w.requests);
  AV_CHECK(offsets[0] == 0, AV_ERR_INVALID_ARG, "offsets[0] must be 0");
  for (int64_t i = 0; i < n_req; ++i) {
    AV_CHECK(offsets[i + 1] >= offsets[i], AV_ERR_INVALID_ARG, "offsets must not decrease");
    AV_CHECK(local_node(e, nodes[i]), AV_ERR_INVALID_ARG, "node %lld not in this shard", (long long)nodes[i]);
  }
  const int64_t n = offsets[n_req];
  AV_CHECK(n == 0 || have_arrays, AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(n < (1ll << 31), AV_ERR_INVALID_ARG, "too many %s in one call", w.entries);
  AV_CHECK(e->t1 - e->t0 <= (int64_t)avk::kDropTl + 1, AV_ERR_UNSUPPORTED, "%s need <= 4M local targets", w.call);
  AV_TRY(materialize_votes(e));
  *n_out = n;
  return AV_OK;
}

// The table in the kernels' form: 32-bit offsets, nodes local to the shard.
void fill_table(const av_engine* e, int64_t n_req, const int64_t* nodes, const int64_t* offsets,
                const avlay::Table& t) {
  for (int64_t i = 0; i <= n_req; ++i) t.off[i] = (uint32_t)offsets[i];
  for (int64_t i = 0; i < n_req; ++i) t.node[i] = (uint32_t)(nodes[i] - e->n0);
}

// The engine's fields of DropInParams and a batch on the device: its packed entries and its table.
avk::DropInParams dropin_params(const av_engine* e, const uint32_t* packed, const avlay::Table& tab, int64_t n_req) {
  avk::DropInParams p{};
  p.planes = e->planes;
  p.pref = e->pref[e->cur];
  p.valid = e->valid;
  p.byz = e->byz;
  p.n0 = (uint32_t)e->n0;
  p.BL = e->BL;
  p.PS = e->PS;
  p.L = e->L;
  p.round = (uint32_t)e->round;
  p.pub_mode = (uint32_t)e->pub_mode;
  p.packed = packed;
  p.resp_off = tab.off;
  p.resp_node = tab.node;
  p.n_resp = (uint32_t)n_req;
  p.order = tab.order;
  p.grp_off = tab.grp_off;
  return p;
}

// The batch's m entries grouped by lane keeping their order: lane keys on the device (k_dropin_keys; key
// L = an unknown or foreign target), the stable radix sort of (lane, position) and the run-length
// encoding (launch_group_votes). The run count comes back (4 bytes, one synchronization) and p gets
// the runs a lane kernel walks.
int group_by_lane(av_engine* e, avk::DropInParams& p, const avk::GroupScratch& g, uint32_t m) {
  int key_bits = 1;
  while (key_bits < 32 && (1ull << key_bits) < (uint64_t)e->L + 1) ++key_bits;
  AV_HIP(avk::launch_dropin_keys(p, g, e->stream));
  AV_HIP(avk::launch_group_votes(g, m, key_bits, e->stream));
  uint32_t nb = 0;
  AV_HIP(hipMemcpyAsync(&nb, g.nruns, 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  p.blocks = g.lanes;
  p.offs = g.offs;
  p.entries = g.entries;
  p.n_blocks = nb;
  return AV_OK;
}

}  // namespace

extern "C" {

int av_add_targets(av_engine* e, int64_t node, const int64_t* targets, const uint8_t* accepted, int64_t n,
                   uint8_t* added) {
  const int64_t offs[2] = {0, n};
  return av_add_targets_batch(e, 1, &node, offs, targets, accepted, added);
}

// Many Processors' AddTargetToReconcile lists in one call (processor.go:45-58 per entry, in call
// order). Nothing inside the call changes validity or deletes a record, so the first occurrence of a
// (node, target) decides and every later one returns false. The host packs each entry into one u32
// (add_word) in pinned memory; the device groups the entries by lane (group_by_lane) and walks each
// touched lane once (k_add_lanes). Copies: 4 B per entry in, 1 B back.
int av_add_targets_batch(av_engine* e, int64_t n_req, const int64_t* nodes, const int64_t* offsets,
                         const int64_t* targets, const uint8_t* accepted, uint8_t* added) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_TRY(peer_local_write_check(e));
  AV_CHECK(n_req >= 0 && (n_req == 0 || (nodes && offsets)), AV_ERR_INVALID_ARG, "null argument");
  if (n_req == 0) return AV_OK;
  int64_t n = 0;
  AV_TRY(check_table(e, n_req, nodes, offsets, targets && accepted && added, {"requests", "entries", "batched adds"},
                     &n));
  e->facts.add_targets();
  if (n == 0) return AV_OK;
  const uint32_t m = (uint32_t)n;
  const size_t temp_words = (size_t)avk::group_votes_scratch_words(m);
  // the batch in pinned memory; on the device the grouping scratch follows it
  avlay::Carver size;
  avlay::add_batch(size, m, (size_t)n_req);
  AV_HIP(e->dropin_host.reserve(size.bytes(), avmem::Slack::kMiB, hipHostMallocDefault));
  avlay::group_scratch(size, m, temp_words);
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, size.bytes(), &buf));
  avlay::Carver host(e->dropin_host.get()), dev(buf);
  const avlay::AddBatch h = avlay::add_batch(host, m, (size_t)n_req);
  const avlay::AddBatch d = avlay::add_batch(dev, m, (size_t)n_req);
  const avk::GroupScratch g = avlay::group_scratch(dev, m, temp_words);
  fill_table(e, n_req, nodes, offsets, h.tab);
  const int64_t T0 = e->t0, T1 = e->t1;
  uint32_t* const hpack = h.packed;
  parallel_chunks(n, 1 << 18, [&](int, int64_t a, int64_t b) {
    for (int64_t v = a; v < b; ++v) {
      const int64_t tg = targets[v];
      hpack[v] = avk::add_word(tg - T0, tg >= T0 && tg < T1, accepted[v] != 0);
    }
  });
  AV_HIP(hipMemcpyAsync(d.packed, h.packed, h.prefix_bytes, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipMemsetAsync(d.added, 0, (size_t)m, e->stream));
  avk::DropInParams p = dropin_params(e, d.packed, d.tab, n_req);
  AV_TRY(group_by_lane(e, p, g, m));
  AV_HIP(avk::launch_add_lanes(p, d.added, e->stream));
  AV_HIP(hipMemcpyAsync(h.added, d.added, (size_t)m, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  std::memcpy(added, h.added, (size_t)m);
  return AV_OK;
}

// AddTargetToReconcile of a target list by every node of [n0, n1) (main.go:97-103: every node adds a
// transaction when it appears). The host folds the list into the blocks it touches: per block a
// request mask, the caller's acceptance mask and, for each requested bit, the list position of its
// first occurrence (a repeat finds the record: processor.go:50-53). One table upload, one launch, the
// touched blocks' counters back, one synchronization.
int av_admit_targets(av_engine* e, int64_t n0, int64_t n1, const int64_t* targets, int64_t n, int32_t init_mode,
                     uint32_t init_param, const uint8_t* accepted, int64_t* added_nodes) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_TRY(peer_local_write_check(e));
  AV_CHECK(n >= 0 && (n == 0 || targets), AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(n < (1ll << 31), AV_ERR_INVALID_ARG, "too many targets in one call");
  AV_CHECK(init_mode >= AV_INIT_REJECTED && init_mode <= AV_INIT_GIVEN, AV_ERR_INVALID_ARG, "bad init_mode");
  AV_CHECK(init_mode != AV_INIT_GIVEN || accepted, AV_ERR_INVALID_ARG, "AV_INIT_GIVEN needs accepted[]");
  if (n0 == 0 && n1 == 0) {
    n0 = e->n0;
    n1 = e->n1;
  }
  AV_CHECK(n0 >= e->n0 && n0 <= n1 && n1 <= e->n1, AV_ERR_INVALID_ARG, "node range outside this engine's shard");
  AV_TRY(materialize_votes(e));
  e->facts.add_targets();
  if (added_nodes) std::fill(added_nodes, added_nodes + n, (int64_t)0);
  // table: tblk | treq | tacc, TB words each; first[j * 32 + bit]: list position of the bit's first occurrence
  std::vector<int32_t> slot_of(e->BL, -1);
  std::vector<uint32_t> tblk, treq, tacc;
  std::vector<int64_t> first;
  for (int64_t i = 0; i < n; ++i) {
    if (!local_target(e, targets[i])) continue;
    const int64_t tl = targets[i] - e->t0;
    const uint32_t b = (uint32_t)(tl >> 5), bit = (uint32_t)(tl & 31);
    if (slot_of[b] < 0) {
      slot_of[b] = (int32_t)tblk.size();
      tblk.push_back(b);
      treq.push_back(0u);
      tacc.push_back(0u);
      first.insert(first.end(), 32, (int64_t)-1);
    }
    const size_t j = (size_t)slot_of[b];
    if ((treq[j] >> bit) & 1u) continue;
    treq[j] |= 1u << bit;
    if (init_mode == AV_INIT_GIVEN && accepted[i]) tacc[j] |= 1u << bit;
    first[j * 32 + bit] = i;
  }
  const uint32_t TB = (uint32_t)tblk.size();
  if (!TB || n0 == n1) return AV_OK;
  std::vector<uint32_t> table;
  table.reserve(3 * (size_t)TB);
  table.insert(table.end(), tblk.begin(), tblk.end());
  table.insert(table.end(), treq.begin(), treq.end());
  table.insert(table.end(), tacc.begin(), tacc.end());
  const size_t cnt_words = added_nodes ? (size_t)TB * 32 : 0;
  avlay::Carver size;
  avlay::admit_table(size, TB, cnt_words);
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, size.bytes(), &buf));
  avlay::Carver dev(buf);
  const avlay::AdmitTable d = avlay::admit_table(dev, TB, cnt_words);
  AV_HIP(hipMemcpyAsync(d.tblk, table.data(), d.prefix_bytes, hipMemcpyHostToDevice, e->stream));
  if (cnt_words) AV_HIP(hipMemsetAsync(d.counts, 0, cnt_words * 4, e->stream));
  avk::AdmitParams p{};
  p.planes = e->planes;
  p.pref = e->pref[e->cur];
  p.valid = e->valid;
  p.byz = e->byz;
  p.tblk = d.tblk;
  p.treq = d.treq;
  p.tacc = d.tacc;
  p.counts = d.counts;
  p.seed = e->cfg.seed;
  p.n0 = (uint32_t)e->n0;
  p.nl0 = (uint32_t)(n0 - e->n0);
  p.nn = (uint32_t)(n1 - n0);
  p.TB = TB;
  p.BL = e->BL;
  p.PS = e->PS;
  p.t0 = (uint32_t)e->t0;
  p.round = (uint32_t)e->round;
  p.pub_mode = (uint32_t)e->pub_mode;
  p.mode = init_mode;
  p.param = init_param;
  // the thread mapping (DESIGN.md "Admission"): a wave per 64 nodes of one block pays a pass over every
  // node's plane lines per touched block, so it is taken for a single touched block only, where both
  // mappings reach the same words and its counting is the cheaper one; option "admit_map" forces one
  const bool lane_major = TB > 65535u || (e->admit_map ? e->admit_map == 2u : TB > 1u);
  AV_HIP(avk::launch_admit(p, lane_major, e->stream));
  std::vector<uint32_t> counts(cnt_words);
  if (cnt_words) AV_HIP(hipMemcpyAsync(counts.data(), p.counts, cnt_words * 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  for (size_t s = 0; s < cnt_words; ++s)
    if (first[s] >= 0) added_nodes[first[s]] = (int64_t)counts[s];
  return AV_OK;
}

int av_register_votes(av_engine* e, int64_t node, const int64_t* targets, const uint32_t* errs, int64_t n,
                      int32_t* status_out) {
  const int64_t offs[2] = {0, n};
  return av_register_votes_batch(e, 1, &node, offs, targets, errs, status_out);
}

}  // extern "C"

namespace {

// What av_register_votes_batch and av_register_votes_hashed derive from the caller's Response table
// before any vote is looked at.
struct RespTable {
  int64_t n = 0;               // votes
  int64_t max_node_votes = 0;  // at most one confidence step per vote: the most votes one node gets
  // the Responses grouped by node, in call order inside a group (fast path)
  std::vector<uint32_t> order, grp_off;
  uint32_t n_groups = 0;
};

// check_table for a vote call (n_resp > 0), then the Responses' grouping
int resp_table(av_engine* e, int64_t n_resp, const int64_t* nodes, const int64_t* offsets, const void* votes,
               const uint32_t* errs, const int32_t* status_out, RespTable& t) {
  AV_TRY(check_table(e, n_resp, nodes, offsets, votes && errs && status_out, {"Responses", "votes", "drop-in votes"},
                     &t.n));
  t.order.resize((size_t)n_resp);
  std::vector<std::pair<int64_t, uint32_t>> nn((size_t)n_resp);
  for (int64_t i = 0; i < n_resp; ++i) nn[(size_t)i] = {nodes[i], (uint32_t)i};
  std::sort(nn.begin(), nn.end());  // (node, Response index): call order inside a node
  for (size_t i = 0; i < nn.size();) {
    int64_t c = 0;
    size_t j = i;
    t.grp_off.push_back((uint32_t)i);
    for (; j < nn.size() && nn[j].first == nn[i].first; ++j) {
      c += offsets[nn[j].second + 1] - offsets[nn[j].second];
      t.order[j] = nn[j].second;
    }
    t.max_node_votes = std::max(t.max_node_votes, c);
    i = j;
  }
  t.grp_off.push_back((uint32_t)n_resp);
  t.n_groups = (uint32_t)t.grp_off.size() - 1u;
  return AV_OK;
}

void fill_resp_table(const av_engine* e, int64_t n_resp, const int64_t* nodes, const int64_t* offsets,
                     const RespTable& t, const avlay::Table& h) {
  fill_table(e, n_resp, nodes, offsets, h);
  std::memcpy(h.order, t.order.data(), (size_t)n_resp * 4);
  std::memcpy(h.grp_off, t.grp_off.data(), ((size_t)t.n_groups + 1) * 4);
}

// The packed votes (dpack[m], dropin_word) and the Response table dtab are on the device, the
// statuses dstat[m] preset to -1: apply them by the fast path (g null: every Response fit for
// k_dropin_resp) or by the general one over the grouping scratch g, copy the statuses to hstat
// (pinned) and widen them.
int apply_packed_votes(av_engine* e, const RespTable& t, int64_t n_resp, const uint32_t* dpack,
                       const avlay::Table& dtab, int8_t* dstat, const avk::GroupScratch* g, int8_t* hstat,
                       int32_t* status_out) {
  const uint32_t m = (uint32_t)t.n;
  avk::DropInParams p = dropin_params(e, dpack, dtab, n_resp);
  p.status_out = dstat;
  p.n_groups = t.n_groups;
  if (!g) {
    AV_HIP(avk::launch_dropin_resp(p, e->stream));
  } else {
    AV_TRY(group_by_lane(e, p, *g, m));
    AV_HIP(avk::launch_register_votes(p, e->stream));
  }
  AV_HIP(hipMemcpyAsync(hstat, dstat, (size_t)m, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  parallel_chunks(t.n, 1 << 20, [&](int, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) status_out[i] = hstat[i];
  });
  return AV_OK;
}

}  // namespace

extern "C" {

// Many Responses in one call (processor.go:61-122 for each, in order). The
// host packs each vote into one u32 (target's local index, unknown-hash, yes
// and considered bits: dropin_word) in pinned memory, in parallel, and checks
// on the way whether every Response has strictly ascending targets (a poll
// set's order, rule R1). Then:
//  * fast path (it holds): one workgroup per node applies the node's
//    Responses in call order, each lane's run of votes where it lies
//    (k_dropin_resp), no grouping step;
//  * otherwise: the votes grouped by lane (group_by_lane), then
//    k_register_votes over the runs.
// Statuses come back as one byte per vote and are widened on the host.
// Copies: 4 B per vote each way plus 1 B back (the caller's int64 hashes and
// u32 errs are never copied as such).
int av_register_votes_batch(av_engine* e, int64_t n_resp, const int64_t* nodes, const int64_t* offsets,
                            const int64_t* targets, const uint32_t* errs, int32_t* status_out) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_TRY(peer_local_write_check(e));
  AV_CHECK(n_resp >= 0 && (n_resp == 0 || (nodes && offsets)), AV_ERR_INVALID_ARG, "null argument");
  if (n_resp == 0) return AV_OK;
  RespTable rt;
  AV_TRY(resp_table(e, n_resp, nodes, offsets, targets, errs, status_out, rt));
  const int64_t n = rt.n;
  if (n == 0) {
    e->facts.dropin_votes(rt.max_node_votes, false);
    return AV_OK;
  }
  // ---- pack (pinned host staging, grown on demand and kept by the engine)
  const uint32_t m = (uint32_t)n;
  avlay::Carver size;
  avlay::vote_batch(size, m, (size_t)n_resp, rt.n_groups);
  AV_HIP(e->dropin_host.reserve(size.bytes(), avmem::Slack::kMiB, hipHostMallocDefault));
  avlay::Carver host(e->dropin_host.get());
  const avlay::VoteBatch h = avlay::vote_batch(host, m, (size_t)n_resp, rt.n_groups);
  fill_resp_table(e, n_resp, nodes, offsets, rt, h.tab);
  std::vector<uint8_t> asc_t(64, 1), neutral_t(64, 0);
  const int64_t T0 = e->t0, T1 = e->t1;
  uint32_t* const hpack = h.packed;
  parallel_chunks(n_resp, std::max<int64_t>(1, n_resp * (1 << 18) / std::max<int64_t>(1, n)),
                  [&](int t, int64_t r0, int64_t r1) {
    bool asc = true, neutral = false;
    for (int64_t r = r0; r < r1; ++r) {
      for (int64_t v = offsets[r]; v < offsets[r + 1]; ++v) {
        const int64_t tg = targets[v];
        const uint32_t err = errs[v];
        hpack[v] = avk::dropin_word(tg - T0, tg >= T0 && tg < T1, err);
        neutral |= (int32_t)err < 0;
        if (v > offsets[r]) asc &= tg > targets[v - 1];
      }
    }
    asc_t[t] = asc;
    neutral_t[t] = neutral;
  });
  bool ascending = true, neutral = false;
  for (int t = 0; t < 64; ++t) {
    ascending &= asc_t[t] != 0;
    neutral |= neutral_t[t] != 0;
  }
  e->facts.dropin_votes(rt.max_node_votes, neutral);
  const bool fast = ascending && e->dropin_fast;
  // ---- device: the batch, then the grouping scratch of the general path
  const size_t temp_words = fast ? 0 : (size_t)avk::group_votes_scratch_words(m);
  if (!fast) avlay::group_scratch(size, m, temp_words);
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, size.bytes(), &buf));
  avlay::Carver dev(buf);
  const avlay::VoteBatch d = avlay::vote_batch(dev, m, (size_t)n_resp, rt.n_groups);
  avk::GroupScratch g{};
  if (!fast) g = avlay::group_scratch(dev, m, temp_words);
  AV_HIP(hipMemcpyAsync(d.packed, h.packed, h.prefix_bytes, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipMemsetAsync(d.status, 0xFF, (size_t)m, e->stream));
  return apply_packed_votes(e, rt, n_resp, d.packed, d.tab, d.status, fast ? nullptr : &g, h.status, status_out);
}

// av_register_votes_batch with the caller's hashes in place of slots. The host copies the 8-byte
// hashes and the err classes into pinned memory and looks nothing up: the device probes its copy of
// the catalog's table per vote and writes the packed votes (catalog.hip k_catalog_pack) that both
// apply paths of the slot call consume. Whether the fast path may run (every Response's slots
// ascending) is the kernel's finding too, read back before the apply is enqueued. What the round
// plan needs is derived from the errs exactly as the slot call derives it.
// Copies: 12 B per vote in, 1 B back.
int av_register_votes_hashed(av_engine* e, int64_t n_resp, const int64_t* nodes, const int64_t* offsets,
                             const int64_t* hashes, const uint32_t* errs, int32_t* status_out) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_TRY(peer_local_write_check(e));
  AV_CHECK(n_resp >= 0 && (n_resp == 0 || (nodes && offsets)), AV_ERR_INVALID_ARG, "null argument");
  if (n_resp == 0) return AV_OK;
  RespTable rt;
  AV_TRY(resp_table(e, n_resp, nodes, offsets, hashes, errs, status_out, rt));
  const int64_t n = rt.n;
  if (n == 0) {
    e->facts.dropin_votes(rt.max_node_votes, false);
    return AV_OK;
  }
  AV_TRY(catalog_sync(e));
  // ---- the batch in pinned memory: the host fills the hashes, the errs and the Response table
  const uint32_t m = (uint32_t)n;
  avlay::Carver size;
  avlay::hashed_batch(size, m, (size_t)n_resp, rt.n_groups);
  AV_HIP(e->dropin_host.reserve(size.bytes(), avmem::Slack::kMiB, hipHostMallocDefault));
  avlay::Carver host(e->dropin_host.get());
  const avlay::HashedBatch h = avlay::hashed_batch(host, m, (size_t)n_resp, rt.n_groups);
  fill_resp_table(e, n_resp, nodes, offsets, rt, h.tab);
  std::vector<uint8_t> neutral_t(64, 0);
  int64_t* const hhash = h.hashes;
  uint32_t* const herr = h.errs;
  parallel_chunks(n, 1 << 18, [&](int t, int64_t a, int64_t b) {
    std::memcpy(hhash + a, hashes + a, (size_t)(b - a) * 8);
    bool neutral = false;
    for (int64_t v = a; v < b; ++v) {
      const uint32_t err = errs[v];
      herr[v] = err;
      neutral |= (int32_t)err < 0;
    }
    neutral_t[t] = neutral;
  });
  bool neutral = false;
  for (int t = 0; t < 64; ++t) neutral |= neutral_t[t] != 0;
  e->facts.dropin_votes(rt.max_node_votes, neutral);
  // ---- the same batch in the engine's scratch
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, size.bytes(), &buf));
  avlay::Carver dev(buf);
  const avlay::HashedBatch d = avlay::hashed_batch(dev, m, (size_t)n_resp, rt.n_groups);
  AV_HIP(hipMemcpyAsync(d.hashes, h.hashes, h.prefix_bytes, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipMemsetAsync(d.flag, 0, 4, e->stream));
  AV_HIP(hipMemsetAsync(d.status, 0xFF, (size_t)m, e->stream));
  AV_TRY(catalog_pack(e, d.hashes, d.errs, d.tab.off, (uint32_t)n_resp, m, d.packed, d.flag));
  uint32_t unordered = 1;
  AV_HIP(hipMemcpyAsync(&unordered, d.flag, 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  const bool fast = !unordered && e->dropin_fast;
  avk::GroupScratch g{};
  if (!fast) {
    // the engine's scratch holds the batch: the grouping scratch is a buffer of its own, kept
    const size_t temp_words = (size_t)avk::group_votes_scratch_words(m);
    avlay::Carver grp_size;
    avlay::group_scratch(grp_size, m, temp_words);
    AV_HIP(e->cat_group.reserve((grp_size.bytes() + 3) / 4, avmem::Slack::kEighth));
    avlay::Carver grp(e->cat_group.get());
    g = avlay::group_scratch(grp, m, temp_words);
  }
  return apply_packed_votes(e, rt, n_resp, d.packed, d.tab, d.status, fast ? nullptr : &g, h.status, status_out);
}

}  // extern "C"
