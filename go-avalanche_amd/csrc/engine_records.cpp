// libavhip.so: record I/O outside a round. Validity and added targets, the drop-in vote batches,
// reads and writes of records, preferences and poll sets, the census and the counter queries.
#include <cstring>

#include "engine.h"

using namespace aveng;

namespace {

// Peer-push engines keep every replica of a snapshot buffer identical; a
// write to this rank's rows outside a round would break that.
int peer_local_write_check(const av_engine* e) {
  AV_CHECK(e->peer_world <= 1, AV_ERR_UNSUPPORTED,
           "record writes outside a round are not supported on a peer-push node-sharded engine");
  return AV_OK;
}

// A sharded 64-bit device counter (kLogShards words at dev) copied back and added up.
int sum_shards(av_engine* e, const unsigned long long* dev, int64_t* out) {
  std::vector<unsigned long long> c(avk::kLogShards);
  AV_HIP(hipMemcpyAsync(c.data(), dev, avk::kLogShards * 8, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  unsigned long long t = 0;
  for (auto v : c) t += v;
  *out = (int64_t)t;
  return AV_OK;
}

}  // namespace

extern "C" {

int av_set_valid(av_engine* e, int64_t target, int32_t valid) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_CHECK(target >= 0 && target < e->M, AV_ERR_INVALID_ARG, "target out of range");
  if (!local_target(e, target)) return AV_OK;
  AV_TRY(materialize_votes(e));  // stale tiles must not gain live-but-invalid records
  const int64_t tl = target - e->t0;
  const uint32_t b = (uint32_t)(tl >> 5), m = 1u << (tl & 31);
  e->valid_host[b] = valid ? (e->valid_host[b] | m) : (e->valid_host[b] & ~m);
  AV_HIP(hipMemcpyAsync(e->valid + b, &e->valid_host[b], 4, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_add_targets(av_engine* e, int64_t node, const int64_t* targets, const uint8_t* accepted, int64_t n,
                   uint8_t* added) {
  const int64_t offs[2] = {0, n};
  return av_add_targets_batch(e, 1, &node, offs, targets, accepted, added);
}

// Many Processors' AddTargetToReconcile lists in one call (processor.go:45-58 per entry, in call
// order). Nothing inside the call changes validity or deletes a record, so the first occurrence of a
// (node, target) decides and every later one returns false. The host packs each entry into one u32
// (add_word) in pinned memory; the device forms the lane keys (k_dropin_keys), groups the entries by
// lane keeping their order (launch_group_votes) and walks each touched lane once (k_add_lanes).
// Copies: 4 B per entry in, 1 B back.
int av_add_targets_batch(av_engine* e, int64_t n_req, const int64_t* nodes, const int64_t* offsets,
                         const int64_t* targets, const uint8_t* accepted, uint8_t* added) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_TRY(peer_local_write_check(e));
  AV_CHECK(n_req >= 0 && (n_req == 0 || (nodes && offsets)), AV_ERR_INVALID_ARG, "null argument");
  if (n_req == 0) return AV_OK;
  AV_CHECK(n_req < (1ll << 31), AV_ERR_INVALID_ARG, "too many requests in one call");
  AV_CHECK(offsets[0] == 0, AV_ERR_INVALID_ARG, "offsets[0] must be 0");
  for (int64_t i = 0; i < n_req; ++i) {
    AV_CHECK(offsets[i + 1] >= offsets[i], AV_ERR_INVALID_ARG, "offsets must not decrease");
    AV_CHECK(local_node(e, nodes[i]), AV_ERR_INVALID_ARG, "node %lld not in this shard", (long long)nodes[i]);
  }
  const int64_t n = offsets[n_req];
  AV_CHECK(n == 0 || (targets && accepted && added), AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(n < (1ll << 31), AV_ERR_INVALID_ARG, "too many entries in one call");
  AV_CHECK(e->t1 - e->t0 <= (int64_t)avk::kDropTl + 1, AV_ERR_UNSUPPORTED, "batched adds need <= 4M local targets");
  AV_TRY(materialize_votes(e));
  e->facts.add_targets();
  if (n == 0) return AV_OK;
  const uint32_t m = (uint32_t)n;
  // ---- pack (pinned): entries, then the request table, then the result bytes
  const size_t tab_words = 2 * (size_t)n_req + 1;  // off, node
  AV_HIP(e->dropin_host.reserve(((size_t)m + tab_words) * 4 + (size_t)m + 64, avmem::Slack::kMiB, hipHostMallocDefault));
  auto* hpack = static_cast<uint32_t*>(e->dropin_host.get());
  auto* hoff = hpack + m;
  auto* hnode = hoff + n_req + 1;
  auto* hadd = reinterpret_cast<uint8_t*>(hnode + n_req);
  for (int64_t i = 0; i <= n_req; ++i) hoff[i] = (uint32_t)offsets[i];
  for (int64_t i = 0; i < n_req; ++i) hnode[i] = (uint32_t)(nodes[i] - e->n0);
  const int64_t T0 = e->t0, T1 = e->t1;
  parallel_chunks(n, 1 << 18, [&](int, int64_t a, int64_t b) {
    for (int64_t v = a; v < b; ++v) {
      const int64_t tg = targets[v];
      hpack[v] = avk::add_word(tg - T0, tg >= T0 && tg < T1, accepted[v] != 0);
    }
  });
  // ---- device: packed | off | node | result bytes || keys vidx info keys_s perm_s keys_t perm_t lanes
  // offs(m+1) nruns entries(2m) | u64 scratch (radix sort, run scan)
  int key_bits = 1;
  while (key_bits < 32 && (1ull << key_bits) < (uint64_t)e->L + 1) ++key_bits;  // L = foreign targets
  const size_t tb = (size_t)avk::group_votes_scratch_words(m) * 8;
  const size_t head_words = (size_t)m + tab_words + ((size_t)m + 3) / 4;
  const size_t grp_words = 8 * (size_t)m + ((size_t)m + 1) + 1 + 2 * (size_t)m;
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, (head_words + grp_words) * 4 + tb + 512, &buf));
  auto* w = static_cast<uint32_t*>(buf);
  uint32_t *dpack = w, *doff = dpack + m, *dnode = doff + n_req + 1;
  auto* dadd = reinterpret_cast<uint8_t*>(dnode + n_req);
  AV_HIP(hipMemcpyAsync(dpack, hpack, ((size_t)m + tab_words) * 4, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipMemsetAsync(dadd, 0, (size_t)m, e->stream));
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
  p.packed = dpack;
  p.resp_off = doff;
  p.resp_node = dnode;
  p.n_resp = (uint32_t)n_req;
  uint32_t* g0 = w + head_words;
  uint32_t *keys = g0, *vidx = keys + m, *info = vidx + m, *keys_s = info + m, *perm_s = keys_s + m,
           *keys_t = perm_s + m, *perm_t = keys_t + m, *lanes = perm_t + m, *offs = lanes + m, *nruns = offs + m + 1,
           *ent = nruns + 1;
  auto* temp = reinterpret_cast<uint64_t*>(((uintptr_t)(ent + 2 * (size_t)m) + 255) & ~(uintptr_t)255);
  AV_HIP(avk::launch_dropin_keys(p, keys, vidx, info, e->stream));
  AV_HIP(avk::launch_group_votes(temp, keys, vidx, info, m, key_bits, keys_s, perm_s, keys_t, perm_t, lanes, offs,
                                 nruns, ent, e->stream));
  uint32_t nb = 0;
  AV_HIP(hipMemcpyAsync(&nb, nruns, 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  p.blocks = lanes;
  p.offs = offs;
  p.entries = ent;
  p.n_blocks = nb;
  AV_HIP(avk::launch_add_lanes(p, dadd, e->stream));
  AV_HIP(hipMemcpyAsync(hadd, dadd, (size_t)m, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  std::memcpy(added, hadd, (size_t)m);
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
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, (3 * (size_t)TB + cnt_words) * 4, &buf));
  auto* d = static_cast<uint32_t*>(buf);
  AV_HIP(hipMemcpyAsync(d, table.data(), table.size() * 4, hipMemcpyHostToDevice, e->stream));
  if (cnt_words) AV_HIP(hipMemsetAsync(d + 3 * (size_t)TB, 0, cnt_words * 4, e->stream));
  avk::AdmitParams p{};
  p.planes = e->planes;
  p.pref = e->pref[e->cur];
  p.valid = e->valid;
  p.byz = e->byz;
  p.tblk = d;
  p.treq = d + TB;
  p.tacc = d + 2 * (size_t)TB;
  p.counts = cnt_words ? d + 3 * (size_t)TB : nullptr;
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

// What av_register_votes_batch and av_register_votes_hashed check and derive from the caller's
// Response table before any vote is looked at (n_resp > 0).
struct RespTable {
  int64_t n = 0;               // votes
  int64_t max_node_votes = 0;  // at most one confidence step per vote: the most votes one node gets
  // the Responses grouped by node, in call order inside a group (fast path)
  std::vector<uint32_t> order, grp_off;
  uint32_t n_groups = 0;
};

int resp_table(av_engine* e, int64_t n_resp, const int64_t* nodes, const int64_t* offsets, const void* votes,
               const uint32_t* errs, const int32_t* status_out, RespTable& t) {
  AV_CHECK(n_resp < (1ll << 31), AV_ERR_INVALID_ARG, "too many Responses in one call");
  AV_CHECK(offsets[0] == 0, AV_ERR_INVALID_ARG, "offsets[0] must be 0");
  for (int64_t i = 0; i < n_resp; ++i) {
    AV_CHECK(offsets[i + 1] >= offsets[i], AV_ERR_INVALID_ARG, "offsets must not decrease");
    AV_CHECK(local_node(e, nodes[i]), AV_ERR_INVALID_ARG, "node %lld not in this shard", (long long)nodes[i]);
  }
  const int64_t n = offsets[n_resp];
  AV_CHECK(n == 0 || (votes && errs && status_out), AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(n < (1ll << 31), AV_ERR_INVALID_ARG, "too many votes in one call");
  AV_CHECK(e->t1 - e->t0 <= (int64_t)avk::kDropTl + 1, AV_ERR_UNSUPPORTED, "drop-in votes need <= 4M local targets");
  AV_TRY(materialize_votes(e));
  t.n = n;
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

// words of the Response table on the device: off (n_resp + 1), node, order, grp_off (n_groups + 1)
size_t resp_table_words(int64_t n_resp, const RespTable& t) {
  return 2 * (size_t)n_resp + 1 + (size_t)n_resp + t.n_groups + 1;
}

void fill_resp_table(const av_engine* e, int64_t n_resp, const int64_t* nodes, const int64_t* offsets,
                     const RespTable& t, uint32_t* hoff) {
  auto* hnode = hoff + n_resp + 1;
  auto* horder = hnode + n_resp;
  auto* hgrp = horder + n_resp;
  for (int64_t i = 0; i <= n_resp; ++i) hoff[i] = (uint32_t)offsets[i];
  for (int64_t i = 0; i < n_resp; ++i) hnode[i] = (uint32_t)(nodes[i] - e->n0);
  std::memcpy(horder, t.order.data(), (size_t)n_resp * 4);
  std::memcpy(hgrp, t.grp_off.data(), ((size_t)t.n_groups + 1) * 4);
}

// words of the general path's grouping scratch for m votes, and its radix / scan bytes
size_t group_words(uint32_t m) { return 8 * (size_t)m + ((size_t)m + 1) + 1 + 2 * (size_t)m; }

// The packed votes (dpack[m], dropin_word) and the Response table (doff: fill_resp_table's layout)
// are on the device, the statuses dstat[m] preset to -1: apply them by the fast path (every
// Response fit for k_dropin_resp) or by the general one (grp: group_words(m) words, then 256 bytes
// of slack and group_votes_scratch_words(m) u64), copy the statuses to hstat (pinned) and widen them.
int apply_packed_votes(av_engine* e, const RespTable& t, int64_t n_resp, uint32_t* dpack, uint32_t* doff,
                       int8_t* dstat, bool fast, uint32_t* grp, int8_t* hstat, int32_t* status_out) {
  const uint32_t m = (uint32_t)t.n;
  uint32_t *dnode = doff + n_resp + 1, *dorder = dnode + n_resp, *dgrp = dorder + n_resp;
  avk::DropInParams p{};
  p.planes = e->planes;
  p.pref = e->pref[e->cur];
  p.valid = e->valid;
  p.byz = e->byz;
  p.status_out = dstat;
  p.n0 = (uint32_t)e->n0;
  p.BL = e->BL;
  p.PS = e->PS;
  p.L = e->L;
  p.round = (uint32_t)e->round;
  p.pub_mode = (uint32_t)e->pub_mode;
  p.packed = dpack;
  p.resp_off = doff;
  p.resp_node = dnode;
  p.n_resp = (uint32_t)n_resp;
  p.order = dorder;
  p.grp_off = dgrp;
  p.n_groups = t.n_groups;
  if (fast) {
    AV_HIP(avk::launch_dropin_resp(p, e->stream));
  } else {
    int key_bits = 1;
    const uint64_t keys_total = (uint64_t)e->L + 1;  // L = unknown targets
    while (key_bits < 32 && (1ull << key_bits) < keys_total) ++key_bits;
    uint32_t *keys = grp, *vidx = keys + m, *info = vidx + m, *keys_s = info + m, *perm_s = keys_s + m,
             *keys_t = perm_s + m, *perm_t = keys_t + m, *lanes = perm_t + m, *offs = lanes + m,
             *nruns = offs + m + 1, *ent = nruns + 1;
    auto* temp = reinterpret_cast<uint64_t*>(((uintptr_t)(ent + 2 * (size_t)m) + 255) & ~(uintptr_t)255);
    AV_HIP(avk::launch_dropin_keys(p, keys, vidx, info, e->stream));
    AV_HIP(avk::launch_group_votes(temp, keys, vidx, info, m, key_bits, keys_s, perm_s, keys_t, perm_t, lanes, offs,
                                   nruns, ent, e->stream));
    uint32_t nb = 0;
    AV_HIP(hipMemcpyAsync(&nb, nruns, 4, hipMemcpyDeviceToHost, e->stream));
    AV_HIP(hipStreamSynchronize(e->stream));
    p.blocks = lanes;
    p.offs = offs;
    p.entries = ent;
    p.n_blocks = nb;
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
//  * otherwise: lane keys on the device, the hand-written stable radix sort
//    of (lane, vote position) and run-length encoding (log_ops.hip
//    launch_group_votes, dev_scan.h), then
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
  const int64_t n = rt.n, max_node_votes = rt.max_node_votes;
  if (n == 0) {
    e->facts.dropin_votes(max_node_votes, false);
    return AV_OK;
  }
  // ---- pack (pinned): votes, then the Response table
  const size_t tab_words = resp_table_words(n_resp, rt);
  const size_t hb = (size_t)n * 5 + tab_words * 4 + 64;
  // (pinned host staging, grown on demand and kept by the engine)
  AV_HIP(e->dropin_host.reserve(hb, avmem::Slack::kMiB, hipHostMallocDefault));
  auto* hpack = static_cast<uint32_t*>(e->dropin_host.get());
  auto* hoff = hpack + n;
  auto* hstat = reinterpret_cast<int8_t*>(hoff + tab_words);
  fill_resp_table(e, n_resp, nodes, offsets, rt, hoff);
  std::vector<uint8_t> asc_t(64, 1), neutral_t(64, 0);
  const int64_t T0 = e->t0, T1 = e->t1;
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
  e->facts.dropin_votes(max_node_votes, neutral);
  const bool fast = ascending && e->dropin_fast;
  // ---- device: packed votes + Response table + byte statuses (+ grouping scratch)
  const uint32_t m = (uint32_t)n;
  const size_t tb = fast ? 0 : (size_t)avk::group_votes_scratch_words(m) * 8;
  // packed | off | node | status bytes || keys vidx info keys_s perm_s keys_t perm_t lanes offs(m+1) nruns
  // entries(2m) | u64 scratch (radix sort, run scan)
  const size_t head_words = (size_t)m + tab_words + ((size_t)m + 3) / 4;
  const size_t grp_words = fast ? 0 : group_words(m);
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, (head_words + grp_words) * 4 + tb + 512, &buf));
  auto* w = static_cast<uint32_t*>(buf);
  uint32_t *dpack = w, *doff = dpack + m;
  auto* dstat = reinterpret_cast<int8_t*>(doff + tab_words);
  AV_HIP(hipMemcpyAsync(dpack, hpack, ((size_t)m + tab_words) * 4, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipMemsetAsync(dstat, 0xFF, (size_t)m, e->stream));
  return apply_packed_votes(e, rt, n_resp, dpack, doff, dstat, fast, w + head_words, hstat, status_out);
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
  // ---- pinned: hashes (8 B each), errs, the Response table, then the status bytes
  const uint32_t m = (uint32_t)n;
  const size_t tab_words = resp_table_words(n_resp, rt);
  AV_HIP(e->dropin_host.reserve((size_t)m * 13 + tab_words * 4 + 64, avmem::Slack::kMiB, hipHostMallocDefault));
  auto* hhash = static_cast<int64_t*>(e->dropin_host.get());
  auto* herr = reinterpret_cast<uint32_t*>(hhash + m);
  auto* hoff = herr + m;
  auto* hstat = reinterpret_cast<int8_t*>(hoff + tab_words);
  fill_resp_table(e, n_resp, nodes, offsets, rt, hoff);
  std::vector<uint8_t> neutral_t(64, 0);
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
  // ---- device: hashes | errs | off | node | order | grp_off | packed | flag, pad | status bytes
  const size_t in_words = 3 * (size_t)m + tab_words;
  const size_t head_words = in_words + (size_t)m + 2 + ((size_t)m + 3) / 4;
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, head_words * 4 + 64, &buf));
  auto* dhash = static_cast<int64_t*>(buf);  // the allocation's start: 16-byte aligned
  auto* derr = reinterpret_cast<uint32_t*>(dhash + m);
  uint32_t* doff = derr + m;
  uint32_t* dpack = doff + tab_words;
  dpack += (in_words & 1u);  // 8-byte aligned (the kernel stores two packed votes at once)
  uint32_t* dflag = dpack + m;
  auto* dstat = reinterpret_cast<int8_t*>(dflag + 1);
  AV_HIP(hipMemcpyAsync(dhash, hhash, in_words * 4, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipMemsetAsync(dflag, 0, 4, e->stream));
  AV_HIP(hipMemsetAsync(dstat, 0xFF, (size_t)m, e->stream));
  AV_TRY(catalog_pack(e, dhash, derr, doff, (uint32_t)n_resp, m, dpack, dflag));
  uint32_t unordered = 1;
  AV_HIP(hipMemcpyAsync(&unordered, dflag, 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  const bool fast = !unordered && e->dropin_fast;
  uint32_t* grp = nullptr;
  if (!fast) {
    // the engine's scratch holds the batch: the grouping scratch is a buffer of its own, kept
    AV_HIP(e->cat_group.reserve(group_words(m) + 128 + (size_t)avk::group_votes_scratch_words(m) * 2,
                                avmem::Slack::kEighth));
    grp = e->cat_group;
  }
  return apply_packed_votes(e, rt, n_resp, dpack, doff, dstat, fast, grp, hstat, status_out);
}

int av_read_records(av_engine* e, int64_t n0, int64_t n1, int64_t t0, int64_t t1, uint32_t* out) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(out && n0 >= e->n0 && n0 <= n1 && n1 <= e->n1 && t0 >= e->t0 && t0 <= t1 && t1 <= e->t1,
           AV_ERR_INVALID_ARG, "range outside this engine's shard");
  const size_t n = (size_t)(n1 - n0) * (size_t)(t1 - t0);
  if (!n) return AV_OK;
  // the deferred forms (stale vote planes, pending count steps) are read
  // through, not written back: a read leaves the next round's fast paths on
  avk::RoundParams p = round_params(e, nullptr);
  p.vv = e->facts.v_stale ? 1u : 0u;
  p.klazy = e->facts.k_pend ? 1u : 0u;
  p.c_preset = e->facts.c_preset ? 1u : 0u;
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, n * 4, &buf));
  AV_HIP(avk::launch_read_records_virtual(p, (uint32_t)(n0 - e->n0), (uint32_t)(n1 - e->n0), (uint32_t)(t0 - e->t0),
                                          (uint32_t)(t1 - e->t0), static_cast<uint32_t*>(buf), e->stream));
  AV_HIP(hipMemcpyAsync(out, buf, n * 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  AV_PEER_CHECK(e);
  return AV_OK;
}

int av_write_records(av_engine* e, int64_t n0, int64_t n1, int64_t t0, int64_t t1, const uint32_t* in) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_TRY(peer_local_write_check(e));
  AV_CHECK(in && n0 >= e->n0 && n0 <= n1 && n1 <= e->n1 && t0 >= e->t0 && t0 <= t1 && t1 <= e->t1,
           AV_ERR_INVALID_ARG, "range outside this engine's shard");
  AV_TRY(materialize_votes(e));
  const size_t n = (size_t)(n1 - n0) * (size_t)(t1 - t0);
  if (!n) return AV_OK;
  e->facts.write_records();
  avmem::DevBuf<uint32_t> s;
  AV_HIP(s.alloc(n));
  AV_HIP(hipMemcpyAsync(s, in, n * 4, hipMemcpyHostToDevice, e->stream));
  AV_HIP(avk::launch_write_records(e->planes, e->BL, (uint32_t)(n0 - e->n0), (uint32_t)(n1 - e->n0),
                                   (uint32_t)(t0 - e->t0), (uint32_t)(t1 - e->t0), s, e->stream));
  AV_TRY(refresh_pref(e));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_is_accepted(av_engine* e, int64_t node, int64_t target, int32_t* out) {
  AV_CHECK(e && out, AV_ERR_INVALID_ARG, "null argument");
  *out = 0;
  if (!local_node(e, node) || !local_target(e, target)) return AV_OK;  // no record -> false
  uint32_t w = 0;
  AV_TRY(av_read_records(e, node, node + 1, target, target + 1, &w));
  if (((w >> 17) < (uint32_t)AV_FINALIZATION_SCORE)) *out = (int32_t)((w >> 16) & 1u);
  return AV_OK;
}

int av_get_confidence(av_engine* e, int64_t node, int64_t target, uint16_t* out) {
  AV_CHECK(e && out, AV_ERR_INVALID_ARG, "null argument");
  if (!local_node(e, node) || !local_target(e, target)) return fail(AV_ERR_NOT_FOUND, "VoteRecord not found");
  uint32_t w = 0;
  AV_TRY(av_read_records(e, node, node + 1, target, target + 1, &w));
  if ((w >> 17) >= (uint32_t)AV_FINALIZATION_SCORE) return fail(AV_ERR_NOT_FOUND, "VoteRecord not found");
  *out = (uint16_t)(w >> 17);
  return AV_OK;
}

int av_get_invs(av_engine* e, int64_t node, int64_t* out_targets, int64_t cap, int64_t* n_out) {
  AV_CHECK(e && n_out && (cap == 0 || out_targets), AV_ERR_INVALID_ARG, "null argument");
  *n_out = 0;
  AV_CHECK(local_node(e, node), AV_ERR_INVALID_ARG, "node not in this shard");
  std::vector<uint32_t> w((size_t)(e->t1 - e->t0));
  AV_TRY(av_read_records(e, node, node + 1, e->t0, e->t1, w.data()));
  int64_t cnt = 0;
  for (int64_t tl = 0; tl < (int64_t)w.size() && cnt < AV_MAX_ELEMENT_POLL; ++tl) {
    const bool live = (w[tl] >> 17) < (uint32_t)AV_FINALIZATION_SCORE;
    const bool valid = (e->valid_host[tl >> 5] >> (tl & 31)) & 1u;
    if (!live || !valid) continue;
    if (cnt < cap) out_targets[cnt] = e->t0 + tl;
    cnt++;
  }
  *n_out = cnt;
  AV_CHECK(cnt <= cap, AV_ERR_OVERFLOW, "cap too small (%lld needed)", (long long)cnt);
  return AV_OK;
}

// GetInvsForNextPoll for a node range (processor.go:144-170): counts, their device scan and the CSR
// fill enqueued back to back, the fill writing offsets and targets straight into host-mapped pinned
// staging (coalesced stores): one synchronization per call, then a host copy into the caller's arrays.
int av_get_invs_batch(av_engine* e, int64_t n0, int64_t n1, int64_t* offsets, int32_t* targets, int64_t cap,
                      int64_t* total) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(offsets && total && (cap == 0 || targets), AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(n0 >= e->n0 && n0 <= n1 && n1 <= e->n1, AV_ERR_INVALID_ARG, "node range outside this engine's shard");
  const uint32_t n = (uint32_t)(n1 - n0);
  *total = 0;
  offsets[0] = 0;
  if (!n) return AV_OK;
  // staging: offsets (n + 1 int64) then up to min(cap, the largest possible poll sets) int32 targets
  const uint64_t most = (uint64_t)n * (uint64_t)std::min<int64_t>(AV_MAX_ELEMENT_POLL, e->t1 - e->t0);
  const uint64_t keep = std::min<uint64_t>((uint64_t)std::max<int64_t>(cap, 0), most);
  const size_t hb = ((size_t)n + 1) * 8 + (size_t)keep * 4;
  AV_HIP(e->invs_host.reserve(hb, avmem::Slack::kExact, hipHostMallocMapped));
  void* dev_view = nullptr;
  AV_HIP(hipHostGetDevicePointer(&dev_view, e->invs_host, 0));
  auto* hoffs = static_cast<int64_t*>(e->invs_host.get());
  auto* doffs = static_cast<int64_t*>(dev_view);
  void* scratch = nullptr;
  AV_TRY(engine_scratch(e, (size_t)avk::poll_sets_scratch_words(n) * 8, &scratch));
  AV_HIP(avk::launch_poll_sets_batch(e->planes, e->valid, e->BL, (uint32_t)(n0 - e->n0), n, (uint32_t)e->t0, keep,
                                     static_cast<uint64_t*>(scratch), doffs, reinterpret_cast<int32_t*>(doffs + n + 1),
                                     e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  *total = hoffs[n];
  std::memcpy(offsets, hoffs, ((size_t)n + 1) * 8);
  AV_CHECK(*total <= cap, AV_ERR_OVERFLOW, "cap too small (%lld needed)", (long long)*total);
  if (*total) std::memcpy(targets, reinterpret_cast<const int32_t*>(hoffs + n + 1), (size_t)*total * 4);
  return AV_OK;
}

int av_set_polling(av_engine* e, int64_t node, int32_t polls) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_CHECK(local_node(e, node), AV_ERR_INVALID_ARG, "node %lld not in this shard", (long long)node);
  AV_CHECK(e->peer_world <= 1, AV_ERR_UNSUPPORTED, "av_set_polling on a peer-push engine");
  if (e->nopoll_host.empty()) {
    e->nopoll_host.assign((e->NL + 31) / 32, 0u);
    AV_HIP(e->nopoll.alloc(e->nopoll_host.size()));
  }
  const uint32_t nl = (uint32_t)(node - e->n0);
  uint32_t& w = e->nopoll_host[nl >> 5];
  w = polls ? (w & ~(1u << (nl & 31))) : (w | (1u << (nl & 31)));
  AV_TRY(materialize_votes(e));  // rounds of non-polling networks run the first-generation kernel
  AV_HIP(hipMemcpyAsync(e->nopoll, e->nopoll_host.data(), e->nopoll_host.size() * 4, hipMemcpyHostToDevice,
                        e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  e->any_nopoll = false;
  for (uint32_t v : e->nopoll_host) e->any_nopoll |= v != 0;
  return AV_OK;
}

// Rule R5. A Response that does not arrive is a RegisterVotes call that returns before it reads a
// vote (processor.go:66-76, AvalancheRequestTimeout avalanche.go:19-21): with that check disabled,
// a call that never happens (AV_LOSS_SKIP); a neutral one shifts consider = 0 (vote.go:55-56).
int av_set_loss(av_engine* e, uint32_t loss_threshold, int32_t mode) {
  AV_ENTER(e);
  AV_CHECK(mode == AV_LOSS_SKIP || mode == AV_LOSS_NEUTRAL, AV_ERR_INVALID_ARG, "bad loss mode");
  AV_CHECK(loss_threshold == 0 || e->peer_world <= 1, AV_ERR_UNSUPPORTED, "av_set_loss on a peer-push engine");
  if (loss_threshold && !e->lost) AV_HIP(e->lost.alloc_zeroed(avk::kLogShards, e->stream));
  e->loss_threshold = loss_threshold;
  e->loss_neutral = mode == AV_LOSS_NEUTRAL;
  return AV_OK;
}

int av_set_responding(av_engine* e, const int64_t* nodes, int64_t n, int32_t responds) {
  AV_ENTER(e);
  AV_CHECK(n >= 0 && (nodes || n == 0), AV_ERR_INVALID_ARG, "null argument");
  for (int64_t i = 0; i < n; ++i)
    AV_CHECK(nodes[i] >= 0 && nodes[i] < e->N, AV_ERR_INVALID_ARG, "node %lld outside the network", (long long)nodes[i]);
  AV_CHECK(responds || n == 0 || e->peer_world <= 1, AV_ERR_UNSUPPORTED,
           "av_set_responding(0) on a peer-push engine");
  if (n == 0 || (responds && !e->any_down)) return AV_OK;  // every node responds already
  const size_t words = (size_t)((e->N + 31) / 32);
  if (e->responding_host.empty()) {
    e->responding_host.assign(words, ~0u);
    AV_HIP(e->responding.alloc(words));
  }
  if (!e->lost) AV_HIP(e->lost.alloc_zeroed(avk::kLogShards, e->stream));
  for (int64_t i = 0; i < n; ++i) {
    uint32_t& w = e->responding_host[(size_t)(nodes[i] >> 5)];
    const uint32_t bit = 1u << (nodes[i] & 31);
    w = responds ? (w | bit) : (w & ~bit);
  }
  AV_HIP(hipMemcpyAsync(e->responding, e->responding_host.data(), words * 4, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  e->any_down = false;
  for (int64_t node = 0; node < e->N && !e->any_down; node += 32) {
    const uint32_t all = e->N - node >= 32 ? ~0u : (1u << (e->N - node)) - 1u;
    e->any_down = (e->responding_host[(size_t)(node >> 5)] & all) != all;
  }
  return AV_OK;
}

// The device's own answer (a parity dump, as av_sample_peers is of R1's draw): 1 = the Response of
// that slot is lost, by the draw or because its peer does not respond.
int av_sample_lost(av_engine* e, int64_t round, int64_t n0, int64_t n1, uint8_t* out) {
  AV_ENTER(e);
  AV_CHECK(out && n0 >= 0 && n0 <= n1 && n1 <= e->N && round >= 0, AV_ERR_INVALID_ARG, "bad range");
  const size_t n = (size_t)(n1 - n0) * e->k;
  if (!n) return AV_OK;
  avmem::DevBuf<uint8_t> s;
  AV_HIP(s.alloc(n));
  AV_HIP(avk::launch_sample_lost(e->cfg.seed, (uint32_t)e->N, (uint32_t)n0, (uint32_t)n1, (uint32_t)round, e->k,
                                 e->cfg.peer_mode, e->loss_threshold, e->any_down ? e->responding.get() : nullptr, s,
                                 e->stream));
  AV_HIP(hipMemcpyAsync(out, s, n, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_lost_responses(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  *out = 0;
  return e->lost ? sum_shards(e, e->lost, out) : AV_OK;
}

int av_applied_votes(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  return sum_shards(e, e->applied, out);
}

int av_finalized_count(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  return sum_shards(e, e->finalized, out);
}

int av_live_records(av_engine* e, int32_t honest_only, int64_t* out) {
  AV_TRY(counter_query(e, out));
  AV_HIP(hipMemsetAsync(e->scratch_count, 0, 8, e->stream));
  AV_HIP(avk::launch_count_live(e->planes, e->valid, e->byz, (uint32_t)e->n0, e->BL, e->L, honest_only,
                                e->scratch_count, e->stream));
  unsigned long long v = 0;
  AV_HIP(hipMemcpyAsync(&v, e->scratch_count, 8, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  *out = (int64_t)v;
  return AV_OK;
}

// IsAccepted / GetConfidence over every Processor (processor.go:125-140) and the example's stop test
// (main.go:143-162: a node is done when it holds no live record), tallied on the device: one pass
// over the A and K planes (census.hip), read through the deferred count forms like av_read_records
// and, like it, leaving them in place.
int av_census(av_engine* e, int64_t n0, int64_t n1, int32_t honest_only, const av_census_out* out) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(out && (out->target_classes || out->target_count_sum || out->node_classes || out->count_hist),
           AV_ERR_INVALID_ARG, "no census output requested");
  AV_CHECK(n0 >= e->n0 && n0 <= n1 && n1 <= e->n1, AV_ERR_INVALID_ARG, "range outside this engine's shard");
  const size_t tn = (size_t)(e->t1 - e->t0), nn = (size_t)(n1 - n0);
  if (out->target_classes) std::fill(out->target_classes, out->target_classes + tn * AV_CENSUS_CLASSES, (int64_t)0);
  if (out->target_count_sum) std::fill(out->target_count_sum, out->target_count_sum + tn, (int64_t)0);
  if (out->node_classes) std::fill(out->node_classes, out->node_classes + nn * AV_CENSUS_CLASSES, (int32_t)0);
  if (out->count_hist) std::fill(out->count_hist, out->count_hist + 256, (int64_t)0);
  if (!nn || !tn) return AV_OK;
  // device sums: [tn][3] classes (live rejected, live accepted, absent accepted), [tn] count sums,
  // [256] histogram, the nodes counted, one pad word; then the node rows (16-byte aligned)
  const size_t head = tn * 4 + 256 + 2, head_bytes = head * 8;
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, head_bytes + (out->node_classes ? nn * 16 : 0), &buf));
  AV_HIP(hipMemsetAsync(buf, 0, head_bytes + (out->node_classes ? nn * 16 : 0), e->stream));
  auto* d = static_cast<unsigned long long*>(buf);
  avk::CensusParams p{};
  p.planes = e->planes;
  p.kpend = e->facts.k_pend ? e->kpend : nullptr;
  p.valid = e->valid;
  p.byz = e->byz;
  p.tcls = out->target_classes ? d : nullptr;
  p.tsum = out->target_count_sum ? d + tn * 3 : nullptr;
  p.hist = out->count_hist ? d + tn * 4 : nullptr;
  p.counted = d + tn * 4 + 256;
  p.ncls = out->node_classes ? reinterpret_cast<int32_t*>(d + head) : nullptr;
  p.BL = e->BL;
  p.tn = (uint32_t)tn;
  p.n0 = (uint32_t)e->n0;
  p.honest_only = honest_only ? 1u : 0u;
  AV_HIP(avk::launch_census(p, (uint32_t)(n0 - e->n0), (uint32_t)(n1 - e->n0), e->census_blocks, e->stream));
  std::vector<unsigned long long> h(head);
  AV_HIP(hipMemcpyAsync(h.data(), d, head_bytes, hipMemcpyDeviceToHost, e->stream));
  if (out->node_classes)
    AV_HIP(hipMemcpyAsync(out->node_classes, d + head, nn * 16, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  AV_PEER_CHECK(e);
  if (out->target_classes) {
    const int64_t counted = (int64_t)h[tn * 4 + 256];
    for (size_t t = 0; t < tn; ++t) {
      int64_t* row = out->target_classes + t * AV_CENSUS_CLASSES;
      row[AV_CENSUS_LIVE_REJECTED] = (int64_t)h[t * 3];
      row[AV_CENSUS_LIVE_ACCEPTED] = (int64_t)h[t * 3 + 1];
      row[AV_CENSUS_ABSENT_ACCEPTED] = (int64_t)h[t * 3 + 2];
      // every counted node has exactly one class for the target
      row[AV_CENSUS_ABSENT_REJECTED] = counted - row[0] - row[1] - row[3];
    }
  }
  if (out->target_count_sum)
    for (size_t t = 0; t < tn; ++t) out->target_count_sum[t] = (int64_t)h[tn * 3 + t];
  if (out->count_hist)
    for (size_t i = 0; i < 256; ++i) out->count_hist[i] = (int64_t)h[tn * 4 + i];
  return AV_OK;
}

int av_alg_bytes(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  return sum_shards(e, e->bytes, out);
}

int av_alg_bytes_reread(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  return sum_shards(e, e->bytes + avk::kLogShards, out);
}

int av_changed_words(av_engine* e, int64_t* words, int64_t* segments) {
  AV_TRY(counter_query(e, words));
  AV_TRY(sum_shards(e, e->changed, words));
  return segments ? sum_shards(e, e->changed + avk::kLogShards, segments) : AV_OK;
}

int av_net_quiet_rounds(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  uint32_t v = 0;
  AV_HIP(hipMemcpyAsync(&v, e->nq + 2, 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  *out = (int64_t)v;
  return AV_OK;
}

int av_read_pref(av_engine* e, int64_t n0, int64_t n1, int64_t t0, int64_t t1, uint8_t* out) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(out && n0 >= 0 && n0 <= n1 && n1 <= e->N && t0 >= e->t0 && t0 <= t1 && t1 <= e->t1,
           AV_ERR_INVALID_ARG, "bad range");
  const size_t rows = (size_t)(n1 - n0);
  std::vector<uint32_t> w(rows * e->BL);
  if (rows) AV_TRY(av_read_pref_words(e, n0, n1, w.data()));
  const int64_t W = t1 - t0;
  for (size_t r = 0; r < rows; ++r)
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t tl = t - e->t0;
      out[r * W + (t - t0)] = (uint8_t)((w[r * e->BL + (tl >> 5)] >> (tl & 31)) & 1u);
    }
  return AV_OK;
}

int av_read_pref_words(av_engine* e, int64_t n0, int64_t n1, uint32_t* out) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(out && n0 >= 0 && n0 <= n1 && n1 <= e->N, AV_ERR_INVALID_ARG, "bad range");
  const size_t words = (size_t)(n1 - n0) * e->BL;
  if (!words) return AV_OK;
  AV_HIP(hipMemcpy2DAsync(out, (size_t)e->BL * 4, e->pref[e->cur] + (size_t)n0 * e->PS, (size_t)e->PS * 4,
                          (size_t)e->BL * 4, (size_t)(n1 - n0), hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_sample_peers(av_engine* e, int64_t round, int64_t n0, int64_t n1, int32_t* out) {
  AV_ENTER(e);
  AV_CHECK(out && n0 >= 0 && n0 <= n1 && n1 <= e->N && round >= 0, AV_ERR_INVALID_ARG, "bad range");
  const size_t n = (size_t)(n1 - n0) * e->k;
  if (!n) return AV_OK;
  avmem::DevBuf<uint32_t> s;
  AV_HIP(s.alloc(n));
  AV_HIP(avk::launch_sample_peers(e->cfg.seed, (uint32_t)e->N, (uint32_t)n0, (uint32_t)n1, (uint32_t)round, e->k,
                                  e->cfg.peer_mode, s, e->stream));
  AV_HIP(hipMemcpyAsync(out, s, n * 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_pushed_words(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  return sum_shards(e, e->changed + 2 * avk::kLogShards, out);
}

}  // extern "C"
