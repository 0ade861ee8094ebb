// libavhip.so: record I/O outside a round. Validity, reads and writes of records, preferences and
// poll sets, polling, loss and responding nodes, peer lists, the census and the counter queries. The drop-in
// write batches (added targets, votes) are engine_dropin.cpp's.
#include <cstring>
#include <utility>

#include "engine.h"
#include "peer_list_check.h"

using namespace aveng;

namespace {

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
  if (e->listed) {  // R6: the lost mask of the listed draw, 0 in empty slots
    AV_CHECK(n0 >= e->n0 && n1 <= e->n1, AV_ERR_INVALID_ARG, "an engine with peer lists draws for its own nodes only");
    AV_HIP(avk::launch_sample_listed(e->cfg.seed, (uint32_t)e->n0, (uint32_t)(n0 - e->n0), (uint32_t)(n1 - e->n0),
                                     (uint32_t)round, e->k, e->list_offsets, e->list_peers, e->loss_threshold,
                                     e->any_down ? e->responding.get() : nullptr, nullptr, s, e->stream));
  } else {
    AV_HIP(avk::launch_sample_lost(e->cfg.seed, (uint32_t)e->N, (uint32_t)n0, (uint32_t)n1, (uint32_t)round, e->k,
                                   e->cfg.peer_mode, e->loss_threshold, e->any_down ? e->responding.get() : nullptr, s,
                                   e->stream));
  }
  AV_HIP(hipMemcpyAsync(out, s, n, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_lost_responses(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  *out = 0;
  return e->lost ? sum_shards(e, e->lost, out) : AV_OK;
}

// Rule R6: the Connman of every local node (net.go:11-31), from whose NodesIDs() the reference picks
// whom to query (processor.go:173-182). Validated on the host (peer_list_check.h: the device indexes
// by what passes there, with no check of its own), converted to 32-bit and uploaded into fresh
// buffers, which replace the engine's only once everything has succeeded and the stream has drained.
int av_set_peer_lists(av_engine* e, const int64_t* offsets, const int64_t* peers) {
  AV_ENTER(e);
  if (!offsets) {  // back to the whole network
    if (e->listed || e->list_offsets) {
      // rounds enqueued under the lists read them: drained before the buffers are freed
      AV_HIP(hipStreamSynchronize(e->stream));
      e->list_offsets.reset();
      e->list_peers.reset();
    }
    e->listed = false;
    return AV_OK;
  }
  AV_CHECK(e->peer_world <= 1, AV_ERR_UNSUPPORTED, "av_set_peer_lists on a peer-push engine");
  AV_CHECK(e->cfg.peer_mode != AV_PEERS_ROUND_ROBIN, AV_ERR_UNSUPPORTED,
           "av_set_peer_lists on an engine created with AV_PEERS_ROUND_ROBIN");
  std::vector<uint32_t> off32, list32;
  int64_t bad = -1;
  const avk::PeerListError pe = avk::check_peer_lists(e->N, e->n0, (int64_t)e->NL, offsets, peers, &off32, &list32, &bad);
  AV_CHECK(pe == avk::PeerListError::Ok, AV_ERR_INVALID_ARG, "av_set_peer_lists: %s (local node %lld)",
           avk::peer_list_error_text(pe), (long long)bad);
  avmem::DevBuf<uint32_t> d_off, d_list;
  AV_HIP(d_off.alloc(off32.size()));
  AV_HIP(d_list.alloc(list32.size()));
  if (!e->lost) AV_HIP(e->lost.alloc_zeroed(avk::kLogShards, e->stream));
  if (!e->unsent) AV_HIP(e->unsent.alloc_zeroed(avk::kLogShards, e->stream));
  AV_HIP(hipMemcpyAsync(d_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, e->stream));
  if (!list32.empty())
    AV_HIP(hipMemcpyAsync(d_list, list32.data(), list32.size() * 4, hipMemcpyHostToDevice, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));  // (the host vectors go; rounds enqueued earlier are done with the old lists)
  e->list_offsets = std::move(d_off);
  e->list_peers = std::move(d_list);
  e->listed = true;
  return AV_OK;
}

int av_unsent_polls(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  *out = 0;
  return e->unsent ? sum_shards(e, e->unsent, out) : AV_OK;
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
  avlay::Carver size;
  avlay::census_sums(size, tn, out->node_classes ? nn : 0);
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, size.bytes(), &buf));
  AV_HIP(hipMemsetAsync(buf, 0, size.bytes(), e->stream));
  avlay::Carver dev(buf);
  const avlay::CensusSums d = avlay::census_sums(dev, tn, out->node_classes ? nn : 0);
  avk::CensusParams p{};
  p.planes = e->planes;
  p.kpend = e->facts.k_pend ? e->kpend : nullptr;
  p.valid = e->valid;
  p.byz = e->byz;
  p.tcls = out->target_classes ? d.tcls : nullptr;
  p.tsum = out->target_count_sum ? d.tsum : nullptr;
  p.hist = out->count_hist ? d.hist : nullptr;
  p.counted = d.counted;
  p.ncls = d.ncls;
  p.BL = e->BL;
  p.tn = (uint32_t)tn;
  p.n0 = (uint32_t)e->n0;
  p.honest_only = honest_only ? 1u : 0u;
  AV_HIP(avk::launch_census(p, (uint32_t)(n0 - e->n0), (uint32_t)(n1 - e->n0), e->census_blocks, e->stream));
  // the host's copy of the sums, by the same layout
  std::vector<unsigned long long> hbuf(d.head_bytes / 8);
  avlay::Carver host(hbuf.data());
  const avlay::CensusSums h = avlay::census_sums(host, tn, 0);
  AV_HIP(hipMemcpyAsync(hbuf.data(), buf, d.head_bytes, hipMemcpyDeviceToHost, e->stream));
  if (out->node_classes)
    AV_HIP(hipMemcpyAsync(out->node_classes, d.ncls, nn * 16, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  AV_PEER_CHECK(e);
  if (out->target_classes) {
    const int64_t counted = (int64_t)*h.counted;
    for (size_t t = 0; t < tn; ++t) {
      int64_t* row = out->target_classes + t * AV_CENSUS_CLASSES;
      row[AV_CENSUS_LIVE_REJECTED] = (int64_t)h.tcls[t * 3];
      row[AV_CENSUS_LIVE_ACCEPTED] = (int64_t)h.tcls[t * 3 + 1];
      row[AV_CENSUS_ABSENT_ACCEPTED] = (int64_t)h.tcls[t * 3 + 2];
      // every counted node has exactly one class for the target
      row[AV_CENSUS_ABSENT_REJECTED] = counted - row[0] - row[1] - row[3];
    }
  }
  if (out->target_count_sum)
    for (size_t t = 0; t < tn; ++t) out->target_count_sum[t] = (int64_t)h.tsum[t];
  if (out->count_hist)
    for (size_t i = 0; i < 256; ++i) out->count_hist[i] = (int64_t)h.hist[i];
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
  if (e->listed) {  // R6: the listed draw, AV_NO_PEER in empty slots
    AV_CHECK(n0 >= e->n0 && n1 <= e->n1, AV_ERR_INVALID_ARG, "an engine with peer lists draws for its own nodes only");
    AV_HIP(avk::launch_sample_listed(e->cfg.seed, (uint32_t)e->n0, (uint32_t)(n0 - e->n0), (uint32_t)(n1 - e->n0),
                                     (uint32_t)round, e->k, e->list_offsets, e->list_peers, 0u, nullptr,
                                     reinterpret_cast<int32_t*>(s.get()), nullptr, e->stream));
  } else {
    AV_HIP(avk::launch_sample_peers(e->cfg.seed, (uint32_t)e->N, (uint32_t)n0, (uint32_t)n1, (uint32_t)round, e->k,
                                    e->cfg.peer_mode, s, e->stream));
  }
  AV_HIP(hipMemcpyAsync(out, s, n * 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_pushed_words(av_engine* e, int64_t* out) {
  AV_TRY(counter_query(e, out));
  return sum_shards(e, e->changed + 2 * avk::kLogShards, out);
}

}  // extern "C"
