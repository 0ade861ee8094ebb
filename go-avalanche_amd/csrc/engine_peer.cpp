// libavhip.so: the exchange between the ranks of a node-sharded network. The peer push
// and its barrier, the need-masked exchange, and the calls that set an exchange up: RCCL
// (av_comm_*), IPC peer push (av_peer_handles / av_peer_init) and the in-process serial group.
#include <cstring>
#include <memory>

#include "engine.h"

using namespace aveng;

namespace {

// ---- need-masked exchange (kernels.h RoundParams::need / stale) ----
constexpr size_t kNeedinOff = 4096;  // byte offset of needin in the exported arrival allocation

size_t needin_words(const av_engine* e, int world) {
  return (size_t)2 * (size_t)world * avk::kNeedWin * ((e->NL + 31) / 32);
}

// a row's 32-word segments never straddle a wave: BL a power of two <= 32 (a node's lanes inside one
// tile) or a multiple of 32 (32-aligned segments inside 64-aligned tiles)
bool mask_layout_ok(const av_engine* e) {
  return (e->BL <= 32 && (e->BL & (e->BL - 1)) == 0) || e->BL % 32 == 0;
}

// Window w = push rounds [w W, w W + W): the rows this rank's nodes draw in rounds w W + 1 .. w W + W
// (R1's sampling), pushed to their owners; enqueued before a barrier, combined after it.
int need_draw(av_engine* e, int64_t w, hipStream_t s) {
  const uint32_t W = avk::kNeedWin;
  AV_HIP(hipMemsetAsync(e->need_mine, 0, (size_t)W * e->N, s));
  AV_HIP(avk::launch_need_draw(e->cfg.seed, (uint32_t)e->N, (uint32_t)e->n0, e->NL, (uint32_t)(w * W + 1), W, e->k,
                               e->cfg.peer_mode, e->need_mine, s));
  return AV_OK;
}

// After the exchange's pointers are set (own needin allocated, peer_needin filled): buffers of the
// masked form, every replica identical (nothing withheld).
int mask_setup(av_engine* e) {
  // node shards of an exchange: runs of up to 16 tiles per wave (the longest the shared draw holds,
  // BL >= 16) unless set: the single-GPU rule (>= 15000 waves) gave 4 at 8 ranks of C4, whose settled
  // rounds then paid 4x the per-wave set-up (tools/group_model.py)
  if (!e->tiles_per_wave && !e->sweep_blocks_explicit && e->BL >= 16 && e->peer_world >= 4) {
    e->tiles_per_wave = 16;
    e->sweep_blocks = default_sweep_blocks(e, false);
    AV_TRY(relayout_log_if_empty(e));  // fewer writer waves
  }
  e->masked = e->peer_mask && e->peer_world >= 2 && e->peer_world <= 9 && mask_layout_ok(e) && e->needin;
  if (!e->masked) return AV_OK;
  e->segs = (e->BL + 31) / 32;
  AV_HIP(e->need_mine.alloc((size_t)avk::kNeedWin * e->N));
  AV_HIP(e->needmask.alloc((size_t)avk::kNeedWin * e->NL));
  AV_HIP(e->stale.alloc_zeroed((size_t)3 * e->NL * e->segs, e->stream));
  AV_HIP(e->need_stream.create(hipStreamNonBlocking));
  AV_HIP(e->need_free.create(hipEventDisableTiming));
  AV_HIP(e->need_drawn.create(hipEventDisableTiming));
  e->need_ready = e->need_pushed = e->need_drawn_w = -1;
  return AV_OK;
}

}  // namespace

namespace aveng {

// A serial peer group's members store into each other's buffers: once any member was destroyed (its
// buffers freed), no member may push or exchange need masks any more.
int group_alive(const av_engine* e) {
  if (e->group)
    for (const av_engine* m : e->group->members) AV_CHECK(m, AV_ERR_UNSUPPORTED, "peer group: a rank was destroyed");
  return AV_OK;
}

// Peer-push exchange: copy this rank's rows of snapshot buffer `b` into every
// peer replica (a full resynchronisation of those rows).
int push_own_rows(av_engine* e, int b) {
  AV_TRY(group_alive(e));
  avk::PeerPtrs dst{};
  uint32_t n = 0;
  for (int r = 0; r < e->peer_world; ++r)
    if (r != e->peer_rank) dst.p[n++] = e->peer_pref[b][r];
  const uint64_t w0 = (uint64_t)e->n0 * e->PS, w1 = w0 + (uint64_t)e->NL * e->PS;
  AV_HIP(avk::launch_push_rows(e->pref[b], dst, n, w0, w1, e->stream));
  return AV_OK;
}

// Barrier across the peer ranks, on the engine stream (kernels.h).
// slot_buf >= 0: the barrier kernel first copies this rank's uniform-rows mismatch slot of snapshot
// buffer slot_buf into every peer's replica (the round kernel writes only its own copy, RoundParams::
// uni_post). A serial group has no barrier: the copy alone runs.
int peer_barrier(av_engine* e, int slot_buf) {
  const uint32_t* slot = nullptr;
  avk::PeerPtrs sd{};
  if (slot_buf >= 0 && e->peer_world > 1) {
    slot = e->pref[slot_buf] + e->uni_off + e->peer_rank;
    for (int r = 0; r < e->peer_world; ++r) sd.p[r] = e->peer_pref[slot_buf][r] + e->uni_off + e->peer_rank;
  }
  if (e->group) {  // serial group: every rank's kernels run in one stream's order
    if (slot)
      AV_HIP(avk::launch_peer_barrier(e->peer_arrive, (uint32_t)e->peer_world, (uint32_t)e->peer_rank, 0u, nullptr,
                                      0u, e->stream, slot, sd, 0u));
    return AV_OK;
  }
  if (!e->barrier_ticks) AV_HIP(avk::peer_timeout_ticks(e->cfg.device, e->barrier_timeout_ms, &e->barrier_ticks));
  AV_HIP(avk::launch_peer_barrier(e->peer_arrive, (uint32_t)std::max(1, e->peer_world), (uint32_t)e->peer_rank,
                                  ++e->barrier_seq, e->barrier_err, e->barrier_ticks, e->stream, slot, sd, 1u));
  return AV_OK;
}

// Every replica of snapshot buffer b was just given this rank's rows whole: nothing withheld.
int stale_clear(av_engine* e, int b) {
  if (!e->masked) return AV_OK;
  const size_t n = (size_t)e->NL * e->segs;
  AV_HIP(hipMemsetAsync(e->stale + (size_t)b * n, 0, n, e->stream));
  return AV_OK;
}

int need_gen(av_engine* e, int64_t w) {
  if (!e->masked || e->need_pushed == w) return AV_OK;
  AV_TRY(group_alive(e));
  if (e->need_drawn_w == w) {
    AV_HIP(hipStreamWaitEvent(e->stream, e->need_drawn, 0));  // drawn ahead on the side stream
  } else {
    AV_TRY(need_draw(e, w, e->stream));
  }
  AV_HIP(avk::launch_need_push(e->need_mine, (uint32_t)e->N, e->NL, avk::kNeedWin, (uint32_t)e->peer_world,
                               (uint32_t)e->peer_rank, (uint32_t)(w & 1), e->peer_needin, e->stream));
  AV_HIP(hipEventRecord(e->need_free, e->stream));
  e->need_pushed = w;
  e->need_drawn_w = -1;
  return AV_OK;
}

// Window w + 1's rows drawn on the side stream while window w's rounds run (after window w's push
// released need_mine); need_gen at the end of window w waits for it.
// (not in a serial peer group: there every rank's side stream would run beside the other ranks'
// rounds on the one device, which a rank of a real run never sees; the group draws inline)
int need_draw_ahead(av_engine* e, int64_t w) {
  if (!e->masked || e->group || e->need_drawn_w == w || e->need_pushed >= w) return AV_OK;
  AV_HIP(hipStreamWaitEvent(e->need_stream, e->need_free, 0));
  AV_TRY(need_draw(e, w, e->need_stream));
  AV_HIP(hipEventRecord(e->need_drawn, e->need_stream));
  e->need_drawn_w = w;
  return AV_OK;
}

// After the barrier that ordered every rank's need_gen of window w: the per-row peer masks.
int need_combine(av_engine* e, int64_t w) {
  if (!e->masked || e->need_ready == w || e->need_pushed != w) return AV_OK;
  AV_TRY(ref_pick(e));  // the reference row (uniform rows) is read by every rank
  const uint32_t ref_local =
      e->ref_node >= e->n0 && e->ref_node < e->n1 ? (uint32_t)(e->ref_node - e->n0) : 0xFFFFFFFFu;
  AV_HIP(avk::launch_need_combine(e->needin, (uint32_t)e->peer_world, (uint32_t)e->peer_rank, (uint32_t)(w & 1),
                                  avk::kNeedWin, e->NL, ref_local, e->needmask, e->stream));
  e->need_ready = w;
  return AV_OK;
}

// A peer barrier that timed out (a rank stopped taking part) leaves the
// ranks' snapshot replicas unordered: every later round and every result of
// this engine is refused (sticky), AV_ERR_PEER.
int peer_failed(av_engine* e) {
  if (e->peer_world > 1 && !e->failed && e->barrier_err_host && *e->barrier_err_host) e->failed = true;
  if (e->failed)
    return fail(AV_ERR_PEER, "peer barrier timed out (a rank stopped taking part in the rounds): the exchange is "
                             "broken, results of this engine are invalid");
  return AV_OK;
}

// The arrival slots of the peer barrier (one per rank, fine-grained when peers store into them over
// xGMI) and the barrier's timeout flag in pinned host memory (the barrier kernel stores it with
// system scope, so the host sees it without synchronizing the stream; av_run_rounds refuses to
// enqueue once it is set). Zeroed before any peer can see them: the exchange of handles orders the two.
// The same allocation carries, at kNeedinOff, the table the peers' need_push stores into (sized for
// the world of equal node shards this engine's shard implies, N / NL).
int alloc_arrival(av_engine* e) {
  const int world = e->N % e->NL == 0 && e->N / e->NL <= avk::kMaxPeers + 1 ? (int)(e->N / e->NL) : 1;
  const size_t bytes = (kNeedinOff + needin_words(e, world) * 4 + (2u << 20) - 1) / (2u << 20) * (2u << 20);
  if (e->peer_fine)
    AV_HIP(e->arrive.alloc_flags(bytes / 4, hipDeviceMallocFinegrained));
  else
    AV_HIP(e->arrive.alloc(bytes / 4));
  AV_HIP(e->barrier_err_host.alloc(16, hipHostMallocMapped | hipHostMallocCoherent));
  *e->barrier_err_host = 0u;
  void* dp = nullptr;
  AV_HIP(hipHostGetDevicePointer(&dp, const_cast<uint32_t*>(e->barrier_err_host.get()), 0));
  e->barrier_err = static_cast<uint32_t*>(dp);
  AV_HIP(hipMemset(e->arrive, 0, (size_t)(avk::kMaxPeers + 1) * 4));
  AV_HIP(hipDeviceSynchronize());
  return AV_OK;
}

// The three snapshot buffers moved into memory of another kind (hipExtMallocWithFlags), contents kept;
// the engine's enqueued work finishes first.
int realloc_pref(av_engine* e, unsigned flags) {
  AV_HIP(hipStreamSynchronize(e->stream));
  for (auto& pref : e->pref) {
    avmem::DevBuf<uint32_t> nb;
    AV_HIP(nb.alloc_flags(e->pref_alloc_words, flags));
    AV_HIP(hipMemcpy(nb, pref, e->pref_alloc_words * 4, hipMemcpyDeviceToDevice));
    pref = std::move(nb);
  }
  return AV_OK;
}

}  // namespace aveng

namespace {

// What every exchange asks of a node-sharded engine: rank's shard of world equal ones, all targets.
int shard_checks(const av_engine* e, int world, int rank) {
  AV_CHECK(e->N % world == 0 && (int64_t)e->NL * world == e->N && e->n0 == (int64_t)rank * e->NL,
           AV_ERR_UNSUPPORTED, "node shards must be equal, contiguous and rank-ordered (N %% world == 0)");
  AV_CHECK(e->t0 == 0 && e->t1 == e->M, AV_ERR_UNSUPPORTED, "node sharding needs the full target range");
  return AV_OK;
}

// push_tbl from peer_pref: per snapshot buffer, the replicas of the world's other ranks in rank order.
int upload_push_tbl(av_engine* e, int world, int rank) {
  uint32_t* tbl[3][avk::kMaxPeers] = {};
  for (int b = 0; b < 3; ++b) {
    int n = 0;
    for (int r = 0; r < world; ++r)
      if (r != rank) tbl[b][n++] = e->peer_pref[b][r];
  }
  AV_HIP(e->push_tbl.alloc((size_t)3 * avk::kMaxPeers));
  AV_HIP(hipMemcpy(e->push_tbl, tbl, sizeof(tbl), hipMemcpyHostToDevice));
  return AV_OK;
}

}  // namespace

extern "C" {

int av_comm_unique_id(uint8_t out[128]) {
  AV_CHECK(out, AV_ERR_INVALID_ARG, "null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  AV_CHECK(r == ncclSuccess, AV_ERR_RCCL, "ncclGetUniqueId: %s", ncclGetErrorString(r));
  std::memcpy(out, &id, 128);
  return AV_OK;
}

int av_comm_init(av_engine* e, int32_t world, int32_t rank, const uint8_t id[128]) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_CHECK(id && world >= 1 && rank >= 0 && rank < world, AV_ERR_INVALID_ARG, "bad world/rank");
  AV_TRY(shard_checks(e, world, rank));
  ncclUniqueId uid;
  std::memcpy(&uid, id, 128);
  ncclResult_t r = ncclCommInitRank(&e->comm, world, uid, rank);
  AV_CHECK(r == ncclSuccess, AV_ERR_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
  // make every rank's initial preference rows visible everywhere
  const size_t count = (size_t)e->NL * e->PS;
  uint32_t* cur = e->pref[e->cur];
  r = ncclAllGather(cur + (size_t)e->n0 * e->PS, cur, count, ncclUint32, e->comm, e->stream);
  AV_CHECK(r == ncclSuccess, AV_ERR_RCCL, "ncclAllGather: %s", ncclGetErrorString(r));
  AV_HIP(hipStreamSynchronize(e->stream));
  return AV_OK;
}

int av_peer_handles(av_engine* e, uint8_t out[AV_PEER_HANDLE_BYTES]) {
  AV_ENTER(e);
  AV_CHECK(out, AV_ERR_INVALID_ARG, "null argument");
  static_assert(sizeof(hipIpcMemHandle_t) * 4 + 64 == AV_PEER_HANDLE_BYTES, "peer handle blob size");
  AV_CHECK(!e->solo_used, AV_ERR_UNSUPPORTED,
           "diagnostics option solo_barrier was used on this engine: it cannot join a peer exchange");
  if (!e->arrive) {  // zeroed before any peer can see it: the exchange of handles orders the two
    // Snapshot buffers that peers store into over xGMI are fine-grained: this
    // device's L2 keeps such lines only within a kernel (the system-scope
    // acquire at every kernel start drops them), so a round never reads a
    // stale L2 copy of a row a peer pushed during the previous round. Coarse-
    // grained memory would let a line read two rounds earlier (the 3-deep
    // rotation) survive in L2. Option "peer_fine" 0: keep the
    // coarse-grained buffers (A/B only).
    if (e->peer_fine) AV_TRY(realloc_pref(e, hipDeviceMallocFinegrained));
    AV_TRY(alloc_arrival(e));
  }
  void* bufs[4] = {e->pref[0], e->pref[1], e->pref[2], e->arrive};
  for (int i = 0; i < 4; ++i) {
    hipIpcMemHandle_t h;
    AV_HIP(hipIpcGetMemHandle(&h, bufs[i]));
    std::memcpy(out + i * sizeof(h), &h, sizeof(h));
  }
  // the device's PCI bus id: peers check that they can reach it (av_peer_init)
  char bus[64] = {};
  AV_HIP(hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, e->cfg.device));
  std::memcpy(out + 4 * sizeof(hipIpcMemHandle_t), bus, 64);
  return AV_OK;
}

int av_peer_init(av_engine* e, int32_t world, int32_t rank, const uint8_t* handles) {
  if (e) e->facts.snapshot_written();
  AV_ENTER(e);
  AV_CHECK(handles && world >= 1 && world <= avk::kMaxPeers + 1 && rank >= 0 && rank < world, AV_ERR_INVALID_ARG,
           "bad world/rank (at most %d ranks)", avk::kMaxPeers + 1);
  AV_TRY(shard_checks(e, world, rank));
  AV_CHECK(e->comm == nullptr && e->peer_world == 0, AV_ERR_UNSUPPORTED, "exchange already initialised");
  AV_CHECK(!e->solo_used, AV_ERR_UNSUPPORTED,
           "diagnostics option solo_barrier was used on this engine: it cannot join a peer exchange");
  AV_CHECK(!e->lossy(), AV_ERR_UNSUPPORTED,
           "lost Responses or unresponsive nodes (av_set_loss, av_set_responding) on a peer-push engine");
  // (the need masks are drawn from R1)
  AV_CHECK(!e->listed, AV_ERR_UNSUPPORTED, "peer lists (av_set_peer_lists) on a peer-push engine");
  AV_CHECK(e->arrive != nullptr, AV_ERR_INVALID_ARG, "call av_peer_handles before av_peer_init");
  for (int r = 0; r < world; ++r) {
    void* ptrs[4] = {e->pref[0], e->pref[1], e->pref[2], e->arrive};
    if (r != rank) {
      // a peer GPU this process can see must be reachable (xGMI peer access);
      // one it cannot see (restricted visibility) is left to the IPC mapping
      char bus[65] = {};
      std::memcpy(bus, handles + (size_t)r * AV_PEER_HANDLE_BYTES + 4 * sizeof(hipIpcMemHandle_t), 64);
      int pdev = -1;
      if (bus[0] && hipDeviceGetByPCIBusId(&pdev, bus) == hipSuccess && pdev != e->cfg.device) {
        int can = 0;
        AV_HIP(hipDeviceCanAccessPeer(&can, e->cfg.device, pdev));
        AV_CHECK(can, AV_ERR_UNSUPPORTED, "device %d cannot access peer device %d (%s)", e->cfg.device, pdev, bus);
        hipError_t pe = hipDeviceEnablePeerAccess(pdev, 0);
        AV_CHECK(pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled, AV_ERR_HIP,
                 "hipDeviceEnablePeerAccess(%d): %s", pdev, hipGetErrorString(pe));
        (void)hipGetLastError();
      } else {
        (void)hipGetLastError();
      }
      for (int i = 0; i < 4; ++i) {
        hipIpcMemHandle_t h;
        std::memcpy(&h, handles + (size_t)r * AV_PEER_HANDLE_BYTES + i * sizeof(h), sizeof(h));
        void* m = nullptr;
        AV_HIP(hipIpcOpenMemHandle(&m, h, hipIpcMemLazyEnablePeerAccess));
        e->peer_opened.push_back(m);
        ptrs[i] = m;
      }
    }
    for (int b = 0; b < 3; ++b) e->peer_pref[b][r] = static_cast<uint32_t*>(ptrs[b]);
    e->peer_arrive.p[r] = static_cast<uint32_t*>(ptrs[3]);
    e->peer_needin.p[r] = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ptrs[3]) + kNeedinOff);
  }
  e->needin = e->peer_needin.p[rank];
  AV_TRY(upload_push_tbl(e, world, rank));
  e->peer_world = world;
  e->peer_rank = rank;
  if (world > 1) {
    // every replica of every snapshot buffer identical from here on: each
    // rank pushes its own rows of the three buffers, then all ranks meet
    for (int b = 0; b < 3; ++b) {
      AV_TRY(push_own_rows(e, b));
    }
    AV_TRY(mask_setup(e));
    AV_TRY(need_gen(e, e->round / avk::kNeedWin));
    AV_TRY(peer_barrier(e));
  }
  return av_synchronize(e);
}

int av_peer_group_serial(av_engine** engines, int32_t world) {
  AV_CHECK(engines && world >= 2 && world <= avk::kMaxPeers + 1, AV_ERR_INVALID_ARG,
           "bad engines/world (2..%d ranks)", avk::kMaxPeers + 1);
  for (int r = 0; r < world; ++r) {
    av_engine* e = engines[r];
    AV_CHECK(e, AV_ERR_INVALID_ARG, "null engine");
    AV_CHECK(e->cfg.device == engines[0]->cfg.device, AV_ERR_UNSUPPORTED, "peer group: one device");
    AV_CHECK(e->N == engines[0]->N && e->M == engines[0]->M && e->k == engines[0]->k &&
                 e->cfg.seed == engines[0]->cfg.seed && e->cfg.byz_threshold == engines[0]->cfg.byz_threshold &&
                 e->cfg.peer_mode == engines[0]->cfg.peer_mode && e->round == engines[0]->round &&
                 e->cur == engines[0]->cur,
             AV_ERR_INVALID_ARG, "peer group: engines of one network at one round");
    AV_TRY(shard_checks(e, world, r));
    AV_CHECK(e->comm == nullptr && e->peer_world == 0 && !e->arrive && !e->solo_used, AV_ERR_UNSUPPORTED,
             "exchange already initialised");
    AV_CHECK(!e->lossy(), AV_ERR_UNSUPPORTED,
             "lost Responses or unresponsive nodes (av_set_loss, av_set_responding) on a peer-push engine");
    AV_CHECK(!e->listed, AV_ERR_UNSUPPORTED, "peer lists (av_set_peer_lists) on a peer-push engine");
  }
  AV_HIP(hipSetDevice(engines[0]->cfg.device));
  for (int r = 0; r < world; ++r) AV_HIP(hipStreamSynchronize(engines[r]->stream));
  // the snapshot buffers the real exchange uses (av_peer_handles): fine-grained unless option
  // "peer_fine" is 0, so that the group's parity runs and per-rank timings see the same memory type
  for (int r = 0; r < world; ++r)
    if (engines[r]->peer_fine) AV_TRY(realloc_pref(engines[r], hipDeviceMallocFinegrained));
  // what can fail comes first, with the group still the guard's: an engine is linked to a group
  // (av_destroy then unlinks it) only once every engine can be
  std::unique_ptr<PeerGroup> guard(new PeerGroup());
  AV_CHECK(guard->stream.create(hipStreamNonBlocking) == hipSuccess, AV_ERR_HIP, "hipStreamCreate failed");
  for (int r = 0; r < world; ++r) {
    av_engine* e = engines[r];
    for (int b = 0; b < 3; ++b)
      for (int q = 0; q < world; ++q) e->peer_pref[b][q] = engines[q]->pref[b];
    AV_TRY(upload_push_tbl(e, world, r));
    AV_HIP(e->needin_own.alloc(needin_words(e, world)));
  }
  PeerGroup* g = guard.release();
  g->members.assign(engines, engines + world);
  g->alive = world;
  for (int r = 0; r < world; ++r) {
    av_engine* e = engines[r];
    e->facts.snapshot_written();
    e->group = g;
    e->stream = g->stream;
    e->peer_world = world;
    e->peer_rank = r;
    e->needin = e->needin_own;
    for (int q = 0; q < world; ++q) engines[q]->peer_needin.p[r] = e->needin;
  }
  // every replica of every snapshot buffer identical from here on
  for (int r = 0; r < world; ++r) {
    for (int b = 0; b < 3; ++b) {
      AV_TRY(push_own_rows(engines[r], b));
    }
    AV_TRY(mask_setup(engines[r]));
    AV_TRY(need_gen(engines[r], engines[r]->round / avk::kNeedWin));
  }
  AV_HIP(hipStreamSynchronize(g->stream));
  return AV_OK;
}

int av_peer_sync(av_engine* e) {
  AV_ENTER(e);
  AV_PEER_CHECK(e);
  if (e->peer_world <= 1) return AV_OK;
  AV_TRY(push_own_rows(e, e->cur));
  AV_TRY(stale_clear(e, e->cur));
  AV_TRY(peer_barrier(e));
  AV_HIP(hipStreamSynchronize(e->stream));
  return peer_failed(e);
}

}  // extern "C"
