// libavhip.so: StatusUpdate delivery. The pending log's counters, its canonical order and compact
// encoding on the device (log_ops.hip), the copies out, and the calls that fetch, size and discard it.
#include <cstring>

#include "engine.h"

using namespace aveng;

namespace {

// Reset the three log counters (and the overflow flag) on the engine stream.
int clear_log(av_engine* e) {
  AV_HIP(hipMemsetAsync(e->log_count, 0, (size_t)3 * avk::kLogShards * avk::kCtrStride * 4, e->stream));
  AV_HIP(hipMemsetAsync(e->upd_count, 0, avk::kLogShards * 4, e->stream));
  AV_HIP(hipMemsetAsync(e->log_overflow, 0, 4, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  e->log_base = e->round;
  set_log_layout(e);  // empty now: the shards follow the current sweep grid
  return AV_OK;
}

// Pending log state: per-shard counters copied to the host.
struct LogCounts {
  std::vector<uint32_t> singles, dense, med, upd;
  uint32_t ovf = 0;
  int64_t total = 0, n_singles = 0, n_records = 0, n_med = 0;
};

int read_log_counts(av_engine* e, LogCounts& c) {
  c.singles.assign(avk::kLogShards, 0);
  c.dense.assign(avk::kLogShards, 0);
  c.upd.assign(avk::kLogShards, 0);
  c.med.assign(avk::kLogShards, 0);
  // the three kinds' counters, one per 128-B line (kernels.h kCtrStride): copied 2-D, element 0 of each
  AV_HIP(hipMemcpy2DAsync(c.singles.data(), 4, e->log_count, avk::kCtrStride * 4, 4, avk::kLogShards,
                          hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipMemcpy2DAsync(c.dense.data(), 4, e->dlog_count, avk::kCtrStride * 4, 4, avk::kLogShards,
                          hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipMemcpy2DAsync(c.med.data(), 4, e->mlog_count, avk::kCtrStride * 4, 4, avk::kLogShards,
                          hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipMemcpyAsync(c.upd.data(), e->upd_count, avk::kLogShards * 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipMemcpyAsync(&c.ovf, e->log_overflow, 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  for (uint32_t i = 0; i < avk::kLogShards; ++i) {
    c.n_med += std::min<uint32_t>(c.med[i], e->mlog_cap);
    c.total += c.upd[i];
    c.n_singles += std::min<uint32_t>(c.singles[i], e->log_cap);
    c.n_records += std::min<uint32_t>(c.dense[i], e->dlog_cap);
  }
  return AV_OK;
}

// n bytes from device memory into the caller's host buffer. Pinned caller memory: one DMA. Pageable
// memory: chunks through two pinned staging buffers, the DMA of chunk i + 1 in flight while host
// threads copy chunk i out (a hipMemcpy into pageable memory is staged by the runtime at ~14.5 GB/s,
// DESIGN.md §4 delivery).
int copy_out_bytes(av_engine* e, void* out, const void* dev, size_t n) {
  if (!n) return AV_OK;
  hipPointerAttribute_t at{};
  bool pinned = false;
  if (hipPointerGetAttributes(&at, out) == hipSuccess) pinned = at.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  constexpr size_t kChunk = (size_t)64 << 20;  // bytes
  if (pinned || n <= (size_t)4 << 20) {
    AV_HIP(hipMemcpyAsync(out, dev, n, hipMemcpyDeviceToHost, e->stream));
    AV_HIP(hipStreamSynchronize(e->stream));
    return AV_OK;
  }
  for (int i = 0; i < 2; ++i) {
    if (!e->stage[i]) AV_HIP(e->stage[i].alloc(kChunk, hipHostMallocDefault));
    if (!e->stage_ev[i]) AV_HIP(e->stage_ev[i].create(hipEventDisableTiming));
  }
  const size_t chunks = (n + kChunk - 1) / kChunk;
  const char* src_dev = static_cast<const char*>(dev);
  auto dma = [&](size_t c) -> int {
    const size_t w = std::min(kChunk, n - c * kChunk);
    AV_HIP(hipMemcpyAsync(e->stage[c & 1], src_dev + c * kChunk, w, hipMemcpyDeviceToHost, e->stream));
    AV_HIP(hipEventRecord(e->stage_ev[c & 1], e->stream));
    return AV_OK;
  };
  AV_TRY(dma(0));
  for (size_t c = 0; c < chunks; ++c) {
    if (c + 1 < chunks) {
      AV_TRY(dma(c + 1));  // its staging buffer's previous chunk (c - 1) was copied out already
    }
    AV_HIP(hipEventSynchronize(e->stage_ev[c & 1]));
    const size_t w = std::min(kChunk, n - c * kChunk);
    const char* src = static_cast<const char*>(e->stage[c & 1].get());
    char* dst = static_cast<char*>(out) + c * kChunk;
    parallel_chunks((int64_t)w, 1 << 21, [&](int, int64_t a, int64_t b) {
      std::memcpy(dst + a, src + a, (size_t)(b - a));
    });
  }
  return AV_OK;
}

// ---- canonical StatusUpdate order on the device (log_ops.hip launch_encode_log) ----
constexpr uint32_t kChunkNodes = 4096;         // compact index granularity (nodes per index entry)
constexpr size_t kHdrBytes = sizeof(av_compact_header);

uint32_t bits_for(uint64_t n) {  // bits of the values 0 .. n - 1
  uint32_t b = 0;
  while (b < 32 && (1ull << b) < n) ++b;
  return b;
}

// Rounds the pending log can hold (round_rel < this)
uint32_t log_rounds(const av_engine* e) { return (uint32_t)std::max<int64_t>(e->round - e->log_base, 1); }

avk::EncodeParams encode_params(av_engine* e) {
  avk::EncodeParams p{};
  p.log = e->log;
  p.mlog = e->mlog;
  p.dlog = e->dlog;
  p.log_count = e->log_count;
  p.log_cap = e->log_cap;
  p.mlog_cap = e->mlog_cap;
  p.dlog_cap = e->dlog_cap;
  p.shards = e->log_shards;
  p.K = (uint32_t)e->k;
  p.n0 = (uint32_t)e->n0;
  p.NL = e->NL;
  p.BL = e->BL;
  p.t0 = (uint32_t)e->t0;
  p.r_total = log_rounds(e);
  p.round_shift = e->round_shift;
  const uint32_t tb = bits_for((uint64_t)(e->t1 - e->t0)), sb = bits_for((uint64_t)e->k);
  p.target_bits = tb;
  p.code_bytes = sb + tb + 2 <= 16 ? 2u : 4u;
  p.err = e->enc_err;
  return p;
}

// Device bytes a compact stream of the pending log needs at most (c: the log's counts).
size_t compact_bound(const av_engine* e, const avk::EncodeParams& p, const LogCounts& c) {
  const uint64_t R = p.r_total, chunks = (e->NL + kChunkNodes - 1) / kChunkNodes;
  const uint64_t entries = (uint64_t)(c.n_singles + c.n_med + c.n_records);
  const uint64_t groups = std::min<uint64_t>(R * e->NL, entries);
  return kHdrBytes + (size_t)(R * chunks + 1) * 16 + (size_t)groups * 12 + (size_t)c.total * p.code_bytes + 256;
}

// Encode the pending log (counts c) into dev: packed words (compact = false; dev holds c.total u64)
// or the compact stream (dev: compact_bound bytes; the header, with the whole stream's size in bytes,
// is returned, not written). Enqueued on the engine stream; synchronizes once per encoder pass (a log
// spanning more (round, node) buckets than one pass holds takes several) and checks that every
// counted update was laid out.
int encode_log(av_engine* e, const LogCounts& c, bool compact, void* dev, av_compact_header* hdr) {
  *hdr = av_compact_header{};
  if (!e->enc_err) AV_HIP(e->enc_err.alloc(1));
  if (!e->enc_tot) AV_HIP(e->enc_tot.alloc(4));
  avk::EncodeParams p = encode_params(e);
  const uint32_t R = p.r_total;
  const uint32_t per = std::max<uint32_t>(1, std::min<uint32_t>(R, e->enc_buckets / std::max<uint32_t>(e->NL, 1)));
  const uint64_t entries = (uint64_t)(c.n_singles + c.n_med + c.n_records);
  AV_CHECK(entries < (1ull << 40), AV_ERR_UNSUPPORTED, "StatusUpdate log too large to order");
  p.nr = per;
  void* scratch = nullptr;
  AV_TRY(engine_scratch(e, avk::encode_scratch_bytes(p, entries, per * e->NL), &scratch));
  const uint32_t chunks = (e->NL + kChunkNodes - 1) / kChunkNodes;
  auto* base = static_cast<uint8_t*>(dev);
  uint64_t* cidx = compact ? reinterpret_cast<uint64_t*>(base + kHdrBytes) : nullptr;
  uint8_t* groups = compact ? base + kHdrBytes + (size_t)((uint64_t)R * chunks + 1) * 16 : nullptr;
  AV_HIP(hipMemsetAsync(e->enc_err, 0, 4, e->stream));
  uint64_t ubase = 0, cbase = 0;
  for (uint32_t r0 = 0; r0 < R; r0 += per) {
    p.r0 = r0;
    p.nr = std::min(per, R - r0);
    const bool last = r0 + p.nr >= R;
    AV_HIP(avk::launch_encode_log(p, entries, scratch, compact ? nullptr : static_cast<uint64_t*>(dev), groups, cidx,
                                  chunks, kChunkNodes, ubase, cbase, last, e->enc_tot, e->stream));
    uint64_t tot[4] = {0, 0, 0, 0};
    uint32_t err = 0;
    AV_HIP(hipMemcpyAsync(tot, e->enc_tot, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
    AV_HIP(hipMemcpyAsync(&err, e->enc_err, 4, hipMemcpyDeviceToHost, e->stream));
    AV_HIP(hipStreamSynchronize(e->stream));
    AV_CHECK(err == 0, AV_ERR_HIP, "StatusUpdate log inconsistent (encoder flags %u)", err);
    ubase += tot[0];
    cbase += tot[1];
  }
  AV_CHECK((int64_t)ubase == c.total, AV_ERR_HIP, "StatusUpdate log inconsistent (%lld of %lld updates ordered)",
           (long long)ubase, (long long)c.total);
  if (compact) {
    av_compact_header& h = *hdr;
    h.magic = AV_COMPACT_MAGIC;
    h.version = AV_COMPACT_VERSION;
    h.log_base = e->log_base;
    h.n_updates = (int64_t)ubase;
    h.node_base = e->n0;
    h.target_base = e->t0;
    h.n_rounds = (int32_t)R;
    h.chunks = (int32_t)chunks;
    h.chunk_nodes = (int32_t)kChunkNodes;
    h.code_bytes = (int32_t)p.code_bytes;
    h.target_bits = (int32_t)p.target_bits;
    h.slot_bits = (int32_t)bits_for((uint64_t)e->k);
    h.round_shift = (int32_t)e->round_shift;
    h.bytes = (int64_t)(groups - base) + (int64_t)cbase;
  }
  return AV_OK;
}

// A compact slot's device buffer, grown with an eighth to spare (contents not kept).
int grow_dev(avmem::DevBuf<uint8_t>& buf, size_t want) {
  const hipError_t he = buf.reserve(want, avmem::Slack::kEighth);
  AV_CHECK(he == hipSuccess, oom_or_hip(he), "device buffer (%zu B): %s",
           avmem::grown_size(want, avmem::Slack::kEighth), hipGetErrorString(he));
  return AV_OK;
}

// Read the log's counters, failing (and clearing the log) if it overflowed.
int pending_counts(av_engine* e, LogCounts& c) {
  AV_TRY(read_log_counts(e, c));
  if (c.ovf) {
    AV_TRY(clear_log(e));
    return fail(AV_ERR_OVERFLOW, "device StatusUpdate log overflowed (%lld updates, capacity %lld per shard)",
                (long long)c.total, (long long)e->log_cap);
  }
  return AV_OK;
}

}  // namespace

namespace aveng {

// A sweep-grid option changed the number of log writers: re-shard the log now if it is empty
// (every enqueued round has finished: read_log_counts synchronizes), else at the next clear_log.
int relayout_log_if_empty(av_engine* e) {
  LogCounts c;
  AV_TRY(read_log_counts(e, c));
  if (!c.ovf && c.total == 0 && c.n_singles == 0 && c.n_med == 0 && c.n_records == 0) set_log_layout(e);
  return AV_OK;
}

}  // namespace aveng

extern "C" {

int av_update_round_shift(av_engine* e, int32_t* out) {
  AV_CHECK(e && out, AV_ERR_INVALID_ARG, "null argument");
  *out = (int32_t)e->round_shift;
  return AV_OK;
}

int av_log_base_round(av_engine* e, int64_t* out) {
  AV_CHECK(e && out, AV_ERR_INVALID_ARG, "null argument");
  *out = e->log_base;
  return AV_OK;
}

int av_updates_count(av_engine* e, int64_t* n) {
  AV_TRY(counter_query(e, n));
  LogCounts c;
  AV_TRY(read_log_counts(e, c));
  *n = c.total;
  return AV_OK;
}

int av_update_log_overflowed(av_engine* e, int32_t* out) {
  AV_ENTER(e);
  AV_CHECK(out, AV_ERR_INVALID_ARG, "null argument");
  uint32_t ovf = 0;
  AV_HIP(hipMemcpyAsync(&ovf, e->log_overflow, 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  *out = ovf ? 1 : 0;
  return AV_OK;
}

int av_fetch_updates(av_engine* e, uint64_t* out, int64_t cap, int64_t* n_out) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(n_out && (cap == 0 || out), AV_ERR_INVALID_ARG, "null argument");
  LogCounts c;
  int rc = pending_counts(e, c);
  *n_out = c.total;
  if (rc != AV_OK) return rc;
  AV_CHECK(c.total <= cap, AV_ERR_OVERFLOW, "cap too small: %lld updates pending", (long long)c.total);
  if (c.total > 0) {
    // the compact slots' device buffers hold no in-flight copy source after this wait
    if (e->copy_stream) AV_HIP(hipStreamSynchronize(e->copy_stream));
    AV_TRY(grow_dev(e->cdev[0], (size_t)c.total * 8));
    av_compact_header r;
    AV_TRY(encode_log(e, c, false, e->cdev[0], &r));
    AV_TRY(copy_out_bytes(e, out, e->cdev[0], (size_t)c.total * 8));
  }
  return clear_log(e);
}

int av_fetch_compact(av_engine* e, void* out, int64_t cap, int64_t* bytes) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(bytes && (cap == 0 || out), AV_ERR_INVALID_ARG, "null argument");
  *bytes = 0;
  LogCounts c;
  AV_TRY(pending_counts(e, c));
  if (e->copy_stream) AV_HIP(hipStreamSynchronize(e->copy_stream));
  const avk::EncodeParams p = encode_params(e);
  AV_TRY(grow_dev(e->cdev[0], compact_bound(e, p, c)));
  av_compact_header r;
  AV_TRY(encode_log(e, c, true, e->cdev[0], &r));
  *bytes = r.bytes;
  AV_CHECK(r.bytes <= cap, AV_ERR_OVERFLOW, "cap too small: the stream takes %lld bytes", (long long)r.bytes);
  AV_TRY(copy_out_bytes(e, static_cast<uint8_t*>(out) + kHdrBytes, e->cdev[0] + kHdrBytes, (size_t)r.bytes - kHdrBytes));
  std::memcpy(out, &r, kHdrBytes);
  return clear_log(e);
}

int av_fetch_compact_async(av_engine* e, int64_t* ticket) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(ticket, AV_ERR_INVALID_ARG, "null argument");
  if (!e->copy_stream) AV_HIP(e->copy_stream.create(hipStreamNonBlocking));
  const int s = (int)(e->cticket % av_engine::kSlots);
  if (!e->cev[s]) AV_HIP(e->cev[s].create(hipEventDisableTiming));
  LogCounts c;
  AV_TRY(pending_counts(e, c));  // waits for the rounds enqueued before
  // the slot's previous copy (ticket - kSlots) has read its device buffer and filled its host buffer
  if (e->cpend[s]) AV_HIP(hipEventSynchronize(e->cev[s]));
  e->cpend[s] = false;
  const avk::EncodeParams p = encode_params(e);
  e->cdev_hwm = std::max(e->cdev_hwm, compact_bound(e, p, c));
  AV_TRY(grow_dev(e->cdev[s], e->cdev_hwm));
  av_compact_header r;
  AV_TRY(encode_log(e, c, true, e->cdev[s], &r));  // synchronizes the engine stream
  e->chost_hwm = std::max(e->chost_hwm, (size_t)r.bytes + 16);
  AV_HIP(e->chost[s].reserve(e->chost_hwm, avmem::Slack::kEighth, hipHostMallocMapped));
  if (e->copy_blocks) {  // a small copy kernel (the header's bytes are copied too, and overwritten on wait)
    void* hdev = nullptr;
    AV_HIP(hipHostGetDevicePointer(&hdev, e->chost[s], 0));
    AV_HIP(avk::launch_stream_out(e->cdev[s], hdev, (uint64_t)r.bytes, e->copy_blocks, e->copy_stream));
  } else {
    AV_HIP(hipMemcpyAsync(e->chost[s] + kHdrBytes, e->cdev[s] + kHdrBytes, (size_t)r.bytes - kHdrBytes,
                          hipMemcpyDeviceToHost, e->copy_stream));
  }
  AV_HIP(hipEventRecord(e->cev[s], e->copy_stream));
  e->chdr[s] = r;
  e->cpend[s] = true;
  *ticket = e->cticket++;
  return clear_log(e);
}

int av_fetch_compact_wait(av_engine* e, int64_t ticket, const void** stream, int64_t* bytes) {
  AV_ENTER(e);
  AV_CHECK(stream && bytes, AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(ticket >= 0 && ticket < e->cticket && ticket >= e->cticket - av_engine::kSlots, AV_ERR_INVALID_ARG,
           "ticket %lld is not one of the last %d issued", (long long)ticket, av_engine::kSlots);
  const int s = (int)(ticket % av_engine::kSlots);
  AV_CHECK(e->cpend[s], AV_ERR_INVALID_ARG, "ticket %lld has no copy", (long long)ticket);
  AV_HIP(hipEventSynchronize(e->cev[s]));
  std::memcpy(e->chost[s], &e->chdr[s], kHdrBytes);
  *stream = e->chost[s];
  *bytes = e->chdr[s].bytes;
  return AV_OK;
}

int av_compact_expand(const void* stream, int64_t bytes, uint64_t* out, int64_t cap, int64_t* n_out) {
  AV_CHECK(stream && n_out && (cap == 0 || out), AV_ERR_INVALID_ARG, "null argument");
  *n_out = 0;
  AV_CHECK(bytes >= (int64_t)kHdrBytes, AV_ERR_INVALID_ARG, "stream shorter than its header");
  av_compact_header h;
  std::memcpy(&h, stream, kHdrBytes);
  AV_CHECK(h.magic == AV_COMPACT_MAGIC && h.version == AV_COMPACT_VERSION, AV_ERR_INVALID_ARG, "not a compact stream");
  AV_CHECK(h.bytes == bytes && h.n_rounds >= 1 && h.chunks >= 1 && (h.code_bytes == 2 || h.code_bytes == 4) &&
               h.target_bits >= 0 && h.target_bits <= 22 && h.n_updates >= 0 && h.round_shift >= 52 &&
               h.round_shift <= 60 && h.n_rounds <= (1ll << (64 - h.round_shift)),
           AV_ERR_INVALID_ARG, "malformed compact stream header");
  const uint64_t n_idx = (uint64_t)h.n_rounds * (uint64_t)h.chunks + 1;
  const uint8_t* base = static_cast<const uint8_t*>(stream);
  const uint64_t gstart = kHdrBytes + n_idx * 16;
  AV_CHECK((uint64_t)bytes >= gstart, AV_ERR_INVALID_ARG, "compact stream index truncated");
  const uint64_t* idx = reinterpret_cast<const uint64_t*>(base + kHdrBytes);
  AV_CHECK(idx[2 * (n_idx - 1)] == (uint64_t)bytes - gstart && idx[2 * (n_idx - 1) + 1] == (uint64_t)h.n_updates,
           AV_ERR_INVALID_ARG, "compact stream index inconsistent");
  *n_out = h.n_updates;
  AV_CHECK(h.n_updates <= cap, AV_ERR_OVERFLOW, "cap too small: %lld updates", (long long)h.n_updates);
  const uint8_t* groups = base + gstart;
  const uint32_t tb = (uint32_t)h.target_bits, cw = (uint32_t)h.code_bytes;
  const uint32_t tmask = (1u << tb) - 1u;
  std::vector<int> bad(64, 0);
  parallel_chunks((int64_t)(n_idx - 1), 1, [&](int t, int64_t j0, int64_t j1) {
    for (int64_t j = j0; j < j1; ++j) {
      const uint64_t rr = (uint64_t)j / (uint64_t)h.chunks;
      const uint64_t b0 = idx[2 * j], b1 = idx[2 * j + 2];
      uint64_t u = idx[2 * j + 1];
      const uint64_t u1 = idx[2 * j + 3];
      if (b0 > b1 || b1 > (uint64_t)bytes - gstart || u > u1) {
        bad[t] = 1;
        return;
      }
      for (uint64_t at = b0; at < b1;) {
        if (at + 8 > b1) {
          bad[t] = 1;
          return;
        }
        uint32_t node, n;
        std::memcpy(&node, groups + at, 4);
        std::memcpy(&n, groups + at + 4, 4);
        const uint64_t len = 8 + (((uint64_t)n * cw + 3) & ~3ull);
        if (at + len > b1 || u + n > u1 || (uint64_t)node >= (1ull << (h.round_shift - 28))) {
          bad[t] = 1;
          return;
        }
        const uint64_t hi = (rr << h.round_shift) | ((uint64_t)node << 28);
        const uint8_t* cp = groups + at + 8;
        for (uint32_t i = 0; i < n; ++i) {
          uint32_t code;
          if (cw == 2) {
            uint16_t v;
            std::memcpy(&v, cp + 2 * i, 2);
            code = v;
          } else {
            std::memcpy(&code, cp + 4 * i, 4);
          }
          const uint64_t slot = code >> (tb + 2), tl = (code >> 2) & tmask;
          out[u + i] = hi | (slot << 24) | (((uint64_t)h.target_base + tl) << 2) | (code & 3u);
        }
        u += n;
        at += len;
      }
      if (u != u1) {
        bad[t] = 1;
        return;
      }
    }
  });
  for (int b : bad) AV_CHECK(!b, AV_ERR_INVALID_ARG, "malformed compact stream groups");
  return AV_OK;
}

int av_updates_digest(av_engine* e, uint64_t out[3]) { return av_updates_digest_range(e, 0, e ? e->N : 0, out); }

int av_updates_digest_range(av_engine* e, int64_t n0, int64_t n1, uint64_t out[3]) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(out && n0 >= 0 && n0 <= n1 && n1 <= e->N, AV_ERR_INVALID_ARG, "bad argument");
  uint32_t ovf = 0;
  AV_HIP(hipMemcpyAsync(&ovf, e->log_overflow, 4, hipMemcpyDeviceToHost, e->stream));
  if (!e->digest) AV_HIP(e->digest.alloc(3));
  AV_HIP(avk::launch_log_digest(e->log, e->log_count, e->log_cap, e->dlog, e->dlog_count, e->dlog_cap, e->mlog,
                                e->mlog_count, e->mlog_cap, e->log_shards, (uint32_t)e->k, (uint32_t)n0, (uint32_t)n1,
                                e->round_shift, e->digest, e->stream));
  unsigned long long d[3] = {0, 0, 0};
  AV_HIP(hipMemcpyAsync(d, e->digest, sizeof(d), hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  AV_CHECK(!ovf, AV_ERR_OVERFLOW, "device StatusUpdate log overflowed: the digest would miss updates");
  for (int i = 0; i < 3; ++i) out[i] = (uint64_t)d[i];
  return AV_OK;
}

int av_discard_updates(av_engine* e) {
  AV_ENTER(e);
  return clear_log(e);
}

int av_log_entries(av_engine* e, int64_t out[3]) {
  AV_TRY(counter_query(e, out));
  LogCounts c;
  AV_TRY(read_log_counts(e, c));
  out[0] = c.n_singles;
  out[1] = c.n_med;
  out[2] = c.n_records;
  return AV_OK;
}

int av_resize_log(av_engine* e, const int64_t entries[3]) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(entries && entries[0] >= 0 && entries[1] >= 0 && entries[2] >= 0, AV_ERR_INVALID_ARG, "bad entries");
  LogCounts c;
  AV_TRY(read_log_counts(e, c));
  AV_CHECK(!c.ovf && c.total == 0 && c.n_singles == 0 && c.n_med == 0 && c.n_records == 0, AV_ERR_UNSUPPORTED,
           "av_resize_log: the log holds updates (fetch or discard them first)");
  // sized for the current grid's writer waves (log_writer_waves): a shard takes every sh-th writer, so
  // with w writers one shard serves up to ceil(w / sh) of them; each writer gets ceil(n / w) + 1 entries
  // (a writer owns one run of lanes, at most one more than the lanes' mean: "one entry per lane" holds
  // any round), >= 16 per shard. The allocation is that per-shard share times kLogShards, so that a
  // later re-layout to more shards keeps the total.
  const uint64_t sh = avk::kLogShards;
  const uint64_t w = std::max<uint64_t>(log_writer_waves(e), 1), lsh = log_shards_for(w);
  auto per = [&](int64_t n) {
    const uint64_t shard = (((uint64_t)n + w - 1) / w + 1) * ((w + lsh - 1) / lsh);
    return std::max<uint64_t>((shard * lsh + sh - 1) / sh, 16);
  };
  const uint64_t s1 = per(entries[0]) * sh, s2 = per(entries[1]) * sh, s3 = per(entries[2]) * sh;
  AV_CHECK(s1 / sh < (1ull << 32) && s2 / sh < (1ull << 32) && s3 / sh < (1ull << 32), AV_ERR_INVALID_ARG,
           "log too large");
  AV_HIP(hipStreamSynchronize(e->stream));
  // the new log is swapped in only once all of it exists: on failure the old one stays as it was
  avmem::DevBuf<uint64_t> log, mlog, dlog;
  hipError_t he = log.alloc(s1);
  if (he == hipSuccess) he = mlog.alloc(s2 * avk::med_rec_words());
  if (he == hipSuccess) he = dlog.alloc(s3 * avk::dense_words((uint32_t)e->k));
  if (he != hipSuccess) {
    (void)hipGetLastError();
    return fail(oom_or_hip(he), "av_resize_log: %s", hipGetErrorString(he));
  }
  e->log = std::move(log);
  e->mlog = std::move(mlog);
  e->dlog = std::move(dlog);
  e->log_alloc = s1;
  e->mlog_alloc = s2;
  e->dlog_alloc = s3;
  set_log_layout(e);
  return AV_OK;
}

}  // extern "C"
