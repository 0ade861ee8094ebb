// libavhip.so: the engine's Hash catalog (catalog.h). The caller's 64-bit hashes (avalanche.go:71)
// are interned into the slots of the engine's target range on the host; the device holds a copy of
// the table image that av_register_votes_hashed (engine_dropin.cpp) and av_catalog_find_device probe.
#include <cstring>

#include "engine.h"

using namespace aveng;

namespace {

void catalog_ensure(av_engine* e) {
  if (!e->cat.ready()) e->cat.init((uint32_t)(e->t1 - e->t0));
}

}  // namespace

namespace aveng {

int catalog_sync(av_engine* e) {
  catalog_ensure(e);
  avcat::Catalog& c = e->cat;
  const bool fresh = !e->cat_dev.get();
  if (fresh) AV_HIP(e->cat_dev.alloc(c.entries()));
  if (fresh || c.dirty_all()) {
    AV_HIP(hipMemcpyAsync(e->cat_dev, c.image(), (size_t)c.entries() * sizeof(avcat::Entry), hipMemcpyHostToDevice,
                          e->stream));
  } else {
    for (uint32_t i : c.dirty())
      AV_HIP(hipMemcpyAsync(e->cat_dev + i, c.image() + i, sizeof(avcat::Entry), hipMemcpyHostToDevice, e->stream));
  }
  if (fresh || c.dirty_all() || !c.dirty().empty()) AV_HIP(hipStreamSynchronize(e->stream));
  c.clear_dirty();
  return AV_OK;
}

int catalog_pack(av_engine* e, const int64_t* dh, const uint32_t* derr, const uint32_t* dresp_off, uint32_t n_resp,
                 uint32_t n, uint32_t* dpacked, uint32_t* dunordered) {
  avk::CatalogPackParams p{};
  p.tab = e->cat_dev;
  p.hashes = dh;
  p.errs = derr;
  p.resp_off = dresp_off;
  p.packed = dpacked;
  p.unordered = dunordered;
  p.mask = e->cat.mask();
  p.n = n;
  p.n_resp = n_resp;
  const bool lds = e->catalog_lds && e->cat.entries() <= avk::kCatLdsEntries;
  AV_HIP(avk::launch_catalog_pack(p, e->catalog_blocks, lds, e->stream));
  return AV_OK;
}

}  // namespace aveng

extern "C" {

int av_catalog_intern(av_engine* e, const int64_t* hashes, int64_t n, int64_t* slots) {
  AV_CHECK(e, AV_ERR_INVALID_ARG, "null engine");
  AV_CHECK(n >= 0 && (n == 0 || (hashes && slots)), AV_ERR_INVALID_ARG, "null argument");
  if (n == 0) return AV_OK;
  catalog_ensure(e);
  for (int64_t i = 0; i < n; ++i) {
    bool fresh = false;
    const int32_t s = e->cat.intern(hashes[i], &fresh);
    slots[i] = s < 0 ? -1 : e->t0 + s;
    // a new hash in a slot whose validity bit is off (its last tenant was invalid): valid again
    if (fresh && !((e->valid_host[(uint32_t)s >> 5] >> (s & 31)) & 1u)) AV_TRY(av_set_valid(e, e->t0 + s, 1));
  }
  return AV_OK;
}

int av_catalog_find(av_engine* e, const int64_t* hashes, int64_t n, int64_t* slots) {
  AV_CHECK(e, AV_ERR_INVALID_ARG, "null engine");
  AV_CHECK(n >= 0 && (n == 0 || (hashes && slots)), AV_ERR_INVALID_ARG, "null argument");
  for (int64_t i = 0; i < n; ++i) {
    const int32_t s = e->cat.find(hashes[i]);
    slots[i] = s < 0 ? -1 : e->t0 + s;
  }
  return AV_OK;
}

int av_catalog_find_device(av_engine* e, const int64_t* hashes, int64_t n, int64_t* slots) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(n >= 0 && (n == 0 || (hashes && slots)), AV_ERR_INVALID_ARG, "null argument");
  AV_CHECK(n < (1ll << 31), AV_ERR_INVALID_ARG, "too many hashes in one call");
  AV_TRY(catalog_sync(e));
  if (n == 0) return AV_OK;
  const size_t m = (size_t)n;
  avlay::Carver size;
  avlay::find_staging(size, m);
  AV_HIP(e->dropin_host.reserve(size.bytes(), avmem::Slack::kMiB, hipHostMallocDefault));
  void* buf = nullptr;
  AV_TRY(engine_scratch(e, size.bytes(), &buf));
  avlay::Carver host(e->dropin_host.get()), dev(buf);
  const avlay::FindStaging h = avlay::find_staging(host, m), d = avlay::find_staging(dev, m);
  std::memcpy(h.hashes, hashes, m * 8);
  AV_HIP(hipMemcpyAsync(d.hashes, h.hashes, m * 8, hipMemcpyHostToDevice, e->stream));
  AV_TRY(catalog_pack(e, d.hashes, nullptr, nullptr, 0u, (uint32_t)n, d.packed, nullptr));
  AV_HIP(hipMemcpyAsync(h.packed, d.packed, m * 4, hipMemcpyDeviceToHost, e->stream));
  AV_HIP(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < m; ++i)
    slots[i] = (h.packed[i] & avk::kDropUnknown) ? -1 : e->t0 + (int64_t)(h.packed[i] & avk::kDropTl);
  return AV_OK;
}

int av_catalog_hashes(av_engine* e, int64_t* hashes, uint8_t* used) {
  AV_CHECK(e && hashes && used, AV_ERR_INVALID_ARG, "null argument");
  const uint32_t tn = (uint32_t)(e->t1 - e->t0);
  for (uint32_t s = 0; s < tn; ++s) {
    const bool u = e->cat.ready() && e->cat.slot_used(s);
    used[s] = u ? 1 : 0;
    hashes[s] = u ? e->cat.hash_of(s) : 0;
  }
  return AV_OK;
}

// A hash may go once no local node holds a record of its slot, live or of an invalid target: the
// census' classes (av_census: stream-ordered after the rounds, the deferred state left in place).
int av_catalog_retire(av_engine* e, const int64_t* hashes, int64_t n, int32_t commit, uint8_t* retirable) {
  AV_ENTER(e);
  AV_PEER_SYNC_CHECK(e);
  AV_CHECK(n >= 0 && (n == 0 || (hashes && retirable)), AV_ERR_INVALID_ARG, "null argument");
  if (n == 0) return AV_OK;
  if (commit) {
    // pending StatusUpdate words carry slots: the caller fetches them before a slot changes hands
    int64_t pending = 0;
    AV_TRY(av_updates_count(e, &pending));
    AV_CHECK(pending == 0, AV_ERR_UNSUPPORTED, "%lld StatusUpdates pending: fetch them before retiring hashes",
             (long long)pending);
  }
  std::vector<int32_t> slot((size_t)n);
  bool any = false;
  for (int64_t i = 0; i < n; ++i) any |= (slot[(size_t)i] = e->cat.find(hashes[i])) >= 0;
  std::fill(retirable, retirable + n, (uint8_t)0);
  if (!any) return AV_OK;
  std::vector<int64_t> cls((size_t)(e->t1 - e->t0) * AV_CENSUS_CLASSES);
  av_census_out out{};
  out.target_classes = cls.data();
  AV_TRY(av_census(e, e->n0, e->n1, 0, &out));
  for (int64_t i = 0; i < n; ++i) {
    const int32_t s = slot[(size_t)i];
    if (s < 0) continue;
    const int64_t* row = cls.data() + (size_t)s * AV_CENSUS_CLASSES;
    retirable[i] = row[AV_CENSUS_LIVE_REJECTED] + row[AV_CENSUS_LIVE_ACCEPTED] == 0 ? 1 : 0;
  }
  if (commit)
    for (int64_t i = 0; i < n; ++i)
      if (retirable[i]) e->cat.retire(hashes[i]);  // a repeated hash: gone at its first position
  return AV_OK;
}

}  // extern "C"
