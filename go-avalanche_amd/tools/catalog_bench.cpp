// catalog_bench — what the device Hash catalog costs and saves on a C2-shaped drop-in batch
// (DESIGN.md §4 "Hash catalog"): nodes x responses Responses of `votes` slot-ascending votes over
// `targets` catalogued random 64-bit hashes, registered three ways:
//   (a) av_register_votes_batch with the slots already translated (the floor),
//   (b) a host std::unordered_map translation on one thread, then (a) (what a caller did before),
//   (c) av_register_votes_hashed (the device looks the hashes up).
// The records are re-initialised (untimed) before every timed call, so each call does the same work.
// Prints per-call wall times, their medians after the warm-up calls, and the time of a pinned
// host-to-device copy of 4 and 8 bytes per vote (c copies 12 B per vote where a copies 4).
//   bin/catalog_bench [--nodes 1000] [--resp 8] [--votes 4096] [--targets 10000] [--reps 7] [--warmup 2]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/avhip.h"

namespace {

uint64_t mix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void must(int rc, const char* what) {
  if (rc == AV_OK) return;
  std::fprintf(stderr, "%s: %s: %s\n", what, av_strerror(rc), av_last_error());
  std::exit(1);
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}

}  // namespace

int main(int argc, char** argv) {
  int64_t nodes = 1000, resp = 8, votes = 4096, targets = 10000, reps = 7, warmup = 2;
  for (int i = 1; i + 1 < argc; i += 2) {
    const std::string a = argv[i];
    const int64_t v = std::atoll(argv[i + 1]);
    if (a == "--nodes") nodes = v;
    else if (a == "--resp") resp = v;
    else if (a == "--votes") votes = v;
    else if (a == "--targets") targets = v;
    else if (a == "--reps") reps = v;
    else if (a == "--warmup") warmup = v;
    else return std::fprintf(stderr, "unknown option %s\n", a.c_str()), 2;
  }
  if (votes > targets || nodes < 9) return std::fprintf(stderr, "need votes <= targets and nodes >= 9\n"), 2;
  av_config cfg;
  av_config_init(&cfg);
  cfg.n_nodes = nodes;
  cfg.n_targets = targets;
  cfg.k = 8;
  av_engine* e = nullptr;
  must(av_create(&cfg, &e), "av_create");

  uint64_t seed = 12345;
  std::vector<int64_t> hash((size_t)targets), slot_of_hash((size_t)targets);
  for (auto& h : hash) h = (int64_t)mix(seed);
  must(av_catalog_intern(e, hash.data(), targets, slot_of_hash.data()), "av_catalog_intern");
  std::unordered_map<int64_t, int64_t> map;  // the catalog a caller kept before
  for (int64_t t = 0; t < targets; ++t) map[hash[(size_t)t]] = slot_of_hash[(size_t)t];

  const int64_t n_resp = nodes * resp, n = n_resp * votes;
  std::vector<int64_t> rnode((size_t)n_resp), offs((size_t)n_resp + 1), slots((size_t)n), hashes((size_t)n),
      translated((size_t)n);
  std::vector<uint32_t> errs((size_t)n, 0u);
  std::vector<int32_t> status((size_t)n);
  for (int64_t r = 0; r < n_resp; ++r) {
    rnode[(size_t)r] = r / resp;
    offs[(size_t)r + 1] = (r + 1) * votes;
    // selection sampling: `votes` of the `targets` slots, ascending (a poll set's order)
    int64_t need = votes, at = r * votes;
    for (int64_t t = 0; t < targets && need; ++t)
      if ((int64_t)(mix(seed) % (uint64_t)(targets - t)) < need) {
        slots[(size_t)at] = slot_of_hash[(size_t)t];
        hashes[(size_t)at++] = hash[(size_t)t];
        --need;
      }
  }
  std::printf("catalog_bench: %lld nodes x %lld Responses x %lld votes = %lld votes over %lld hashes\n",
              (long long)nodes, (long long)resp, (long long)votes, (long long)n, (long long)targets);

  std::vector<double> ta, tb, tc, tmap;
  for (int64_t it = 0; it < warmup + reps; ++it) {
    double t[3] = {0, 0, 0}, tm = 0;
    for (int c = 0; c < 3; ++c) {
      const int which = (int)((it + c) % 3);  // rotate the order of the three cases
      must(av_init_records(e, AV_INIT_ACCEPTED, 0), "av_init_records");
      must(av_synchronize(e), "av_synchronize");
      const double t0 = now_ms();
      if (which == 0) {
        must(av_register_votes_batch(e, n_resp, rnode.data(), offs.data(), slots.data(), errs.data(), status.data()),
             "av_register_votes_batch");
      } else if (which == 1) {
        for (int64_t v = 0; v < n; ++v) {
          auto f = map.find(hashes[(size_t)v]);
          translated[(size_t)v] = f == map.end() ? -1 : f->second;
        }
        tm = now_ms() - t0;
        must(av_register_votes_batch(e, n_resp, rnode.data(), offs.data(), translated.data(), errs.data(),
                                     status.data()),
             "av_register_votes_batch");
      } else {
        must(av_register_votes_hashed(e, n_resp, rnode.data(), offs.data(), hashes.data(), errs.data(), status.data()),
             "av_register_votes_hashed");
      }
      t[which] = now_ms() - t0;
    }
    std::printf("call %lld%s: (a) slots %.1f ms  (b) host map + slots %.1f ms (map %.1f)  (c) hashed %.1f ms\n",
                (long long)it, it < warmup ? " (warm-up)" : "", t[0], t[1], tm, t[2]);
    if (it < warmup) continue;
    ta.push_back(t[0]);
    tb.push_back(t[1]);
    tc.push_back(t[2]);
    tmap.push_back(tm);
  }
  if (translated != slots) return std::fprintf(stderr, "host translation differs from the catalog\n"), 1;

  // the copy the hashed call adds: 8 more bytes per vote in (12 B against 4 B), pinned to device
  double copy_ms[2] = {0, 0};
  for (int w = 0; w < 2; ++w) {
    const size_t bytes = (size_t)n * (w ? 8 : 4);
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&d, bytes) != hipSuccess)
      return std::fprintf(stderr, "copy buffers: out of memory\n"), 1;
    std::memset(h, 1, bytes);
    std::vector<double> ts;
    for (int i = 0; i < 5; ++i) {
      const double t0 = now_ms();
      if (hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return 1;
      ts.push_back(now_ms() - t0);
    }
    copy_ms[w] = median(ts);
    (void)hipFree(d);
    (void)hipHostFree(h);
  }
  const double a = median(ta), b = median(tb), c = median(tc);
  std::printf("medians of %lld calls: (a) %.1f ms  (b) %.1f ms (host map alone %.1f ms)  (c) %.1f ms\n",
              (long long)reps, a, b, median(tmap), c);
  std::printf("(c) - (a) = %.1f ms; pinned copy of 4 B per vote %.1f ms, of 8 B per vote %.1f ms\n", c - a, copy_ms[0],
              copy_ms[1]);
  std::printf("{\"votes\": %lld, \"a_ms\": %.2f, \"b_ms\": %.2f, \"map_ms\": %.2f, \"c_ms\": %.2f, \"copy4_ms\": %.2f, "
              "\"copy8_ms\": %.2f, \"c_below_b\": %s}\n",
              (long long)n, a, b, median(tmap), c, copy_ms[0], copy_ms[1], c < b ? "true" : "false");
  must(av_destroy(e), "av_destroy");
  return 0;
}
