// The Hash catalog on the device (CDNA4, gfx950): av_register_votes_hashed's lookup-and-pack kernel,
// which av_catalog_find_device runs as a parity dump. Per vote: the caller's 64-bit hash -> probe of
// the engine's table image (catalog.h probe, the host's own function) -> slot -> the packed vote
// (dropin_word) that k_dropin_resp / k_dropin_keys consume. The host has not looked anything up, so
// the kernel also says whether the batch may take the fast apply path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "catalog.h"
#include "kernels.h"

namespace avk {

namespace {

using avcat::Entry;

// The Response of vote v: the largest r of [lo, hi] with off[r] <= v (off[lo] <= v). Empty Responses
// share their offset with the next one; the largest r is the one that holds v.
__device__ __forceinline__ uint32_t resp_of(const uint32_t* off, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
    if (off[mid] <= v) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// Whether the catalogued vote v (slot sv) keeps its Response fit for k_dropin_resp, which starts one
// thread at every vote whose predecessor is uncatalogued or in another 32-slot block: the nearest
// catalogued vote before v in the Response must have a lower slot and, if uncatalogued votes lie
// between the two, another block (else two threads would walk one lane). sp: the slot of vote v - 1
// (-1: uncatalogued). The walk back over uncatalogued votes is bounded; past the bound the batch
// takes the general path.
constexpr uint32_t kCatBack = 32;
template <typename Tab>
__device__ __forceinline__ bool keeps_order(Tab tab, uint32_t mask, const int64_t* hashes, uint32_t start, uint32_t v,
                                            int32_t sv, int32_t sp) {
  if (sv < 0 || v == start) return true;
  if (sp >= 0) return sp < sv;
  uint32_t u = v - 1u;
  for (uint32_t steps = 0; u > start; ++steps) {
    if (steps == kCatBack) return false;
    --u;
    const int32_t s = avcat::probe(tab, mask, hashes[u]);
    if (s >= 0) return s < sv && (s >> 5) != (sv >> 5);
  }
  return true;
}

// A wave takes 128 consecutive votes per pass, two per lane (one 16-B hash load, one 8-B packed
// store), grid-stride over the batch. kLds: the table image (<= kCatLdsEntries entries) is staged
// into LDS once per workgroup and probed there; else it is probed in global memory (it stays in L2).
// p.n_resp == 0 (the parity dump): no Responses, no order test.
template <bool kLds>
__global__ __launch_bounds__(256) void k_catalog_pack(const CatalogPackParams p) {
  __shared__ Entry s_tab[kLds ? kCatLdsEntries : 1u];
  if (kLds) {
    for (uint32_t i = threadIdx.x; i <= p.mask; i += 256u) s_tab[i] = p.tab[i];
    __syncthreads();
  }
  auto lookup = [&](int64_t h) -> int32_t {
    return kLds ? avcat::probe(&s_tab[0], p.mask, h) : avcat::probe(p.tab, p.mask, h);
  };
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6), waves = (uint64_t)gridDim.x * 4u;
  bool bad = false;
  for (uint64_t base = wave * 128u; base < p.n; base += waves * 128u) {  // wave-uniform
    const uint32_t v0 = (uint32_t)base + 2u * lane, v1 = v0 + 1u;
    const bool in0 = v0 < p.n, in1 = v1 < p.n;
    int64_t h0 = 0, h1 = 0;
    if (in1) {
      const longlong2 hh = *reinterpret_cast<const longlong2*>(p.hashes + v0);  // v0 even, hashes 16-B aligned
      h0 = hh.x;
      h1 = hh.y;
    } else if (in0) {
      h0 = p.hashes[v0];
    }
    const int32_t s0 = in0 ? lookup(h0) : -1;
    const int32_t s1 = in1 ? lookup(h1) : -1;
    const uint32_t e0 = p.errs && in0 ? p.errs[v0] : 0u, e1 = p.errs && in1 ? p.errs[v1] : 0u;
    const uint32_t w0 = dropin_word(s0, s0 >= 0, e0), w1 = dropin_word(s1, s1 >= 0, e1);
    if (in1) *reinterpret_cast<uint2*>(p.packed + v0) = make_uint2(w0, w1);
    else if (in0) p.packed[v0] = w0;
    if (!p.n_resp) continue;
    // the slot before v0: the previous lane's second vote; the wave's first lane looks it up
    int32_t sp = __shfl_up(s1, 1);
    if (lane == 0u) sp = base ? lookup(p.hashes[base - 1u]) : -1;
    const uint32_t last = (uint32_t)std::min<uint64_t>(base + 127u, (uint64_t)p.n - 1u);
    const uint32_t ra = resp_of(p.resp_off, 0u, p.n_resp - 1u, (uint32_t)base);
    const uint32_t rb = resp_of(p.resp_off, ra, p.n_resp - 1u, last);
    if (in0) {
      const uint32_t r = resp_of(p.resp_off, ra, rb, v0);
      bad |= kLds ? !keeps_order(&s_tab[0], p.mask, p.hashes, p.resp_off[r], v0, s0, sp)
                  : !keeps_order(p.tab, p.mask, p.hashes, p.resp_off[r], v0, s0, sp);
    }
    if (in1) {
      const uint32_t r = resp_of(p.resp_off, ra, rb, v1);
      bad |= kLds ? !keeps_order(&s_tab[0], p.mask, p.hashes, p.resp_off[r], v1, s1, s0)
                  : !keeps_order(p.tab, p.mask, p.hashes, p.resp_off[r], v1, s1, s0);
    }
  }
  if (bad) atomicOr(p.unordered, 1u);
}

}  // namespace

hipError_t launch_catalog_pack(const CatalogPackParams& p, uint32_t blocks, bool lds, hipStream_t s) {
  if (!p.n) return hipSuccess;
  if (lds && p.mask >= kCatLdsEntries) return hipErrorInvalidValue;
  const uint32_t need = (p.n + 511u) / 512u;  // 512 votes per workgroup and pass
  const uint32_t g = std::min(need, blocks ? blocks : 2048u);
  if (lds) hipLaunchKernelGGL(k_catalog_pack<true>, dim3(g), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(k_catalog_pack<false>, dim3(g), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace avk
