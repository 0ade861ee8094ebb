// Engine state kernels of the batched Avalanche voting engine (CDNA4, gfx950):
// record-plane and published-preference initialisation (k_init_planes,
// k_init_pref, k_byz), record I/O in the canonical word form (k_read_records,
// k_read_records_v, k_write_records), the published row of a changed record
// (k_refresh_pref), the peer draw and the synthetic replay stream as tables
// (k_sample_peers, k_gen_replay), the live-record count (k_count_live) and the
// batched poll sets (k_poll_sets). Each launcher sits below its kernel.
//
// The round kernels are in round_firstgen.hip, round_sweep.hip and
// round_node.hip, the drop-in Processor calls in dropin.hip, the exchange of
// node-sharded engines in peer_ops.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev_scan.h"
#include "kernels.h"
#include "round_common.h"

namespace avk {

namespace {
__device__ __forceinline__ uint32_t target_mask(uint32_t tb, uint32_t n_targets) {
  if (tb >= n_targets) return 0u;
  const uint32_t r = n_targets - tb;
  return r >= 32u ? ~0u : ((1u << r) - 1u);
}

__global__ void k_init_planes(const InitParams p) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.L) return;
  const uint32_t nl = g / p.BL, b = g - nl * p.BL;
  const uint32_t tb = p.t0 + 32u * b;
  const uint32_t live = p.mode == 0 ? 0u : target_mask(tb, p.n_targets);
  const uint32_t acc = init_accept_block(p.seed, p.mode, p.param, p.n0 + nl, tb) & live;
  St s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s.V[i] = 0u;
    s.C[i] = p.c_preset ? ~0u : ~live;  // kernels.h c_preset
    s.K[i] = 0u;
  }
  s.K[7] = ~live;
  s.A = acc;
  store_state(p.planes, g, s);
}

__global__ void k_init_pref(const InitParams p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)p.n_nodes * p.BL) return;
  const uint32_t node = (uint32_t)(i / p.BL), b = (uint32_t)(i - (size_t)node * p.BL);
  const size_t o = (size_t)node * p.PS + b;
  const uint32_t tb = p.t0 + 32u * b;
  uint32_t v;
  if (is_byz(p.byz, node))
    v = byz_pattern(p.round);
  else
    v = p.mode == 0 ? (p.pub_mode == 2u ? target_mask(tb, p.n_targets) : 0u)  // no records (K7 set)
                    : (init_accept_block(p.seed, p.mode, p.param, node, tb) & target_mask(tb, p.n_targets));
  p.pref[o] = v;
}
}  // namespace

hipError_t launch_init(const InitParams& p, hipStream_t s) {
  if (p.L) hipLaunchKernelGGL(k_init_planes, dim3((p.L + 255) / 256), dim3(256), 0, s, p);
  const size_t rows = (size_t)p.n_nodes * p.BL;
  if (rows) hipLaunchKernelGGL(k_init_pref, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

namespace {
__global__ void k_byz(uint32_t* byz, uint32_t n_nodes, uint64_t seed, uint32_t threshold) {
  const uint32_t wi = blockIdx.x * blockDim.x + threadIdx.x;
  if (wi >= (n_nodes + 31u) / 32u) return;
  uint32_t bits = 0;
  for (uint32_t i = 0; i < 32u; ++i) {
    const uint32_t node = wi * 32u + i;
    if (node >= n_nodes) break;
    uint32_t x[4];
    philox(x, seed, node, 0u, 0u, kDomByz);
    bits |= (x[0] < threshold ? 1u : 0u) << i;
  }
  byz[wi] = bits;
}
}  // namespace

namespace {
// The consider planes a preset k_init_planes did not store (kernels.h c_preset): consider = 0 on every
// existing record, 1 past the engine's last target.
__global__ __launch_bounds__(256) void k_c_unpreset(uint32_t* planes, uint32_t BL, uint32_t L, uint32_t tn) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= L) return;
  const uint32_t c = ~real_mask(tn, g % BL);
#pragma unroll
  for (int i = 0; i < 8; ++i) pst<true>(pw(planes, g, kPC + i), c);
}
}  // namespace

hipError_t launch_c_unpreset(uint32_t* planes, uint32_t BL, uint32_t L, uint32_t tn, hipStream_t s) {
  if (L) hipLaunchKernelGGL(k_c_unpreset, dim3((L + 255) / 256), dim3(256), 0, s, planes, BL, L, tn);
  return hipGetLastError();
}

hipError_t launch_byz(uint32_t* byz, uint32_t n_nodes, uint64_t seed, uint32_t threshold, hipStream_t s) {
  const uint32_t words = (n_nodes + 31u) / 32u;
  hipLaunchKernelGGL(k_byz, dim3((words + 255) / 256), dim3(256), 0, s, byz, n_nodes, seed, threshold);
  return hipGetLastError();
}

namespace {
__global__ void k_read_records(const uint32_t* planes, uint32_t BL, uint32_t nl0, uint32_t nl1, uint32_t tl0,
                               uint32_t tl1, uint32_t* out) {
  const uint32_t W = tl1 - tl0;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)(nl1 - nl0) * W) return;
  const uint32_t nl = nl0 + (uint32_t)(i / W), tl = tl0 + (uint32_t)(i % W);
  const uint32_t g = nl * BL + (tl >> 5), bit = tl & 31u;
  const uint32_t a = (*pw(planes, g, kPA) >> bit) & 1u;
  if ((*pw(planes, g, kPK + 7) >> bit) & 1u) {
    out[i] = 0xFFFE0000u | (a << 16);
    return;
  }
  uint32_t v = 0, c = 0, k = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    v |= ((*pw(planes, g, kPV + q) >> bit) & 1u) << q;
    c |= ((*pw(planes, g, kPC + q) >> bit) & 1u) << q;
  }
#pragma unroll
  for (int q = 0; q < 7; ++q) k |= ((*pw(planes, g, kPK + q) >> bit) & 1u) << q;
  out[i] = v | (c << 8) | (((k << 1) | a) << 16);
}
}  // namespace

hipError_t launch_read_records(const uint32_t* planes, uint32_t BL, uint32_t nl0, uint32_t nl1, uint32_t tl0,
                               uint32_t tl1, uint32_t* out, hipStream_t s) {
  const size_t n = (size_t)(nl1 - nl0) * (tl1 - tl0);
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_read_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, planes, BL, nl0, nl1, tl0,
                     tl1, out);
  return hipGetLastError();
}

namespace {
// The same canonical words, one thread per 32-record lane, WITHOUT writing
// back the deferred forms the warm rounds leave behind (kernels.h vv / klazy):
// a stale tile's vote register is regathered from the previous snapshot
// (p.pref_prev) with round p.round - 1's peers, and a tile's pending +8 count
// steps are added to its polled (live, valid) records. Reads (IsAccepted,
// GetConfidence, GetInvsForNextPoll, dumps) then leave the next round's fast
// paths in place. p.vv / p.klazy: some tile may be stale / hold pending steps.
__global__ __launch_bounds__(256) void k_read_records_v(const RoundParams p, uint32_t nl0, uint32_t nl1, uint32_t tl0,
                                                        uint32_t tl1, uint32_t* out) {
  const uint32_t b0 = tl0 >> 5, NB = ((tl1 + 31u) >> 5) - b0, W = tl1 - tl0;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (nl1 - nl0) * NB) return;
  const uint32_t nl = nl0 + i / NB, b = b0 + i % NB;
  const uint32_t g = nl * p.BL + b, tile = g >> 6;
  St s;
  load_state(p.planes, g, s);
  const uint32_t raw = p.vv ? p.vstale[tile] : 0u, st = raw & kVMask;
  if (raw & kCAll) {  // consider planes left unstored by the fresh round: all-ones
#pragma unroll
    for (int q = 0; q < 8; ++q) s.C[q] = ~0u;
  }
  if (p.c_preset) {  // stored all-ones by av_init_records, no round since (kernels.h c_preset)
#pragma unroll
    for (int q = 0; q < 8; ++q) s.C[q] = ~real_mask(p.tn, b);
  }
  if (st == kVStale) {  // V_i = the vote of round - 1's slot 7 - i (k = 8)
    uint32_t pp[8];
    sample_peers<8>(p.seed, p.n0 + nl, p.round - 1u, p.n_nodes, p.peer_mode, pp);
#pragma unroll
    for (int q = 0; q < 8; ++q) s.V[q] = p.pref_prev[pp[7 - q] * p.PS + b];
  } else if (st == kVUniform) {  // every polled record's vote register = its accepted bit
#pragma unroll
    for (int q = 0; q < 8; ++q) s.V[q] = s.A;
  }
  if (p.klazy) {
    const uint32_t kw = p.kpend[tile];
    if (kw & kHiVirt) {  // the K4..K7 group is virtual (kernels.h)
      s.K[4] = s.K[5] = s.K[6] = 0u;
      s.K[7] = ~real_mask(p.tn, b);
    }
    const uint32_t pend = kw & 0xFFu;
    if (pend) {  // + 8 * pend on the polled records: pend added to count bits 3..6
      const uint32_t P0 = ~s.K[7] & p.valid[b];
      uint32_t cy = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t bi = ((pend >> q) & 1u) ? P0 : 0u;
        const uint32_t t = s.K[3 + q] ^ bi;
        const uint32_t si = t ^ cy;
        cy = (t & cy) | (s.K[3 + q] & bi);
        s.K[3 + q] = si;
      }
    }
  }
  const uint32_t lo = max(tl0, b * 32u), hi = min(tl1, b * 32u + 32u);
  uint32_t* dst = out + (size_t)(nl - nl0) * W;
  for (uint32_t tl = lo; tl < hi; ++tl) {
    const uint32_t bit = tl & 31u;
    const uint32_t a = (s.A >> bit) & 1u;
    uint32_t word;
    if ((s.K[7] >> bit) & 1u) {
      word = 0xFFFE0000u | (a << 16);
    } else {
      uint32_t v = 0, c = 0, k = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        v |= ((s.V[q] >> bit) & 1u) << q;
        c |= ((s.C[q] >> bit) & 1u) << q;
      }
#pragma unroll
      for (int q = 0; q < 7; ++q) k |= ((s.K[q] >> bit) & 1u) << q;
      word = v | (c << 8) | (((k << 1) | a) << 16);
    }
    dst[tl - tl0] = word;
  }
}
}  // namespace

hipError_t launch_read_records_virtual(const RoundParams& p, uint32_t nl0, uint32_t nl1, uint32_t tl0, uint32_t tl1,
                                       uint32_t* out, hipStream_t s) {
  const uint32_t nb = ((tl1 + 31u) >> 5) - (tl0 >> 5);
  const uint32_t n = (nl1 - nl0) * nb;
  if (!n || tl1 <= tl0) return hipSuccess;
  hipLaunchKernelGGL(k_read_records_v, dim3((n + 255) / 256), dim3(256), 0, s, p, nl0, nl1, tl0, tl1, out);
  return hipGetLastError();
}

namespace {
__global__ void k_write_records(uint32_t* planes, uint32_t BL, uint32_t nl0, uint32_t nl1, uint32_t tl0,
                                uint32_t tl1, const uint32_t* in) {
  const uint32_t b0 = tl0 >> 5, b1 = (tl1 + 31u) >> 5, NB = b1 - b0, W = tl1 - tl0;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (nl1 - nl0) * NB) return;
  const uint32_t nl = nl0 + i / NB, b = b0 + i % NB;
  const uint32_t g = nl * BL + b;
  St s;
  load_state(planes, g, s);
  for (uint32_t bit = 0; bit < 32u; ++bit) {
    const uint32_t tl = b * 32u + bit;
    if (tl < tl0 || tl >= tl1) continue;
    const uint32_t w = in[(size_t)(nl - nl0) * W + (tl - tl0)];
    const uint32_t m = 1u << bit;
    const uint32_t conf = w >> 16;
    const bool live = (conf >> 1) < 128u;
    for (int q = 0; q < 8; ++q) {
      const uint32_t vb = live ? (w >> q) & 1u : 0u;
      const uint32_t cb = live ? (w >> (8 + q)) & 1u : 1u;
      const uint32_t kb = live ? ((conf >> 1) >> q) & 1u : (q == 7 ? 1u : 0u);
      s.V[q] = (s.V[q] & ~m) | (vb << bit);
      s.C[q] = (s.C[q] & ~m) | (cb << bit);
      s.K[q] = (s.K[q] & ~m) | (kb << bit);
    }
    s.A = (s.A & ~m) | ((conf & 1u) << bit);
  }
  store_state(planes, g, s);
}
}  // namespace

hipError_t launch_write_records(uint32_t* planes, uint32_t BL, uint32_t nl0, uint32_t nl1, uint32_t tl0, uint32_t tl1,
                                const uint32_t* in, hipStream_t s) {
  const uint32_t nb = ((tl1 + 31u) >> 5) - (tl0 >> 5);
  const uint32_t n = (nl1 - nl0) * nb;
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_write_records, dim3((n + 255) / 256), dim3(256), 0, s, planes, BL, nl0, nl1, tl0, tl1, in);
  return hipGetLastError();
}

namespace {
__global__ void k_refresh_pref(uint32_t pub_mode, const uint32_t* planes, uint32_t* pref, const uint32_t* byz,
                               uint32_t n0, uint32_t NL, uint32_t BL, uint32_t PS, uint32_t round) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= NL * BL) return;
  const uint32_t nl = g / BL, b = g - nl * BL, node = n0 + nl;
  pref[(size_t)node * PS + b] =
      is_byz(byz, node) ? byz_pattern(round) : publish_word(*pw(planes, g, kPA), *pw(planes, g, kPK + 7), pub_mode);
}
}  // namespace

hipError_t launch_refresh_pref(uint32_t pub_mode, const uint32_t* planes, uint32_t* pref, const uint32_t* byz,
                               uint32_t n0, uint32_t NL, uint32_t BL, uint32_t PS, uint32_t round, hipStream_t s) {
  const uint32_t n = NL * BL;
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_refresh_pref, dim3((n + 255) / 256), dim3(256), 0, s, pub_mode, planes, pref, byz, n0, NL, BL,
                     PS, round);
  return hipGetLastError();
}

namespace {
template <int K>
__global__ void k_sample_peers(uint64_t seed, uint32_t n_nodes, uint32_t a, uint32_t b, uint32_t round, int mode,
                               uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (a + i >= b) return;
  uint32_t peers[K];
  sample_peers<K>(seed, a + i, round, n_nodes, mode, peers);
#pragma unroll
  for (int j = 0; j < K; ++j) out[(size_t)i * K + j] = peers[j];
}

template <int K>
hipError_t launch_sample_k(uint64_t seed, uint32_t n_nodes, uint32_t a, uint32_t b, uint32_t round, int mode,
                           uint32_t* out, hipStream_t s) {
  const uint32_t n = b - a;
  hipLaunchKernelGGL((k_sample_peers<K>), dim3((n + 255) / 256), dim3(256), 0, s, seed, n_nodes, a, b, round, mode,
                     out);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_sample_peers(uint64_t seed, uint32_t n_nodes, uint32_t a, uint32_t b, uint32_t round, int k,
                               int mode, uint32_t* out, hipStream_t s) {
  if (b <= a) return hipSuccess;
  return dispatch_k<kMaxK>(k, [&](auto K) { return launch_sample_k<K()>(seed, n_nodes, a, b, round, mode, out, s); });
}

namespace {
// Synthetic replayed vote stream (C2): class per (node, round, slot, target)
// from philox(node, round, t>>1, REPLAY | slot<<8); same definition as
// avo_replay_err in the oracle. Output: the tiled replay layout (kernels.h replay_idx).
__global__ void k_gen_replay(uint64_t seed, uint32_t n0, uint32_t BL, uint32_t L, uint32_t Lpad, uint32_t t0,
                             uint32_t n_targets, uint32_t round, int k, uint32_t* out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= Lpad) return;
  if (g >= L) {
    for (int s = 0; s < k; ++s) {
      out[replay_idx(g, k, s, 0)] = 0u;
      out[replay_idx(g, k, s, 1)] = 0u;
    }
    return;
  }
  const uint32_t nl = g / BL, b = g - nl * BL, node = n0 + nl;
  const uint32_t tb = t0 + 32u * b;
  const uint32_t tm = target_mask(tb, n_targets);
  for (int s = 0; s < k; ++s) {
    uint32_t y = 0, c = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      uint32_t x[4];
      philox(x, seed, node, round, (tb >> 1) + q, kDomReplay | ((uint32_t)s << 8));
      const uint32_t v0 = x[0], v1 = x[2];
      y |= (v0 < kReplayYes ? 1u : 0u) << (2 * q);
      c |= (v0 < kReplayNo ? 1u : 0u) << (2 * q);
      y |= (v1 < kReplayYes ? 1u : 0u) << (2 * q + 1);
      c |= (v1 < kReplayNo ? 1u : 0u) << (2 * q + 1);
    }
    out[replay_idx(g, k, s, 0)] = y & tm;
    out[replay_idx(g, k, s, 1)] = c & tm;
  }
}
}  // namespace

hipError_t launch_gen_replay(uint64_t seed, uint32_t n0, uint32_t NL, uint32_t BL, uint32_t L, uint32_t Lpad,
                             uint32_t t0, uint32_t n_targets, uint32_t round, int k, uint32_t* out, hipStream_t s) {
  (void)NL;
  if (!Lpad) return hipSuccess;
  hipLaunchKernelGGL(k_gen_replay, dim3((Lpad + 255) / 256), dim3(256), 0, s, seed, n0, BL, L, Lpad, t0, n_targets,
                     round, k, out);
  return hipGetLastError();
}

namespace {
// Live valid records (optionally of honest nodes only): the convergence
// measure for rounds-to-finalization. Grid-stride, one atomic per block.
__global__ void k_count_live(const uint32_t* planes, const uint32_t* valid, const uint32_t* byz, uint32_t n0,
                             uint32_t BL, uint32_t L, int honest_only, unsigned long long* out) {
  __shared__ unsigned long long part[4];
  unsigned long long c = 0;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < L; g += gridDim.x * blockDim.x) {
    const uint32_t nl = g / BL, b = g - nl * BL;
    if (honest_only && is_byz(byz, n0 + nl)) continue;
    c += __popc(~*pw(planes, g, kPK + 7) & valid[b]);
  }
  const uint32_t w = wave_sum((uint32_t)c);  // <= 32 * 64 per wave per pass: fits u32
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}
}  // namespace

hipError_t launch_count_live(const uint32_t* planes, const uint32_t* valid, const uint32_t* byz, uint32_t n0,
                             uint32_t BL, uint32_t L, int honest_only, unsigned long long* out, hipStream_t s) {
  if (!L) return hipSuccess;
  const uint32_t blocks = std::min<uint32_t>(2048u, (L + 255u) / 256u);
  hipLaunchKernelGGL(k_count_live, dim3(blocks), dim3(256), 0, s, planes, valid, byz, n0, BL, L, honest_only, out);
  return hipGetLastError();
}

namespace {
// Batched GetInvsForNextPoll (processor.go:144-170) for local nodes
// [nl0, nl0 + gridDim.x): one 64-lane workgroup per node walks the node's
// blocks in order with a running wave prefix count of live, valid records
// (rule R1: ascending target order, at most kMaxPoll). counts != nullptr: only
// count them. Else write the poll set at out + offsets[node] (entries at or past
// cap skipped): per 64-block chunk, lane i writes the chunk's records i, i + 64,
// ... (its block by binary search over the chunk's prefix counts in LDS, its
// target by the rank-th set bit), so every store is coalesced — the output may
// be host-mapped memory written over PCIe. lane 0 of each node also writes
// offs_out[node] (and the last node offs_out[n]) as int64.
__global__ __launch_bounds__(64) void k_poll_sets(const uint32_t* planes, const uint32_t* valid, uint32_t BL,
                                                  uint32_t nl0, uint32_t t0, uint32_t* counts,
                                                  const uint64_t* offsets, uint64_t cap, int64_t* offs_out,
                                                  int32_t* out) {
  __shared__ uint32_t pre[64];
  __shared__ uint32_t bits_s[64];
  const uint32_t i = blockIdx.x, nl = nl0 + i, lane = threadIdx.x;
  const uint64_t o0 = counts ? 0ull : offsets[i];
  if (!counts && lane == 0) {
    offs_out[i] = (int64_t)o0;
    if (i == gridDim.x - 1u) offs_out[i + 1u] = (int64_t)offsets[i + 1u];
  }
  uint32_t run = 0;  // records selected so far (wave-uniform)
  for (uint32_t b0 = 0; b0 < BL && run < kMaxPoll; b0 += 64u) {
    const uint32_t b = b0 + lane;
    const uint32_t bits = b < BL ? ~*pw(planes, nl * BL + b, kPK + 7) & valid[b] : 0u;
    const uint32_t c = (uint32_t)__popc(bits);
    const uint32_t incl = wave_incl_scan(c, lane);
    const uint32_t tot = (uint32_t)__shfl((int)incl, 63, 64);
    if (!counts) {
      pre[lane] = incl - c;
      bits_s[lane] = bits;
      __syncthreads();
      const uint32_t take = min(tot, kMaxPoll - run);
      for (uint32_t q = lane; q < take; q += 64u) {
        uint32_t l0 = 0, l1 = 63;  // the last block lane whose prefix is <= q
        while (l0 < l1) {
          const uint32_t mid = (l0 + l1 + 1u) >> 1;
          if (pre[mid] <= q) l0 = mid; else l1 = mid - 1u;
        }
        uint32_t m = bits_s[l0], r = q - pre[l0], pos = 0;
#pragma unroll
        for (uint32_t w = 16; w >= 1; w >>= 1) {
          const uint32_t low = m & ((1u << w) - 1u);
          const uint32_t cl = (uint32_t)__popc(low);
          if (r >= cl) {
            r -= cl;
            m >>= w;
            pos += w;
          } else {
            m = low;
          }
        }
        const uint64_t at = o0 + run + q;
        if (at < cap) out[at] = (int32_t)(t0 + 32u * (b0 + l0) + pos);
      }
      __syncthreads();
    }
    run += tot;
  }
  if (counts && lane == 0) counts[i] = min(run, kMaxPoll);
}
}  // namespace

uint64_t poll_sets_scratch_words(uint32_t n) {
  return ((uint64_t)n + 1u) / 2u + 1u + ((uint64_t)n + 1u) + dscan::scan_scratch_words(n);
}

hipError_t launch_poll_sets_batch(const uint32_t* planes, const uint32_t* valid, uint32_t BL, uint32_t nl0,
                                  uint32_t n, uint32_t t0, uint64_t cap, uint64_t* scratch, int64_t* offs_out,
                                  int32_t* targets_out, hipStream_t s) {
  if (!n) return hipSuccess;
  uint32_t* counts = reinterpret_cast<uint32_t*>(scratch);
  uint64_t* offs = scratch + ((uint64_t)n + 1u) / 2u + 1u;
  uint64_t* sc = offs + (uint64_t)n + 1u;
  hipLaunchKernelGGL(k_poll_sets, dim3(n), dim3(64), 0, s, planes, valid, BL, nl0, t0, counts,
                     (const uint64_t*)nullptr, (uint64_t)0, (int64_t*)nullptr, (int32_t*)nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = dscan::launch_scan(dscan::In32{counts}, n, offs, sc, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_poll_sets, dim3(n), dim3(64), 0, s, planes, valid, BL, nl0, t0, (uint32_t*)nullptr,
                     (const uint64_t*)offs, cap, offs_out, targets_out);
  return hipGetLastError();
}

}  // namespace avk
