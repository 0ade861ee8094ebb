// First-generation round kernels of the batched Avalanche voting engine (CDNA4,
// gfx950): one lane per 32-record block (k_round_fast), the exact capped round
// (k_round_capped, also the exact pass behind round_node.hip) and the example
// responder's re-adds (k_readd). k = 1..16; the engine's default rounds run in
// round_sweep.hip (k <= 8).
//
// A round is one turn of go-avalanche's poll loop for every simulated node at
// once, here as in round_sweep.hip: peer sampling (processor.go:173-182 / main.go:110-116 replaced
// by a counter-RNG k-peer draw), the peer-preference gather (main.go:168-192
// responder), the VoteRecord shift-register / confidence update
// (vote.go:54-91) inside RegisterVotes (processor.go:92-117) and StatusUpdate
// emission (processor.go:111) with deletion on finalization (:114-116).
//
// Records are bit-sliced: one lane owns 32 records (a block of 32 targets of
// one node) as 25 u32 planes, so every VALU instruction advances 32
// VoteRecords. Nothing here is a dense contraction; there is no MFMA. The
// kernels are HBM-bound streaming kernels (DESIGN.md "Roofline").
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "round_common.h"

namespace avk {

namespace {
// ---------------------------------------------------------------------------
// Body of the uncapped round kernel for one lane (one 32-record block).
// WARM (sim mode only): every consider plane of the wave's blocks is all-ones
// (each record has seen >= 8 votes and, with no replay / neutral vote ever
// applied in this engine, every consider bit shifted in was 1). Then the 7
// younger consider planes are neither loaded nor stored: 176 B per lane
// instead of 236 B at k=8. NT: non-temporal plane stream.
// ---------------------------------------------------------------------------
template <int K, bool REPLAY, bool WARM, bool NT>
__device__ __forceinline__ void round_fast_body(const RoundParams& p, uint32_t g, uint32_t lane, bool active,
                                                uint32_t b, uint32_t node) {
  St s;
  uint32_t* const tile = tile_of(p.planes, g);
  u32x4* const grp = reinterpret_cast<u32x4*>(tile) + lane;  // V0-3, V4-7, K0-3, K4-7 at +0, +64, +128, +192
  if (!active) {
    dead_state(s);
  } else {
    const u32x4 v0 = pld4<NT>(grp), v1 = pld4<NT>(grp + 64), k0 = pld4<NT>(grp + 128), k1 = pld4<NT>(grp + 192);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.V[i] = v0[i];
      s.V[4 + i] = v1[i];
      s.K[i] = k0[i];
      s.K[4 + i] = k1[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s.C[i] = WARM ? ~0u : pld<NT>(tile + plane_off(kPC + i, lane));
    s.A = pld<NT>(tile + plane_off(kPA, lane));
  }

  uint32_t w[K], cw[K], peer_of[K];
  if (REPLAY) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      w[j] = active ? p.replay[replay_idx(g, K, j, 0)] : 0u;
      cw[j] = active ? p.replay[replay_idx(g, K, j, 1)] : 0u;
    }
  } else {
    uint32_t peers[K];
    sample_peers<K>(p.seed, node, p.round, p.n_nodes, p.peer_mode, peers);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      // peer's published preference; the ablation (timing diagnostics only,
      // results invalid) reads the node's own row instead: coalesced, same count
      const uint32_t src = p.ablate_gather ? (node ^ (uint32_t)j) % p.n_nodes : peers[j];
      w[j] = active ? p.pref_in[(size_t)src * p.PS + b] : 0u;
      cw[j] = ~0u;  // honest/Byzantine votes are 0 or 1
      peer_of[j] = src - p.n0;  // local row of the peer (responder re-adds: single-engine networks only)
    }
  }
  const uint32_t vmask = active ? p.valid[b] : 0u;
  const uint32_t live0 = ~s.K[7];
  // a node whose run loop has returned (main.go:160-162) polls nothing
  const uint32_t nl = g / p.BL;
  const bool polls = !p.nopoll || !((p.nopoll[nl >> 5] >> (nl & 31u)) & 1u);
  const uint32_t P0 = polls ? live0 & vmask : 0u;

  uint32_t alive = P0, applied = 0, E[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    applied += __popc(alive);
    // the example's responder re-adds what it is queried for (main.go:175-177)
    if (!REPLAY && p.readd && alive) atomicOr(&p.readd[peer_of[j] * p.BL + b], alive);
    uint32_t fin;
    vote_step<false>(s, w[j], cw[j], alive, E[j], fin);
    alive &= ~fin;
  }
  const uint32_t died = P0 & ~alive;
  const uint32_t keep = live0 & ~P0;  // live but !IsValid() (processor.go:101-103) or not polling: untouched
  if (p.died_out && active) p.died_out[g] = died;

  if (active) {
    uint32_t Vo[8], Co[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) Vo[i] = Co[i] = 0u;
    if (keep) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        Vo[i] = tile[plane_off(kPV + i, lane)];
        if (!WARM) Co[i] = tile[plane_off(kPC + i, lane)];
      }
    }
    const uint32_t dead = ~(alive | keep);
    u32x4 v0, v1, k0, k1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v0[i] = (s.V[i] & alive) | (Vo[i] & keep);
      v1[i] = (s.V[4 + i] & alive) | (Vo[4 + i] & keep);
      k0[i] = s.K[i];
      k1[i] = s.K[4 + i];
    }
    pst4<NT>(grp, v0);
    pst4<NT>(grp + 64, v1);
    pst4<NT>(grp + 128, k0);
    pst4<NT>(grp + 192, k1);
    if (!WARM) {  // WARM: consider planes stay all-ones (dead records are canonical all-ones too)
#pragma unroll
      for (int i = 0; i < 8; ++i) pst<NT>(tile + plane_off(kPC + i, lane), (s.C[i] & alive) | (Co[i] & keep) | dead);
    }
    pst<NT>(tile + plane_off(kPA, lane), s.A);
    p.pref_out[(size_t)node * p.PS + b] =
        is_byz(p.byz, node) ? byz_pattern(p.round + 1u) : publish_word(s.A, s.K[7], p.pub_mode);
  }
  const uint32_t wave_id = g >> 6;
  uint32_t upd = 0;
  const uint32_t emitted = emit_updates<K>(p, wave_id, lane, node, p.t0 + b * 32u, E, s.A, died, upd);
  constexpr uint32_t plane_bytes = WARM ? (18u + 17u) * 4u : 2u * kPlanes * 4u;
  constexpr uint32_t bytes = plane_bytes + (REPLAY ? 8u : 4u) * K + 4u;
  count_stats(p, wave_id, lane, applied, active, bytes, emitted, upd, died);
}

// ---------------------------------------------------------------------------
// Round kernel, uncapped path (every node has <= 4096 live valid targets, so
// GetInvsForNextPoll never truncates: processor.go:165-167). One lane = one
// 32-record block; no cross-lane dependence except the emission scan.
// ---------------------------------------------------------------------------
template <int K, bool REPLAY>
__global__ __launch_bounds__(256) void k_round_fast(const RoundParams p) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  if ((g & ~63u) >= p.L) return;  // whole wave beyond the last tile
  const bool active = g < p.L;
  const uint32_t nl = active ? g / p.BL : 0u;
  const uint32_t b = active ? g - nl * p.BL : 0u;
  const uint32_t node = p.n0 + nl;
  if (!REPLAY && p.warm_skip) {
    const uint32_t c7 = active ? *pw(p.planes, g, kPC + 7) : ~0u;
    if (__all(c7 == ~0u)) {  // wave-uniform
      if (p.plane_nt)
        round_fast_body<K, false, true, true>(p, g, lane, active, b, node);
      else
        round_fast_body<K, false, true, false>(p, g, lane, active, b, node);
      return;
    }
  }
  if (p.plane_nt)
    round_fast_body<K, REPLAY, false, true>(p, g, lane, active, b, node);
  else
    round_fast_body<K, REPLAY, false, false>(p, g, lane, active, b, node);
}

// ---------------------------------------------------------------------------
// Round kernel, capped path: one workgroup per node; per slot a workgroup
// prefix count of live valid records selects the first 4096 in ascending
// target order (GetInvsForNextPoll truncation, processor.go:165-167).
// ---------------------------------------------------------------------------
template <int K, bool REPLAY>
__device__ __forceinline__ void capped_node(const RoundParams& p, uint32_t nl, uint32_t (&wsum)[2][16]);

template <int K, bool REPLAY>
__global__ __launch_bounds__(1024) void k_round_capped(const RoundParams p) {
  __shared__ uint32_t wsum[2][16];
  if (!p.node_flags) {
    capped_node<K, REPLAY>(p, blockIdx.x, wsum);
    return;
  }
  // exact pass behind k_round_node: a small grid walks the nodes and takes
  // only the ones it flagged (an almost empty pass costs ~1-2 us, not the
  // dispatch of one workgroup per node)
  for (uint32_t nl = blockIdx.x; nl < p.NL; nl += gridDim.x) {
    const uint32_t f = p.node_flags[nl];  // workgroup-uniform
    if (f == 0u || f - 1u > p.exact_rel) continue;
    __syncthreads();
    if (threadIdx.x == 0 && !p.exact_keep) p.node_flags[nl] = 0u;
    capped_node<K, REPLAY>(p, nl, wsum);
    __syncthreads();  // wsum reuse by the next node
  }
}

template <int K, bool REPLAY>
__device__ __forceinline__ void capped_node(const RoundParams& p, uint32_t nl, uint32_t (&wsum)[2][16]) {
  const uint32_t b = threadIdx.x;
  const uint32_t lane = b & 63u, wave = b >> 6;
  const bool active = b < p.BL;
  const uint32_t g = nl * p.BL + b;
  const uint32_t node = p.n0 + nl;

  St s;
  if (active)
    load_state(p.planes, g, s);
  else
    dead_state(s);
  uint32_t w[K], cw[K];
  if (REPLAY) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      w[j] = active ? p.replay[replay_idx(g, K, j, 0)] : 0u;
      cw[j] = active ? p.replay[replay_idx(g, K, j, 1)] : 0u;
    }
  } else {
    uint32_t peers[K];
    sample_peers<K>(p.seed, node, p.round, p.n_nodes, p.peer_mode, peers);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      w[j] = active ? p.pref_in[(size_t)peers[j] * p.PS + b] : 0u;
      cw[j] = ~0u;
    }
  }
  const uint32_t vmask = active ? p.valid[b] : 0u;
  const uint32_t P0 = ~s.K[7] & vmask;

  uint32_t alive = P0, applied = 0, E[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t c = __popc(alive);
    const uint32_t incl = wave_incl_scan(c, lane);
    if (lane == 63u) wsum[j & 1][wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t q = 0; q < wave; ++q) before += wsum[j & 1][q];
    const uint32_t excl = before + incl - c;
    uint32_t polled;
    if (excl >= kMaxPoll) {
      polled = 0u;
    } else if (excl + c <= kMaxPoll) {
      polled = alive;
    } else {  // keep the lowest (4096 - excl) set bits
      uint32_t x = alive;
      polled = 0u;
      for (uint32_t q = 0; q < kMaxPoll - excl; ++q) {
        const uint32_t low = x & (0u - x);
        polled |= low;
        x ^= low;
      }
    }
    applied += __popc(polled);
    uint32_t fin;
    vote_step<true>(s, w[j], cw[j], polled, E[j], fin);
    alive &= ~fin;
  }
  const uint32_t died = P0 & ~alive;
  if (active) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s.V[i] &= ~died;
      s.C[i] |= died;
    }
    store_state(p.planes, g, s);
    p.pref_out[(size_t)node * p.PS + b] =
        is_byz(p.byz, node) ? byz_pattern(p.round + 1u) : publish_word(s.A, s.K[7], p.pub_mode);
  }
  const uint32_t wave_id = nl * (blockDim.x >> 6) + wave;  // dense: matches log_shards sizing
  uint32_t upd = 0;
  const uint32_t emitted = emit_updates<K>(p, wave_id, lane, node, p.t0 + b * 32u, E, s.A, died, upd);
  count_stats(p, wave_id, lane, applied, active, 2u * kPlanes * 4u + (REPLAY ? 8u : 4u) * K + 4u, emitted, upd,
              died);
}

template <int K>
hipError_t launch_round_k(const RoundParams& p, bool replay, bool capped, hipStream_t s) {
  if (capped) {
    const uint32_t bt = ((p.BL + 63u) / 64u) * 64u;
    const uint32_t grid = p.node_flags ? std::min(p.NL, 128u) : p.NL;
    if (replay)
      hipLaunchKernelGGL((k_round_capped<K, true>), dim3(grid), dim3(bt), 0, s, p);
    else
      hipLaunchKernelGGL((k_round_capped<K, false>), dim3(grid), dim3(bt), 0, s, p);
  } else {
    const uint32_t blocks = (p.Lpad + 255u) / 256u;
    if (replay)
      hipLaunchKernelGGL((k_round_fast<K, true>), dim3(blocks), dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL((k_round_fast<K, false>), dim3(blocks), dim3(256), 0, s, p);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t launch_round(const RoundParams& p, int k, bool replay, bool capped, hipStream_t s) {
  return dispatch_k<kMaxK>(k, [&](auto K) { return launch_round_k<K()>(p, replay, capped, s); });
}

namespace {
// The example's responder (main.go:175-177), after a round: every record a
// node was queried for (readd, OR of the querying lanes' polled masks) and
// did not hold at the round start (no record now, not deleted this round) is
// re-created as AddTargetToReconcile(&tx{isAccepted: true}) (processor.go:
// 45-58, valid targets only): votes, consider and count zero, accepted.
__global__ __launch_bounds__(256) void k_readd(const RoundParams p) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.L) return;
  const uint32_t q = p.readd[g];
  if (!q) return;
  p.readd[g] = 0u;
  const uint32_t b = g % p.BL;
  const uint32_t m = q & *pw(p.planes, g, kPK + 7) & ~p.died_out[g] & p.valid[b];
  if (!m) return;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    *pw(p.planes, g, kPV + i) &= ~m;
    *pw(p.planes, g, kPC + i) &= ~m;
    *pw(p.planes, g, kPK + i) &= ~m;
  }
  *pw(p.planes, g, kPA) |= m;
}
}  // namespace

hipError_t launch_readd(const RoundParams& p, hipStream_t s) {
  if (!p.readd || !p.died_out || !p.L) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_readd, dim3((p.L + 255) / 256), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace avk
