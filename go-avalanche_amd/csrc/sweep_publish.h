// The sweep kernel's publish path (k_round_sweep, sweep_kernel.h): a wave's counters (SweepAcc), the
// published word of a lane into pref_out with the peer-push exchange behind it (publish, push_word,
// flush_pushes) and the reference-row flags (ref_tag, ref_flag_store). Included by the sweep
// translation units only; reads no build knob (AVK_PUB_PRELOAD is read by publish's caller, sweep_tile.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "round_common.h"

namespace avk {
namespace {

struct SweepAcc {
  uint32_t applied = 0, died = 0, lane_bytes = 0;
  uint32_t reread = 0;  // per lane: gathered preference bytes beyond the one compulsory read of each word
  uint32_t emitted_bytes = 0, updates = 0;  // wave-uniform: StatusUpdate log bytes written, updates emitted
  uint32_t umis = 0;  // per lane: some published word differed from ref_node's word of pref_in (p.uni_out)
  // wave-uniform (p.count_changed): published words that differ from the word they overwrite, and the
  // 16-lane groups holding one (64-B row segments when PS == BL, a multiple of 16); two scalars, so
  // that a wave walking many tiles (a small grid) cannot carry one count into the other
  uint32_t changed = 0, changed_segs = 0;
  uint32_t pushed = 0;  // wave-uniform: words stored into peer replicas (all peers)
  // deferred pushes (p.push_q): the wave's queue in LDS, slot = the tile's place in the wave's tiles
  uint32_t* qpub = nullptr;
  uint8_t* qpm = nullptr;
  uint32_t qslot = 0;
  uint32_t shard = 0;  // wave-uniform: this wave's log / counter shard (wave index % log_shards)
};

// Peer r's replica pointer from the engine's device table: a scalar load through the constant address
// space (the table is written once at av_peer_init), so a pushing lane issues no vector load and its
// wave no vmcnt drain.
__device__ __forceinline__ uint32_t* peer_ptr(uint32_t* const* tbl, uint32_t r) {
  using cptr = __attribute__((address_space(4))) const uint64_t*;
  const cptr t = (cptr)(tbl);
  return reinterpret_cast<uint32_t*>(t[__builtin_amdgcn_readfirstlane((int)r)]);
}

// One word into a peer's replica (p.push_store): 1 = a plain store (default: the round kernel's
// completion releases it at system scope before the barrier kernel that follows it on the stream runs,
// which orders it for the peer; measured far cheaper to issue than the scoped form), 0 = a system-scope
// store (the first form), 2 = none (diagnostics: the exchange's stores ablated, results invalid).
__device__ __forceinline__ void push_word(const RoundParams& p, uint32_t* dst, uint32_t v) {
  if (p.push_store == 1u)
    *dst = v;
  else if (p.push_store == 0u)
    __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The published word of one lane into pref_out. In a peer-push round the word being overwritten is
// what every peer replica holds (kernels.h), so only a changed word is stored into each replica
// (system-scope write-through stores over xGMI; the barrier after the round orders them before any
// peer reads them). Changed words are counted when p.count_changed (the push volume),
// per wave by ballot (a scalar: a per-lane counter live across the tile loop spilled).
// `old`: the overwritten word when the caller knows it (`known`: implied by the tile's history,
// below); else it is loaded here, or ahead by the caller (`pre`, AVK_PUB_PRELOAD).
// A tile whose count steps were deferred in the two rounds before this one (kpend >= 2) kept its
// accepted plane through them, so an honest row it publishes unchanged this round equals the
// snapshot being overwritten (written three rounds ago): no load, no push; a Byzantine row's word
// there is the pattern of that snapshot.
// Need-masked exchange (p.stale, kernels.h): peer i gets this lane's word if one of its nodes draws
// the row next round (need bit i) and either the word changed or peer i's copy of the segment may
// differ (stale bit i: a change it did not need was withheld earlier); a withheld change marks the
// segment stale for that peer, a push to it clears the mark. The segment's bits are decided per wave
// (any changed word of the wave: a superset, so a mark is never lost; a segment never straddles a
// wave), so every lane of a segment stores the same byte.
// Deferred pushes (p.push_q): the peers a lane's word goes to (bit i: peer i) and the word are queued
// in LDS and stored after the wave's last tile (flush_pushes), so that no load of a later tile waits
// for them (vmcnt counts loads and stores in issue order, and a system-scope store to a peer completes
// only at the peer: pushed from inside the tile loop, every tile waited for the last one's pushes).
// The loads publish() needs (the overwritten word, the segment's stale byte, the node's need byte),
// issued by the caller before the tile's plane stores: vmcnt counts loads and stores in issue order,
// so loads issued after the stores would make the tile wait for the stores' completion too (a round
// trip per tile in every peer-push round; the stale and need bytes exist on need-masked engines only).
struct PubPre {
  uint32_t old, st, nm;
  bool have;
};
__device__ __forceinline__ PubPre publish_loads(const RoundParams& p, uint32_t prow, uint32_t nl) {
  PubPre q{0u, 0u, p.peer_all, true};
  q.old = p.pref_out[prow];
  if (p.stale) {
    q.st = p.stale[nl * p.segs + ((prow - (p.n0 + nl) * p.PS) >> 5)];
    if (p.need) q.nm = (uint32_t)p.need[nl];
  }
  return q;
}

template <int POL, bool CC>
__device__ __forceinline__ void publish(const RoundParams& p, uint32_t prow, uint32_t pub, uint32_t old,
                                        SweepAcc& acc, bool known, uint32_t nl, uint32_t slot,
                                        const PubPre* pre = nullptr) {
  if (CC && p.count_changed) {
    const bool pl = pre && pre->have;  // loaded ahead (an unknown word only)
    if (!known) old = pl ? pre->old : p.pref_out[prow];
    uint32_t nm = p.peer_all, st = 0u, si = 0u;
    if (p.stale) {
      si = nl * p.segs + ((prow - (p.n0 + nl) * p.PS) >> 5);
      st = pl ? pre->st : p.stale[si];
      // a word known unchanged (a settled tile) goes out only where a change was withheld: the need
      // mask is read only then (settled rounds after the catch-up read one byte per lane, not two)
      if (p.need && (!known || __ballot(st != 0u) != 0ull)) nm = pl ? pre->nm : (uint32_t)p.need[nl];
    }
    const unsigned long long m = __ballot(pub != old);
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    const uint32_t groups = ((lo & 0xFFFFu) ? 1u : 0u) + ((lo >> 16) ? 1u : 0u) + ((hi & 0xFFFFu) ? 1u : 0u) + ((hi >> 16) ? 1u : 0u);
    acc.changed += (uint32_t)__popcll(m);
    acc.changed_segs += groups;
    if (p.push_q) {
      const uint32_t push = p.stale ? nm & (pub != old ? p.peer_all : st) : (pub != old ? p.peer_all : 0u);
      const uint32_t lane = __lane_id();
      acc.qpm[slot * 64u + lane] = (uint8_t)push;
      if (push) acc.qpub[slot * 64u + lane] = pub;  // (read only where pm != 0; counted by flush_pushes)
      if (p.stale) {
        const uint32_t nst = (st | (m ? p.peer_all : 0u)) & ~nm;
        if (nst != st) p.stale[si] = (uint8_t)nst;
      }
    } else if (p.stale) {
      const uint32_t push = nm & (pub != old ? p.peer_all : st);
      for (uint32_t r = 0; r < p.push_n; ++r) {
        const bool go = (push >> r) & 1u;
        if (go) push_word(p, peer_ptr(p.push_dst, r) + prow, pub);
        acc.pushed += (uint32_t)__popcll(__ballot(go));
      }
      const uint32_t nst = (st | (m ? p.peer_all : 0u)) & ~nm;
      if (nst != st) p.stale[si] = (uint8_t)nst;
    } else {
      if (pub != old)
        for (uint32_t r = 0; r < p.push_n; ++r)
          push_word(p, peer_ptr(p.push_dst, r) + prow, pub);
      acc.pushed += (uint32_t)__popcll(m) * p.push_n;
    }
  }
  const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(p.pref_out, 0, (int)0xFFFFFFFFu, kRsrcWord3);
  st1<POL>(pr, p.pref_out + prow, prow * 4u, pub);
}

// The queued pushes of a wave's tiles (p.push_q): tile first + s * step for queue slot s < n. The peer
// pointers are read once; the stores are the wave's last memory instructions, back to back.
__device__ __forceinline__ uint32_t flush_pushes(const RoundParams& p, uint32_t lane, uint32_t first, uint32_t step,
                                                 uint32_t n, const uint32_t* qpub, const uint8_t* qpm) {
  uint32_t* dst[8];
#pragma unroll
  for (uint32_t r = 0; r < 8u; ++r) dst[r] = r < p.push_n ? peer_ptr(p.push_dst, r) : nullptr;
  uint32_t words = 0u;  // this lane's pushed words (returned: the caller sums the wave once)
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t g = (first + s * step) * 64u + lane;
    const uint32_t pm = g < p.L ? (uint32_t)qpm[s * 64u + lane] : 0u;
    words += (uint32_t)__popc(pm);
    if (pm == 0u) continue;
    const uint32_t pub = qpub[s * 64u + lane];
    const uint32_t nl = div_bl(p, g);
    const uint32_t prow = (p.n0 + nl) * p.PS + (g - nl * p.BL);
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r)
      if ((pm >> r) & 1u) push_word(p, dst[r] + prow, pub);
  }
  return words;
}

// Reference-row flag of the node whose lanes include this one (kernels.h
// rflag_out): every lane of the node published REF's word. BL divides 64, so
// the node's lanes are the aligned BL-lane segment of this wave that holds
// the lane; the node's block-0 lane stores the byte (and pushes it to the
// peers' replicas when it changed, as the published words). The byte is the
// snapshot's tag (ref_tag) when the row equals the reference row, else 0; a
// reader trusts only its own snapshot's tag, so flags are written by settled
// tiles only and every other byte (older snapshots' tags, 0) reads as "gather".
__device__ __forceinline__ uint8_t ref_tag(uint32_t snapshot_round) { return (uint8_t)(0x80u | (snapshot_round & 0x7Fu)); }

__device__ __forceinline__ void ref_flag_store(const RoundParams& p, uint32_t lane, bool active, uint32_t b,
                                               uint32_t node, uint32_t pub, uint32_t ref) {
  const uint64_t eq = __ballot(!active || pub == ref);
  const uint32_t s0 = lane - b;  // the node's first lane (active lanes only)
  const uint64_t seg = (p.BL >= 64u ? ~0ull : ((1ull << p.BL) - 1ull)) << (s0 & 63u);
  if (active && b == 0u) {
    const uint8_t f = (eq & seg) == seg ? ref_tag(p.round + 1u) : 0u;  // pref_out = snapshot round + 1
    if (p.push_n && p.rflag_out[node] != f) {
      for (uint32_t r = 0; r < p.push_n; ++r)
        __hip_atomic_store(reinterpret_cast<uint8_t*>(peer_ptr(p.push_dst, r)) + p.rflag_off + node, f, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    p.rflag_out[node] = f;
  }
}

}  // namespace
}  // namespace avk
