// The drop-in Processor calls on the device (CDNA4, gfx950): RegisterVotes for
// one Response or a batch (k_register_votes; k_dropin_resp when every Response's
// targets ascend, else k_dropin_keys and the stable grouping of the votes by
// lane, launch_group_votes, with the radix sort and scan of dev_scan.h) and
// AddTargetToReconcile (k_add_targets). Each launcher sits below its kernels.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev_scan.h"
#include "kernels.h"
#include "round_common.h"

namespace avk {

namespace {
// ---------------------------------------------------------------------------
// Drop-in RegisterVotes for one node (processor.go:61-122): one thread per
// touched block applies that block's votes in Response order, so duplicate
// hashes in one Response apply sequentially. Status per vote position. One
// thread per touched lane (node, 32-target block) of any number of nodes
// (av_register_votes_batch): a node's Responses apply one after the other.
// ---------------------------------------------------------------------------
__global__ void k_register_votes(const DropInParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_blocks) return;
  const uint32_t g = p.blocks[i];  // lane: local node * BL + block
  if (g >= p.L) return;            // the run of votes for unknown targets: no update (status -1)
  const uint32_t nl = g / p.BL, b = g - nl * p.BL;
  const uint32_t node = p.n0 + nl;
  St s;
  load_state(p.planes, g, s);
  const uint32_t vmask = p.valid[b];
  uint32_t died = 0;
  for (uint32_t e = p.offs[i]; e < p.offs[i + 1]; ++e) {
    const uint32_t pos = p.entries[2 * e];
    const uint32_t meta = p.entries[2 * e + 1];
    const uint32_t m = 1u << (meta & 31u);
    const uint32_t part = ~s.K[7] & vmask & m;  // skip unknown/deleted (:95-99) and invalid (:101-103)
    uint32_t E, fin;
    vote_step<true>(s, (meta >> 5) & 1u ? m : 0u, (meta >> 6) & 1u ? m : 0u, part, E, fin);
    died |= fin;
    int32_t st = -1;
    if (E & m) st = (fin & m) ? ((s.A & m) ? 3 : 0) : ((s.A & m) ? 2 : 1);
    p.status_out[pos] = (int8_t)st;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    s.V[q] &= ~died;
    s.C[q] |= died;
  }
  store_state(p.planes, g, s);
  p.pref[(size_t)node * p.PS + b] =
      is_byz(p.byz, node) ? byz_pattern(p.round) : publish_word(s.A, s.K[7], p.pub_mode);
}
}  // namespace

hipError_t launch_register_votes(const DropInParams& p, hipStream_t s) {
  if (!p.n_blocks) return hipSuccess;
  hipLaunchKernelGGL(k_register_votes, dim3((p.n_blocks + 63) / 64), dim3(64), 0, s, p);
  return hipGetLastError();
}

namespace {
// av_register_votes_batch, fast path: every Response's targets strictly
// ascending. A Response's votes for one (node, 32-target block) lane are then
// consecutive and in order, and the run's first vote is the one whose
// predecessor is in another block: one thread per run applies it (<= 32
// votes) exactly as k_register_votes does, with no sort. One workgroup per
// node (grid-stride over nodes): its Responses apply one after the other
// (processor.go:61-122 per Response, in call order). A Response is walked in
// chunks of kDropChunk votes: the chunk's run heads are collected in LDS, then
// the workgroup's threads take one run each (a run may reach into the next
// chunk; its head is in this one).
constexpr uint32_t kDropChunk = 4096;

__device__ __forceinline__ void dropin_run(const DropInParams& p, uint32_t v, uint32_t o1, uint32_t nl, uint32_t node) {
  const uint32_t blk = (p.packed[v] & kDropTl) >> 5;
  const uint32_t g = nl * p.BL + blk;
  St s;
  load_state(p.planes, g, s);
  const uint32_t vmask = p.valid[blk];
  uint32_t died = 0;
  for (uint32_t u = v; u < o1; ++u) {
    const uint32_t x = p.packed[u];
    if ((x & kDropUnknown) || ((x & kDropTl) >> 5) != blk) break;
    const uint32_t m = 1u << (x & 31u);
    const uint32_t part = ~s.K[7] & vmask & m;  // skip deleted (:95-99) and invalid (:101-103)
    uint32_t E, fin;
    vote_step<true>(s, (x & kDropYes) ? m : 0u, (x & kDropCons) ? m : 0u, part, E, fin);
    died |= fin;
    int32_t st = -1;
    if (E & m) st = (fin & m) ? ((s.A & m) ? 3 : 0) : ((s.A & m) ? 2 : 1);
    p.status_out[u] = (int8_t)st;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    s.V[q] &= ~died;
    s.C[q] |= died;
  }
  store_state(p.planes, g, s);
  p.pref[(size_t)node * p.PS + blk] = is_byz(p.byz, node) ? byz_pattern(p.round) : publish_word(s.A, s.K[7], p.pub_mode);
}

__global__ __launch_bounds__(256) void k_dropin_resp(const DropInParams p) {
  __shared__ uint32_t heads[kDropChunk];
  __shared__ uint32_t nheads;
  for (uint32_t gi = blockIdx.x; gi < p.n_groups; gi += gridDim.x) {
    for (uint32_t k = p.grp_off[gi]; k < p.grp_off[gi + 1]; ++k) {
      const uint32_t r = p.order[k];
      const uint32_t o0 = p.resp_off[r], o1 = p.resp_off[r + 1];
      const uint32_t nl = p.resp_node[r], node = p.n0 + nl;
      for (uint32_t c0 = o0; c0 < o1; c0 += kDropChunk) {
        const uint32_t c1 = min(o1, c0 + kDropChunk);
        if (threadIdx.x == 0) nheads = 0u;
        __syncthreads();
        for (uint32_t v = c0 + threadIdx.x; v < c1; v += blockDim.x) {
          const uint32_t w = p.packed[v];
          if (w & kDropUnknown) continue;
          if (v > o0) {
            const uint32_t q = p.packed[v - 1u];
            if (!(q & kDropUnknown) && ((q ^ w) & kDropTl) >> 5 == 0u) continue;  // inside a run
          }
          heads[atomicAdd(&nheads, 1u)] = v;
        }
        __syncthreads();
        const uint32_t nh = nheads;
        for (uint32_t h = threadIdx.x; h < nh; h += blockDim.x) dropin_run(p, heads[h], o1, nl, node);
        __syncthreads();  // heads reused; the node's next Response sees this one's records
      }
    }
  }
}
}  // namespace

hipError_t launch_dropin_resp(const DropInParams& p, hipStream_t s) {
  if (!p.n_resp) return hipSuccess;
  hipLaunchKernelGGL(k_dropin_resp, dim3(std::min<uint32_t>(p.n_groups, 65535u)), dim3(256), 0, s, p);
  return hipGetLastError();
}

namespace {
// General path: one workgroup per Response writes each vote's lane key (L for
// an unknown target), its index and its packed (bit | yes << 5 | considered << 6)
// for the stable radix grouping (launch_group_votes below).
__global__ __launch_bounds__(256) void k_dropin_keys(const DropInParams p, uint32_t* keys, uint32_t* vidx,
                                                     uint32_t* info) {
  for (uint32_t r = blockIdx.x; r < p.n_resp; r += gridDim.x) {
    const uint32_t o0 = p.resp_off[r], o1 = p.resp_off[r + 1];
    const uint32_t nl = p.resp_node[r];
    for (uint32_t v = o0 + threadIdx.x; v < o1; v += blockDim.x) {
      const uint32_t w = p.packed[v];
      const uint32_t tl = w & kDropTl;
      keys[v] = (w & kDropUnknown) ? p.L : nl * p.BL + (tl >> 5);
      vidx[v] = v;
      info[v] = (tl & 31u) | ((w & kDropYes) ? 1u << 5 : 0u) | ((w & kDropCons) ? 1u << 6 : 0u);
    }
  }
}
}  // namespace

hipError_t launch_dropin_keys(const DropInParams& p, uint32_t* keys, uint32_t* vidx, uint32_t* info, hipStream_t s) {
  if (!p.n_resp) return hipSuccess;
  hipLaunchKernelGGL(k_dropin_keys, dim3(std::min<uint32_t>(p.n_resp, 65535u)), dim3(256), 0, s, p, keys, vidx, info);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Drop-in RegisterVotes batch (engine_records.cpp av_register_votes_batch): group the votes by lane (node,
// 32-target block) keeping their order inside a lane — the stable radix sort of (lane, position) —
// then run-length encode the sorted lanes into the (lanes, offs) CSR k_register_votes walks.
// ---------------------------------------------------------------------------
namespace {
struct HeadsIn {
  const uint32_t* k;
  __device__ uint64_t operator()(uint64_t i) const { return (i == 0 || k[i] != k[i - 1]) ? 1u : 0u; }
};
// run r of the sorted keys: lanes[r] = its key, offs[r] = its first position; offs[n_runs] = n
__global__ __launch_bounds__(256) void k_rle_write(const uint32_t* ks, const uint64_t* run_of, uint32_t n,
                                                   uint32_t* lanes, uint32_t* offs, uint32_t* n_runs) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  if (i == 0 || ks[i] != ks[i - 1]) {
    const uint32_t r = (uint32_t)run_of[i];
    lanes[r] = ks[i];
    offs[r] = i;
  }
  if (i == n - 1u) {
    const uint32_t nr = (uint32_t)run_of[n];
    offs[nr] = n;
    *n_runs = nr;
  }
}
// entries[2i] = vote index, entries[2i+1] = packed vote (k_register_votes)
__global__ __launch_bounds__(256) void k_vote_entries(const uint32_t* perm, const uint32_t* vidx, const uint32_t* info,
                                                      uint32_t n, uint32_t* entries) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = perm[i];
  entries[2u * i] = vidx[j];
  entries[2u * i + 1u] = info[j];
}
}  // namespace

uint64_t group_votes_scratch_words(uint32_t n) {
  return std::max<uint64_t>(dscan::radix_scratch_words(n), (uint64_t)n + 1u + dscan::scan_scratch_words((uint64_t)n + 1u));
}

hipError_t launch_group_votes(uint64_t* scratch, const uint32_t* keys, const uint32_t* vidx, const uint32_t* info,
                              uint32_t n, int key_bits, uint32_t* keys_s, uint32_t* perm_s, uint32_t* keys_t,
                              uint32_t* perm_t, uint32_t* lanes, uint32_t* offs, uint32_t* n_runs, uint32_t* entries,
                              hipStream_t s) {
  if (n == 0) return hipMemsetAsync(n_runs, 0, 4, s);
  hipError_t e = dscan::launch_radix_sort_pairs(keys, nullptr, n, key_bits, keys_s, perm_s, keys_t, perm_t, scratch, s);
  if (e != hipSuccess) return e;
  // run index of every position: exclusive scan of the run heads (run_of[n] = runs)
  uint64_t* run_of = scratch;
  if ((e = dscan::launch_scan(HeadsIn{keys_s}, n, run_of, scratch + n + 1u, s)) != hipSuccess) return e;
  const uint32_t g = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_rle_write, dim3(g), dim3(256), 0, s, (const uint32_t*)keys_s, (const uint64_t*)run_of, n,
                     lanes, offs, n_runs);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_vote_entries, dim3(g), dim3(256), 0, s, (const uint32_t*)perm_s, vidx, info, n, entries);
  return hipGetLastError();
}

namespace {
// AddTargetToReconcile (processor.go:45-58) for a list of targets of one
// node, applied sequentially by one thread (duplicates return false).
__global__ void k_add_targets(const AddParams p) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (uint32_t i = 0; i < p.n; ++i) {
    const uint32_t t = p.targets[i];
    const uint32_t b = t >> 5, m = 1u << (t & 31u);
    const uint32_t g = p.node_local * p.BL + b;
    const bool valid = (p.valid[b] & m) != 0u;               // isWorthyPolling (:46-48)
    const bool exists = (*pw(p.planes, g, kPK + 7) & m) == 0u;  // record present (:50-53)
    if (!valid || exists) {
      p.added[i] = 0;
      continue;
    }
    for (int q = 0; q < 8; ++q) {  // NewVoteRecord(t.IsAccepted()) (vote.go:33-35)
      *pw(p.planes, g, kPV + q) &= ~m;
      *pw(p.planes, g, kPC + q) &= ~m;
      *pw(p.planes, g, kPK + q) &= ~m;
    }
    uint32_t* a = pw(p.planes, g, kPA);
    *a = p.accepted[i] ? (*a | m) : (*a & ~m);
    p.added[i] = 1;
    p.pref[(size_t)p.node * p.PS + b] = is_byz(p.byz, p.node) ? byz_pattern(p.round)
                                                               : publish_word(*a, *pw(p.planes, g, kPK + 7), p.pub_mode);
  }
}
}  // namespace

hipError_t launch_add_targets(const AddParams& p, hipStream_t s) {
  if (!p.n) return hipSuccess;
  hipLaunchKernelGGL(k_add_targets, dim3(1), dim3(64), 0, s, p);
  return hipGetLastError();
}

}  // namespace avk
