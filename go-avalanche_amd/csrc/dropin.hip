// The drop-in Processor calls on the device (CDNA4, gfx950): RegisterVotes for
// one Response or a batch (k_register_votes; k_dropin_resp when every Response's
// targets ascend, else k_dropin_keys and the stable grouping of the votes by
// lane, launch_group_votes, with the radix sort and scan of dev_scan.h) and
// AddTargetToReconcile: many nodes' lists grouped the same way (k_add_lanes), or one list for every
// node of a range (k_admit_blocks, k_admit_lanes). Each launcher sits below its kernels.
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

hipError_t launch_dropin_keys(const DropInParams& p, const GroupScratch& g, hipStream_t s) {
  if (!p.n_resp) return hipSuccess;
  hipLaunchKernelGGL(k_dropin_keys, dim3(std::min<uint32_t>(p.n_resp, 65535u)), dim3(256), 0, s, p, g.keys, g.vidx,
                     g.info);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Drop-in RegisterVotes batch (engine_dropin.cpp group_by_lane): group the votes by lane (node,
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

hipError_t launch_group_votes(const GroupScratch& g, uint32_t n, int key_bits, hipStream_t s) {
  if (n == 0) return hipMemsetAsync(g.nruns, 0, 4, s);
  hipError_t e =
      dscan::launch_radix_sort_pairs(g.keys, nullptr, n, key_bits, g.keys_s, g.perm_s, g.keys_t, g.perm_t, g.temp, s);
  if (e != hipSuccess) return e;
  // run index of every position: exclusive scan of the run heads (run_of[n] = runs)
  uint64_t* run_of = g.temp;
  if ((e = dscan::launch_scan(HeadsIn{g.keys_s}, n, run_of, g.temp + n + 1u, s)) != hipSuccess) return e;
  const uint32_t grid = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_rle_write, dim3(grid), dim3(256), 0, s, (const uint32_t*)g.keys_s, (const uint64_t*)run_of, n,
                     g.lanes, g.offs, g.nruns);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_vote_entries, dim3(grid), dim3(256), 0, s, (const uint32_t*)g.perm_s, (const uint32_t*)g.vidx,
                     (const uint32_t*)g.info, n, g.entries);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// AddTargetToReconcile (processor.go:45-58): av_add_targets_batch (k_add_lanes) and av_admit_targets
// (k_admit_blocks, k_admit_lanes). A record is created iff the target is valid (isWorthyPolling,
// :46-48) and the node holds no live record of it (K7 set, :50-53).
// ---------------------------------------------------------------------------
namespace {
// the word offsets create_records uses are plane_off's
static_assert(plane_off(kPV + 5, 7u) == 1u * 256u + 7u * 4u + 1u && plane_off(kPK + 7, 7u) == 3u * 256u + 7u * 4u + 3u &&
                  plane_off(kPC + 3, 7u) == 1024u + 3u * 64u + 7u && plane_off(kPA, 7u) == 1536u + 7u,
              "tile layout");

// NewVoteRecord(accepted) (vote.go:33-35) on the records `add` of lane g: their votes, consider and
// count bits cleared (the V and K groups as four dwordx4, the eight C words), A = acc on them. A whole
// block is stored without being read. Returns the lane's new A word.
__device__ __forceinline__ uint32_t create_records(const uint32_t* planes, uint32_t g, uint32_t add, uint32_t acc) {
  uint32_t* t = tile_of(planes, g);
  const uint32_t l = g & 63u;
  u32x4* q = reinterpret_cast<u32x4*>(t) + l;
  uint32_t* c = t + 1024u + l;
  uint32_t* a = t + 1536u + l;
  if (add == ~0u) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i * 64] = z;
#pragma unroll
    for (int i = 0; i < 8; ++i) c[i * 64] = 0u;
    *a = acc;
    return acc;
  }
  const uint32_t keep = ~add;
  u32x4 v[4];
  uint32_t cw[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = q[i * 64];
#pragma unroll
  for (int i = 0; i < 8; ++i) cw[i] = c[i * 64];
  const uint32_t A = (*a & keep) | (acc & add);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i][0] &= keep;
    v[i][1] &= keep;
    v[i][2] &= keep;
    v[i][3] &= keep;
    q[i * 64] = v[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i * 64] = cw[i] & keep;
  *a = A;
  return A;
}

// One thread per touched lane (launch_group_votes' runs) walks the lane's entries in call order: the
// first occurrence of a valid, absent target creates its record, every later one returns false. The
// lane's planes are read and written once, its published word once; a lane that creates nothing
// stores nothing.
__global__ void k_add_lanes(const DropInParams p, uint8_t* added) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_blocks) return;
  const uint32_t g = p.blocks[i];
  if (g >= p.L) return;  // the run of foreign targets: added stays 0
  const uint32_t nl = g / p.BL, b = g - nl * p.BL;
  const uint32_t node = p.n0 + nl;
  const uint32_t k7 = *pw(p.planes, g, kPK + 7);
  const uint32_t can = p.valid[b] & k7;
  uint32_t created = 0u, acc = 0u;
  for (uint32_t e = p.offs[i]; e < p.offs[i + 1]; ++e) {
    const uint32_t pos = p.entries[2 * e];
    const uint32_t meta = p.entries[2 * e + 1];
    const uint32_t m = 1u << (meta & 31u);
    const bool ok = (can & ~created & m) != 0u;
    if (ok) {
      created |= m;
      if ((meta >> 5) & 1u) acc |= m;
    }
    added[pos] = ok ? 1 : 0;
  }
  if (!created) return;
  const uint32_t A = create_records(p.planes, g, created, acc);
  p.pref[(size_t)node * p.PS + b] =
      is_byz(p.byz, node) ? byz_pattern(p.round) : publish_word(A, k7 & ~created, p.pub_mode);
}

// av_admit_targets, one lane: local node nl adds the records `req` of local block b. Reads the lane's
// K7 word; a lane with nothing to create stores nothing. Returns the records created.
__device__ __forceinline__ uint32_t admit_lane(const AdmitParams& p, uint32_t nl, uint32_t b, uint32_t req,
                                               uint32_t given) {
  const uint32_t g = nl * p.BL + b;
  const uint32_t k7 = *pw(p.planes, g, kPK + 7);
  const uint32_t add = req & p.valid[b] & k7;
  if (add) {
    const uint32_t node = p.n0 + nl;
    const uint32_t acc = p.mode == 5 ? given : init_accept_block(p.seed, p.mode, p.param, node, p.t0 + 32u * b);
    const uint32_t A = create_records(p.planes, g, add, acc);
    p.pref[(size_t)node * p.PS + b] =
        is_byz(p.byz, node) ? byz_pattern(p.round) : publish_word(A, k7 & ~add, p.pub_mode);
  }
  return add;
}

// A wave = 64 consecutive nodes of one touched block (blockIdx.y): the request mask is wave-uniform,
// and the nodes that created bit i are one ballot and one popcount, kept by lane i over the
// workgroup's node chunks; the four waves add up in LDS and one atomic instruction per workgroup
// (32 lanes, the block's 32 consecutive counters: one request for their 128-B line) adds the sums.
__global__ __launch_bounds__(256) void k_admit_blocks(const AdmitParams p) {
  __shared__ uint32_t s_cnt[32];
  const uint32_t j = blockIdx.y;
  const uint32_t b = p.tblk[j], req = p.treq[j], given = p.tacc[j];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t mine = 0u;
  for (uint32_t base = blockIdx.x * 256u; base < p.nn; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t add = i < p.nn ? admit_lane(p, p.nl0 + i, b, req, given) : 0u;
    if (p.counts) {
      for (uint32_t r = req; r; r &= r - 1u) {
        const uint32_t bit = (uint32_t)__builtin_ctz(r);
        const uint32_t c = (uint32_t)__popcll(__ballot((add >> bit) & 1u));
        if (lane == bit) mine += c;
      }
    }
  }
  if (!p.counts) return;
  if (threadIdx.x < 32u) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  if (lane < 32u && mine) atomicAdd(&s_cnt[lane], mine);
  __syncthreads();
  if (threadIdx.x < 32u && s_cnt[threadIdx.x]) atomicAdd(p.counts + j * 32u + threadIdx.x, s_cnt[threadIdx.x]);
}

// Thread v = (node, touched block v % TB): with every block touched, consecutive threads are
// consecutive lanes and a wave streams whole tiles, as k_init_planes does. The grid's stride is a
// multiple of TB (launch_admit), so a thread keeps its block: it counts its 32 bits in registers,
// the workgroup's threads of one block add up in LDS (same block <=> same threadIdx.x % TB), and
// the sums go to the counters 32 consecutive lanes per block: one request per 128-B counter line
// (one lane per counter, 32 requests per line and workgroup, cost 0.3 - 0.5 ms on 10^6 x 1000).
__global__ __launch_bounds__(256) void k_admit_lanes(const AdmitParams p) {
  __shared__ uint32_t s_cnt[256 * 32];
  const uint64_t total = (uint64_t)p.nn * p.TB;
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  const uint64_t v0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t j = (uint32_t)(v0 % p.TB);
  const uint32_t b = p.tblk[j], req = p.treq[j], given = p.tacc[j];
  if (p.counts) {
    for (uint32_t i = threadIdx.x; i < 256u * 32u; i += 256u) s_cnt[i] = 0u;
    __syncthreads();
  }
  uint32_t cnt[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) cnt[i] = 0u;
  for (uint64_t v = v0; v < total; v += stride) {  // total <= the engine's lanes < 2^32
    const uint32_t add = admit_lane(p, p.nl0 + (uint32_t)v / p.TB, b, req, given);
#pragma unroll
    for (int i = 0; i < 32; ++i) cnt[i] += (add >> i) & 1u;
  }
  if (!p.counts) return;
  const uint32_t slots = min(p.TB, 256u);
  const uint32_t slot = p.TB <= 256u ? threadIdx.x % p.TB : threadIdx.x;
#pragma unroll
  for (int i = 0; i < 32; ++i)
    if (cnt[i]) atomicAdd(&s_cnt[slot * 32u + i], cnt[i]);
  __syncthreads();
  // slot s is the block of the workgroup's thread s (the stride keeps it)
  const uint32_t j0 = (uint32_t)(((uint64_t)blockIdx.x * 256u) % p.TB);
  for (uint32_t i = threadIdx.x; i < slots * 32u; i += 256u) {
    const uint32_t c = s_cnt[i];
    const uint32_t js = (j0 + (i >> 5)) % p.TB;
    if (c) atomicAdd(p.counts + js * 32u + (i & 31u), c);
  }
}
}  // namespace

hipError_t launch_add_lanes(const DropInParams& p, uint8_t* added, hipStream_t s) {
  if (!p.n_blocks) return hipSuccess;
  hipLaunchKernelGGL(k_add_lanes, dim3((p.n_blocks + 63) / 64), dim3(64), 0, s, p, added);
  return hipGetLastError();
}

hipError_t launch_admit(const AdmitParams& p, bool lane_major, hipStream_t s) {
  if (!p.nn || !p.TB) return hipSuccess;
  if (!lane_major) {
    if (p.TB > 65535u) return hipErrorInvalidValue;
    const uint32_t gx = std::min<uint32_t>((p.nn + 255u) / 256u, std::max<uint32_t>(1u, 2048u / p.TB));
    hipLaunchKernelGGL(k_admit_blocks, dim3(gx, p.TB), dim3(256), 0, s, p);
    return hipGetLastError();
  }
  // a grid that does not cover every (node, block) in one pass strides by a multiple of TB
  const uint64_t need = ((uint64_t)p.nn * p.TB + 255u) / 256u;
  uint32_t gcd = p.TB, r = 256u;
  while (r) {
    const uint32_t t = gcd % r;
    gcd = r;
    r = t;
  }
  const uint64_t q = p.TB / gcd;
  const uint64_t cap = (2048u + q - 1u) / q * q;
  hipLaunchKernelGGL(k_admit_lanes, dim3((uint32_t)std::min(need, cap)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace avk
