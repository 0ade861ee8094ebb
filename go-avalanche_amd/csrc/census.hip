// Network census (av_census): per-target, per-node and per-confidence tallies of the VoteRecord
// state in one pass over the A and K planes, with no N x M intermediate. What a caller would get
// from IsAccepted / GetConfidence over every Processor (processor.go:125-140) and from the example's
// stop test (main.go:143-162), reduced on the device.
//
// Mapping. A wave takes whole tiles (lane = g & 63) and steps through them by a multiple of
// P = BL / gcd(64, BL) tiles, so the block index b = g % BL of each lane stays fixed while it
// walks: bit i of a lane's words is always the same target, and the per-target column sums can be
// kept as vertical (bit-sliced, carry-save) counters in registers: one counter per class and per
// count bit, each a stack of u32 planes in which plane d holds bit d of 32 independent counts.
//   level 1: 3 planes, one ripple add per tile, full after kCensusL1 = 7 tiles;
//   level 2: 8 planes, takes a level-1 counter per spill, full after kCensusSpills = 36 spills.
// Every kCensusFlush = 252 tiles a lane expands its level-2 counters into integers and adds them
// to its workgroup's LDS table (64 slots x 32 bits: slot = b when BL < 64, else the lane, whose 64
// blocks are distinct). All four waves of a workgroup work on one unit = (tile class r = tile % P,
// chunk of that class), so they share the table; when the unit ends the table goes to the global
// int64 sums with one no-return atomic per non-zero entry. The three classes with a set bit
// somewhere (live rejected, live accepted, absent accepted) are summed; absent-rejected is what is
// left of the counted nodes (av_census fills it in on the host from the node count).
//
// The deferred forms of the count planes (kernels.h klazy / kHiVirt) are read through exactly as
// k_read_records_v does and never written back. vstale / kCAll concern the V and C planes only.
#include <algorithm>

#include "round_common.h"

namespace avk {
namespace {

constexpr uint32_t kCensusL1 = 7;                            // tiles per level-1 counter (3 planes)
constexpr uint32_t kCensusSpills = 36;                       // level-1 spills per level-2 counter (8 planes: 252 <= 255)
constexpr uint32_t kCensusFlush = kCensusL1 * kCensusSpills;  // tiles between two LDS flushes of a lane
static_assert(kCensusFlush <= 255u, "a level-2 counter holds 8 bits");
constexpr uint32_t kSlots = 64u * 32u;                       // LDS table entries: [bit][slot]

__device__ __forceinline__ void vadd1(uint32_t (&c)[3], uint32_t x) {
  uint32_t t = c[0] & x;
  c[0] ^= x;
  x = t;
  t = c[1] & x;
  c[1] ^= x;
  c[2] ^= t;
}

// level 2 += level 1 (a 3-plane number into an 8-plane one); clears level 1
__device__ __forceinline__ void vspill(uint32_t (&h)[8], uint32_t (&l)[3]) {
  uint32_t cy = 0u;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const uint32_t t = h[d] ^ l[d];
    const uint32_t s = t ^ cy;
    cy = (h[d] & l[d]) | (t & cy);
    h[d] = s;
    l[d] = 0u;
  }
#pragma unroll
  for (int d = 3; d < 8; ++d) {
    const uint32_t t = h[d] & cy;
    h[d] ^= cy;
    cy = t;
  }
}

__device__ __forceinline__ uint32_t vget(const uint32_t (&h)[8], uint32_t bit) {
  uint32_t v = 0u;
#pragma unroll
  for (int d = 0; d < 8; ++d) v |= ((h[d] >> bit) & 1u) << d;
  return v;
}

template <bool TGT, bool SUM, bool NODE, bool HIST>
__global__ __launch_bounds__(256) void k_census(const CensusParams p) {
  constexpr bool LOW = SUM || HIST;  // the K0..K3 group is needed
  constexpr int NCLS = TGT ? 3 : 0, NC = NCLS + (SUM ? 7 : 0), NCA = NC ? NC : 1;
  __shared__ uint32_t s_cls[TGT ? 3 * kSlots : 1];
  __shared__ unsigned long long s_sum[SUM ? kSlots : 1];
  __shared__ unsigned long long s_hist[HIST ? 256 : 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (TGT)
    for (uint32_t i = tid; i < 3u * kSlots; i += 256u) s_cls[i] = 0u;
  if (SUM)
    for (uint32_t i = tid; i < kSlots; i += 256u) s_sum[i] = 0ull;
  if (HIST) s_hist[tid] = 0ull;
  __syncthreads();

  uint32_t counted = 0u;             // nodes this lane counted (its block-0 lanes)
  uint32_t hc = 0u, h0 = 0u, h1 = 0u;  // count_hist run: records of count hc by accepted bit
  const uint32_t classes = p.P < p.nT ? p.P : p.nT;
  const uint32_t nlstep = (uint32_t)((uint64_t)p.P * 256u / p.BL);  // nodes per step of 4 P tiles

  for (uint32_t u = blockIdx.x; u < classes * p.C; u += gridDim.x) {
    const uint32_t r = u % classes, c = u / classes;
    const uint32_t nTr = (p.nT - r + p.P - 1u) / p.P;
    const uint32_t i0 = c * p.S, i1 = min(nTr, i0 + p.S);
    const uint32_t T0 = p.tlo + r;
    const uint32_t b0 = (uint32_t)(((uint64_t)T0 * 64u) % p.BL);
    const uint32_t b = (b0 + lane) % p.BL;
    const uint32_t real = real_mask(p.tn, b), val = p.valid[b];
    const uint32_t slot = p.BL < 64u ? b : lane;
    uint32_t l1[NCA][3], l2[NCA][8];
#pragma unroll
    for (int k = 0; k < NCA; ++k) {
#pragma unroll
      for (int d = 0; d < 3; ++d) l1[k][d] = 0u;
#pragma unroll
      for (int d = 0; d < 8; ++d) l2[k][d] = 0u;
    }
    uint32_t n1 = 0u, n2 = 0u;

    auto flush_lds = [&]() {
#pragma unroll 1
      for (uint32_t bit = 0; bit < 32u; ++bit) {
        const uint32_t idx = bit * 64u + slot;
        if constexpr (TGT) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const uint32_t v = vget(l2[k], bit);
            if (v) atomicAdd(&s_cls[k * kSlots + idx], v);
          }
        }
        if constexpr (SUM) {
          uint32_t sum = 0u;
#pragma unroll
          for (int q = 0; q < 7; ++q) sum += vget(l2[NCLS + q], bit) << q;
          if (sum) atomicAdd(&s_sum[idx], (unsigned long long)sum);
        }
      }
#pragma unroll
      for (int k = 0; k < NCA; ++k) {
#pragma unroll
        for (int d = 0; d < 8; ++d) l2[k][d] = 0u;
      }
    };

    // one tile's words; the next tile's are in flight while this one is counted, and its kpend
    // word (which decides whether the K4..K7 group is loaded at all) one tile further ahead
    struct Raw {
      u32x4 khi, klo;
      uint32_t A, kw;
    };
    auto load_kw = [&](uint32_t ii) -> uint32_t {
      return p.kpend && ii < i1 ? p.kpend[T0 + p.P * ii] : 0u;
    };
    auto load_tile = [&](uint32_t ii, uint32_t kw) -> Raw {
      const uint32_t* tp = p.planes + (size_t)(T0 + p.P * ii) * (kPlanes * 64);  // <= the range's last tile
      Raw t;
      t.kw = kw;
      t.khi = u32x4{0u, 0u, 0u, ~real};  // the virtual K4..K7 group (kernels.h kHiVirt)
      if (!(kw & kHiVirt)) t.khi = pld4<true>(reinterpret_cast<const u32x4*>(tp + plane_off(kPK + 4, lane)));
      t.klo = u32x4{0u, 0u, 0u, 0u};
      if constexpr (LOW) t.klo = pld4<true>(reinterpret_cast<const u32x4*>(tp + plane_off(kPK, lane)));
      t.A = pld<true>(tp + plane_off(kPA, lane));
      return t;
    };

    uint32_t i = i0 + wave;
    uint32_t nl = 0u;
    Raw cur{};
    uint32_t kwn = 0u;
    if (i < i1) {
      nl = (uint32_t)((((uint64_t)T0 + (uint64_t)p.P * i) * 64u + lane) / p.BL);
      cur = load_tile(i, load_kw(i));
      kwn = load_kw(i + 4u);
    }
    for (; i < i1; i += 4u, nl += nlstep) {
      const uint32_t T = T0 + p.P * i;
      Raw nxt = cur;
      if (i + 4u < i1) nxt = load_tile(i + 4u, kwn);
      kwn = load_kw(i + 8u);
      const uint32_t kw = cur.kw, A = cur.A;
      const u32x4 khi = cur.khi, klo = cur.klo;
      cur = nxt;

      const uint32_t g = T * 64u + lane;
      bool act = g >= p.glo && g < p.ghi;  // not padding, inside the node range
      if (p.honest_only && act) act = !is_byz(p.byz, p.n0 + nl);
      const uint32_t K7 = khi[3];
      const uint32_t am = act ? real : 0u;  // the lane's records: existing targets only
      const uint32_t live = ~K7 & am, dead = K7 & am;
      const uint32_t c0 = live & ~A, c1 = live & A, c3 = dead & A;
      if (act && b == 0u) ++counted;

      if constexpr (TGT) {
        vadd1(l1[0], c0);
        vadd1(l1[1], c1);
        vadd1(l1[2], c3);
      }
      if constexpr (NODE) {
        // <= 32 * 64 per field after the reduction over a node's lanes: two fields per word
        uint32_t x = (uint32_t)__popc(c0) | ((uint32_t)__popc(c1) << 16);
        uint32_t y = (uint32_t)__popc(dead & ~A) | ((uint32_t)__popc(c3) << 16);
        if (p.bl_div64) {  // a node's lanes are BL aligned lanes of this wave
          for (uint32_t d = 1u; d < p.BL; d <<= 1) {
            x += (uint32_t)__shfl_xor((int)x, (int)d, 64);
            y += (uint32_t)__shfl_xor((int)y, (int)d, 64);
          }
          if (act && b == 0u) {
            int4 v = {(int)(x & 0xFFFFu), (int)(x >> 16), (int)(y & 0xFFFFu), (int)(y >> 16)};
            *reinterpret_cast<int4*>(p.ncls + (size_t)(nl - p.nl0) * 4u) = v;
          }
        } else if (act) {
          int32_t* row = p.ncls + (size_t)(nl - p.nl0) * 4u;
          if (x & 0xFFFFu) atomicAdd(row + 0, (int)(x & 0xFFFFu));
          if (x >> 16) atomicAdd(row + 1, (int)(x >> 16));
          if (y & 0xFFFFu) atomicAdd(row + 2, (int)(y & 0xFFFFu));
          if (y >> 16) atomicAdd(row + 3, (int)(y >> 16));
        }
      }
      if constexpr (LOW) {
        uint32_t K[7] = {klo[0], klo[1], klo[2], klo[3], khi[0], khi[1], khi[2]};
        const uint32_t pend = kw & 0xFFu;
        if (pend) {  // + 8 * pend on the live valid records, as k_read_records_v adds it
          const uint32_t P0 = ~K7 & val;
          uint32_t cy = 0u;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t bi = ((pend >> q) & 1u) ? P0 : 0u;
            const uint32_t t = K[3 + q] ^ bi;
            const uint32_t si = t ^ cy;
            cy = (t & cy) | (K[3 + q] & bi);
            K[3 + q] = si;
          }
        }
        if constexpr (SUM) {
#pragma unroll
          for (int q = 0; q < 7; ++q) vadd1(l1[NCLS + q], K[q] & live);
        }
        if constexpr (HIST) {
          if (live) {
            uint32_t cnt = 0u;
            bool uni = true;  // every live record of the lane has the same count
#pragma unroll
            for (int q = 0; q < 7; ++q) {
              const uint32_t m = K[q] & live;
              uni = uni && (m == 0u || m == live);
              cnt |= (m ? 1u : 0u) << q;
            }
            if (uni) {
              if (cnt != hc) {
                if (h0) atomicAdd(&s_hist[hc], (unsigned long long)h0);
                if (h1) atomicAdd(&s_hist[128u + hc], (unsigned long long)h1);
                hc = cnt;
                h0 = h1 = 0u;
              }
              h0 += (uint32_t)__popc(c0);
              h1 += (uint32_t)__popc(c1);
            } else {
              for (uint32_t m = live; m; m &= m - 1u) {
                const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
                uint32_t k = 0u;
#pragma unroll
                for (int q = 0; q < 7; ++q) k |= ((K[q] >> bit) & 1u) << q;
                atomicAdd(&s_hist[(((A >> bit) & 1u) << 7) + k], 1ull);
              }
            }
          }
        }
      }
      if constexpr (NC > 0) {
        if (++n1 == kCensusL1) {
          n1 = 0u;
#pragma unroll
          for (int k = 0; k < NC; ++k) vspill(l2[k], l1[k]);
          if (++n2 == kCensusSpills) {
            n2 = 0u;
            flush_lds();
          }
        }
      }
    }
    if constexpr (NC > 0) {
#pragma unroll
      for (int k = 0; k < NC; ++k) vspill(l2[k], l1[k]);
      flush_lds();
      __syncthreads();
      for (uint32_t idx = tid; idx < kSlots; idx += 256u) {
        const uint32_t bit = idx >> 6, sl = idx & 63u;
        const uint32_t bb = p.BL < 64u ? sl : (b0 + sl) % p.BL;
        const uint32_t tl = bb * 32u + bit;
        const bool ok = (p.BL >= 64u || sl < p.BL) && tl < p.tn;
        if constexpr (TGT) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const uint32_t v = s_cls[k * kSlots + idx];
            if (v) {
              if (ok) atomicAdd(p.tcls + (size_t)tl * 3u + k, (unsigned long long)v);
              s_cls[k * kSlots + idx] = 0u;
            }
          }
        }
        if constexpr (SUM) {
          const unsigned long long v = s_sum[idx];
          if (v) {
            if (ok) atomicAdd(p.tsum + tl, v);
            s_sum[idx] = 0ull;
          }
        }
      }
      __syncthreads();
    }
  }

  if constexpr (TGT) {
    const uint32_t w = wave_sum(counted);
    if (lane == 0u && w) atomicAdd(p.counted, (unsigned long long)w);
  }
  if constexpr (HIST) {
    if (h0) atomicAdd(&s_hist[hc], (unsigned long long)h0);
    if (h1) atomicAdd(&s_hist[128u + hc], (unsigned long long)h1);
    __syncthreads();
    const unsigned long long v = s_hist[tid];
    if (v) atomicAdd(p.hist + tid, v);
  }
}

uint32_t gcd_u32(uint32_t a, uint32_t b) {
  while (b) {
    const uint32_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

template <bool TGT, bool SUM, bool NODE, bool HIST>
hipError_t launch_census_t(CensusParams p, uint32_t blocks, hipStream_t s) {
  const uint32_t classes = std::min(p.P, p.nT);
  const uint32_t per_class = (p.nT + p.P - 1u) / p.P;  // tiles of the largest class
  uint32_t grid = blocks;
  if (!grid) {
    int dev = 0, cus = 0, occ = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess)
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_census<TGT, SUM, NODE, HIST>, 256, 0);
    if (e != hipSuccess) return e;
    grid = (uint32_t)std::max(1, cus) * (uint32_t)std::min(8, std::max(1, occ));
  }
  // chunks per class: fill the grid, but leave every wave of a chunk at least 8 tiles
  p.C = std::max(1u, std::min(grid / classes, (per_class + 31u) / 32u));
  p.S = (per_class + p.C - 1u) / p.C;
  grid = std::min(grid, classes * p.C);
  hipLaunchKernelGGL((k_census<TGT, SUM, NODE, HIST>), dim3(grid), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_census(CensusParams p, uint32_t nl0, uint32_t nl1, uint32_t blocks, hipStream_t s) {
  if (nl1 <= nl0 || !p.BL || !p.tn) return hipSuccess;
  if (!p.tcls && !p.tsum && !p.ncls && !p.hist) return hipErrorInvalidValue;
  if (p.tcls && !p.counted) return hipErrorInvalidValue;
  p.nl0 = nl0;
  p.glo = nl0 * p.BL;
  p.ghi = nl1 * p.BL;
  p.tlo = p.glo >> 6;
  p.nT = ((p.ghi - 1u) >> 6) - p.tlo + 1u;
  p.P = p.BL / gcd_u32(64u, p.BL);
  p.bl_div64 = 64u % p.BL == 0u ? 1u : 0u;
  const int sel = (p.tcls ? 8 : 0) | (p.tsum ? 4 : 0) | (p.ncls ? 2 : 0) | (p.hist ? 1 : 0);
  switch (sel) {
#define AVK_CENSUS_CASE(n) \
  case n: return launch_census_t<((n) & 8) != 0, ((n) & 4) != 0, ((n) & 2) != 0, ((n) & 1) != 0>(p, blocks, s);
    AVK_CENSUS_CASE(1) AVK_CENSUS_CASE(2) AVK_CENSUS_CASE(3) AVK_CENSUS_CASE(4) AVK_CENSUS_CASE(5)
    AVK_CENSUS_CASE(6) AVK_CENSUS_CASE(7) AVK_CENSUS_CASE(8) AVK_CENSUS_CASE(9) AVK_CENSUS_CASE(10)
    AVK_CENSUS_CASE(11) AVK_CENSUS_CASE(12) AVK_CENSUS_CASE(13) AVK_CENSUS_CASE(14) AVK_CENSUS_CASE(15)
#undef AVK_CENSUS_CASE
  }
  return hipErrorInvalidValue;
}

}  // namespace avk
