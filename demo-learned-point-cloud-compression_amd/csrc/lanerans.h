// lanerans.h — the pieces of the lane-parallel adaptive binary rANS scheme that the coders built on it share: the
// geometry slot's blob version 2 (octree2.hip) and the attribute blob (attr.hip).
//
// Both code runs of items per lane, 64 lanes per chunk (one wave), every lane with its own 32-bit state (L = 2^16,
// 16-bit words), its own run of renormalisation words and its own copy of an adaptive binary model (12-bit
// probabilities, adaptation shift 4) that starts from the frame's average probability per context (p0).  A chunk's
// payload is 64 x (state lo, state hi) | u16 len[64] | words of lane 0 | words of lane 1 | ...
#pragma once
#include "common.h"

#include <stdint.h>

namespace {

constexpr int kLanes = 64;

// the initial probability of a one from the zeros and ones a context saw over the whole frame
__host__ __device__ inline uint32_t o2_p0(uint64_t c0, uint64_t c1) {
  const uint64_t p = (4096ull * (2 * c1 + 1)) / (2 * (c0 + c1 + 1));
  return (uint32_t)(p < 16 ? 16 : (p > 4080 ? 4080 : p));
}
// (both sides computed and merged by a mask: written as a conditional expression the compiler made it a divergent branch)
__device__ __forceinline__ uint32_t o2_adapt(uint32_t p, uint32_t bit) {
  const uint32_t up = p + ((4096u - p) >> 4), dn = p - (p >> 4), m = 0u - bit;
  return (up & m) | (dn & ~m);
}
__device__ __forceinline__ uint64_t uniform_u64(uint64_t u) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
}

// Every kernel of these coders codes or decodes the frames of one call side by side: a table in device memory has one
// row per frame, a block finds its frame by a search over the rows' first block (the same for all its threads), and a
// single frame is the table of one row.  Last row whose start <= v:
template <typename Start>
__device__ __forceinline__ int o2_find(int nf, int64_t v, Start start) {
  int lo = 0, hi = nf - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start(mid) <= v) lo = mid; else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

// floor(2^32 / f) for f = 1 .. 4095 (entry 0 and 1 unused: a frequency is 15 .. 4081): x / f for x < 2^32 is
// mulhi(x, rcp[f]) or one more (checked by the remainder)
struct O2Rcp {
  uint32_t v[4096];
};
__host__ __device__ constexpr O2Rcp o2_rcp_table() {
  O2Rcp t{};
  for (int f = 2; f < 4096; ++f) t.v[f] = (uint32_t)(0x100000000ull / (uint64_t)f);
  t.v[0] = 0;
  t.v[1] = 0xFFFFFFFFu;
  return t;
}
__device__ const O2Rcp kO2Rcp = o2_rcp_table();

// the 16-KB reciprocal table into LDS by the 64 threads of a chunk's wave
__device__ __forceinline__ void lr_load_rcp(uint32_t* s_rcp, int lane) {
  const uint4* src = reinterpret_cast<const uint4*>(kO2Rcp.v);
  uint4* dst = reinterpret_cast<uint4*>(s_rcp);
#pragma unroll
  for (int i = 0; i < 16; ++i) dst[lane + 64 * i] = src[lane + 64 * i];
}

// Per-lane word-run staging, for a packing block of 256 threads: chunk c's final states, length table and the 64 lanes'
// runs to dst.  The encoder left lane l's run at the END of its T-word region work + (c 64 + l) T (written downwards).
// (k_o2_pack keeps its own copy of these lines: through this function one instruction of it moved.)
__device__ __forceinline__ void lr_stage_chunk(const uint16_t* work, int64_t c, int64_t T, const uint16_t* states,
                                               const uint16_t* lens, uint32_t* s_off, uint16_t* dst) {
  if (threadIdx.x == 0) {   // where every lane's run starts (words behind the states and the length table)
    uint32_t off = 3u * kLanes;
    for (int l = 0; l < kLanes; ++l) {
      s_off[l] = off;
      off += lens[c * kLanes + l];
    }
    s_off[kLanes] = off;
  }
  if (threadIdx.x < 2 * kLanes) dst[threadIdx.x] = states[c * 2 * kLanes + threadIdx.x];
  if (threadIdx.x < kLanes) dst[2 * kLanes + threadIdx.x] = lens[c * kLanes + threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
  for (int l = wave; l < kLanes; l += 4) {
    const uint32_t n_w = s_off[l + 1] - s_off[l];
    const uint16_t* src = work + (c * kLanes + l) * T + (T - n_w);
    uint16_t* d = dst + s_off[l];
    for (uint32_t j = ln; j < n_w; j += 64) d[j] = src[j];
  }
}

inline uint32_t get_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace

// pinned staging of a context, grown on demand (blobs and decoded values cross PCIe through it): octree2.hip
int o2_stage_reserve(pcc_ctx* ctx, size_t bytes);
