// nn.hip — exact nearest neighbours on the int16 lattice, frame by frame: the search behind the D1 (point-to-point)
// distortion of GeometryCodec.distortion.  include/pcc.h has the rule; tests/nn_ref.py restates it in numpy.
//
// The reference of a call is what pcc_octree_encode_frames takes: Morton keys, sorted and distinct, the frame index
// above bit 48.  Sorted keys are an implicit octree: the points of a cell of edge 2^L share the key bits above 3 L and
// lie in one contiguous range of rows.  One thread per query walks the cells of its own frame in row order:
//
//   seed   the two rows around the query's place in key order (clamped to the frame's rows: the neighbour in key order
//          may belong to the next frame) give the first `best`; an equal key ends the search, keys being distinct.
//   walk   at row r the cells that BEGIN at r are those of levels 0 .. b / 3, b the highest bit in which keys r - 1 and
//          r differ (levels 0 .. 15 at the frame's first row).  They are tried from the largest down: a cell whose box
//          distance exceeds best, or equals best while r > best_row, is left out whole — r jumps to the first row
//          behind the cell's key range (a binary search in the rest of the frame).  Cells that hold row r alone are
//          not tried: the point is measured instead, and r advances by one.  Only cells that hold points are ever tried, each once, so a query tries no more
//          nodes than its frame's octree has, every step moves r forward, and no step waits for another thread.
//   state  r, the previous key, best, best_row and the query's three coordinates: scalars, no stack and no array, so
//          nothing lives in scratch (DESIGN.md 6c has the register figures).
//
// Coordinates are the biased ones of the keys, 0 .. 65535; a per-axis difference squared fits 32 bits, the sum of
// three is formed in 64.  Rows are in order, so among equidistant points the first met wins unless the seed was a later
// row: every comparison carries the row as its tie-break.
//
// Statistics: after the walk the wave's lanes meet again; per frame present in the wave one reduction over the lanes
// (shuffles) and then three 64-bit atomics from one lane.  Sorted queries of one frame: one round per wave.
#include "common.h"
#include "nn_cells.h"
#include <algorithm>

static inline unsigned nblk(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

// bit 0: equal neighbours, bit 1: descending neighbours, bit 2: a reference key's frame index >= n_frames,
// bit 3: a query key's frame index >= n_frames
__global__ __launch_bounds__(256) void k_nn_check(const uint64_t* __restrict__ rkeys, int64_t n_r,
                                                  const uint64_t* __restrict__ qkeys, int64_t n_q, int n_frames,
                                                  int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int bits = 0;
  if (i < n_r) {
    const uint64_t k = rkeys[i];
    if ((k >> 48) >= (uint64_t)n_frames) bits |= 4;
    if (i > 0) {
      const uint64_t p = rkeys[i - 1];
      if (p == k) bits |= 1;
      if (p > k) bits |= 2;
    }
  }
  if (i < n_q && (qkeys[i] >> 48) >= (uint64_t)n_frames) bits |= 8;
  if (bits) atomicOr(flag, bits);
}

// offs[f] = the first reference row of frame f, offs[n_frames] = n_r
__global__ __launch_bounds__(64) void k_nn_offsets(const uint64_t* __restrict__ rkeys, int64_t n_r, int n_frames,
                                                   int64_t* __restrict__ offs) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_frames) return;
  int64_t lo = 0, hi = n_r;
  if (f == n_frames) lo = n_r;
  const uint64_t want = (uint64_t)f << 48;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rkeys[mid] < want) lo = mid + 1; else hi = mid;
  }
  offs[f] = lo;
}

// the search of one query among the rows [flo, fhi) of its frame, flo < fhi: seed and walk as described above.
// Returns the nodes tried (cells tested and points measured, the two seeds included): pcc_nn_replay_host reports
// it, the kernel drops it.  One function for the device and the host, so the replay is the kernel's traversal.
__host__ __device__ static inline uint32_t nn_search(const uint64_t* __restrict__ rkeys, int64_t flo, int64_t fhi, uint64_t qk,
                                                     uint64_t* out_best, int64_t* out_row) {
  const uint32_t qx = pcc_compact3(qk >> 2), qy = pcc_compact3(qk >> 1), qz = pcc_compact3(qk);
  uint64_t best = ~0ull;
  int64_t best_row = -1;
  uint32_t nodes = 0;
  int64_t lo = flo, hi = fhi;      // the first row of the frame whose key is not below the query's
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rkeys[mid] < qk) lo = mid + 1; else hi = mid;
  }
  if (lo < fhi) {
    best = nn_d2(qx, qy, qz, rkeys[lo]);
    best_row = lo;
    ++nodes;
  }
  if (lo > flo) {
    const uint64_t d = nn_d2(qx, qy, qz, rkeys[lo - 1]);
    ++nodes;
    if (d <= best) {      // the smaller row wins a tie
      best = d;
      best_row = lo - 1;
    }
  }
  if (best != 0) {      // (0: the query's own key is in the reference, and no other point is as near)
    int64_t r = flo;
    uint64_t prev = 0;
    while (r < fhi) {
      const uint64_t k = rkeys[r];
      int L = r == flo ? 15 : (63 - __builtin_clzll(((prev ^ k) & NN_KEY48) | 1ull)) / 3;      // keys are distinct
      const uint32_t cx = pcc_compact3(k >> 2), cy = pcc_compact3(k >> 1), cz = pcc_compact3(k);
      // the cells of levels 0 .. l1 hold row r alone (key r + 1 leaves them): measuring the point is their test
      const int l1 = r + 1 < fhi ? (63 - __builtin_clzll(((k ^ rkeys[r + 1]) & NN_KEY48) | 1ull)) / 3 : 15;
      bool skipped = false;
      for (; L > l1; --L) {
        const uint64_t bd = (uint64_t)nn_gap_sq(qx, cx, L) + nn_gap_sq(qy, cy, L) + nn_gap_sq(qz, cz, L);
        ++nodes;
        if (bd > best || (bd == best && r > best_row)) {
          // the first row behind the cell, whose keys are [p << 3L, (p + 1) << 3L)
          const uint64_t end = (((k & NN_KEY48) >> (3 * L)) + 1ull) << (3 * L);
          int64_t a = r + 1, b = fhi;
          if (end <= NN_KEY48) {
            const uint64_t want = (k & ~NN_KEY48) | end;
            while (a < b) {
              const int64_t mid = (a + b) >> 1;
              if (rkeys[mid] < want) a = mid + 1; else b = mid;
            }
          } else {
            a = fhi;      // the cell reaches the end of the key range
          }
          r = a;
          skipped = true;
          break;
        }
      }
      if (skipped) {
        if (r < fhi) prev = rkeys[r - 1];
        continue;
      }
      const uint64_t d = (uint64_t)nn_sq(qx, cx) + nn_sq(qy, cy) + nn_sq(qz, cz);
      ++nodes;
      if (d < best || (d == best && r < best_row)) {
        best = d;
        best_row = r;
      }
      prev = k;
      ++r;
    }
  }
  *out_best = best;
  *out_row = best_row;
  return nodes;
}

__global__ __launch_bounds__(256) void k_nn_frames(const uint64_t* __restrict__ qkeys, int64_t n_q,
                                                   const uint64_t* __restrict__ rkeys, const int64_t* __restrict__ offs,
                                                   uint64_t* __restrict__ sqdist, int32_t* __restrict__ row,
                                                   unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  uint64_t best = ~0ull;
  int64_t best_row = -1;
  int f = 0;
  if (i < n_q) {
    const uint64_t qk = qkeys[i];
    f = (int)(qk >> 48);      // below n_frames: k_nn_check
    const int64_t flo = offs[f], fhi = offs[f + 1];
    if (fhi > flo) {
      valid = true;
      (void)nn_search(rkeys, flo, fhi, qk, &best, &best_row);
    }
    if (sqdist) sqdist[i] = best;
    if (row) row[i] = (int32_t)best_row;
  }
  if (!stats) return;      // the same in every lane
  // every lane of the wave is here again: one round per frame among the wave's valid lanes
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int f0 = __shfl(f, leader);
    const bool mine = valid && f == f0;
    unsigned long long s = mine ? best : 0ull, m = s, c = mine ? 1ull : 0ull;
    for (int off = 32; off; off >>= 1) {
      s += __shfl_xor(s, off);
      const unsigned long long o = __shfl_xor(m, off);
      m = o > m ? o : m;
      c += __shfl_xor(c, off);
    }
    if (lane == leader) {
      atomicAdd(&stats[3 * (size_t)f0], c);
      atomicAdd(&stats[3 * (size_t)f0 + 1], s);
      atomicMax(&stats[3 * (size_t)f0 + 2], m);
    }
    todo &= ~__ballot(mine);
  }
}

// sse[f][ch] += (a[i][ch] - b[row[i]][ch])^2 over the queries i of frame f; a query without a row (-1), a row outside
// the reference or a frame index outside the call adds nothing.  The reduction is k_nn_frames'.
template <typename T>
__global__ __launch_bounds__(256) void k_nn_attr_sse(const uint64_t* __restrict__ qkeys, const int32_t* __restrict__ row,
                                                     int64_t n_q, const T* __restrict__ a, const T* __restrict__ b,
                                                     int64_t n_r, int channels, int n_frames,
                                                     unsigned long long* __restrict__ sse) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  int f = 0;
  unsigned long long e0 = 0, e1 = 0, e2 = 0, e3 = 0;
  if (i < n_q) {
    const int64_t r = row[i];
    f = (int)(qkeys[i] >> 48);
    if (r >= 0 && r < n_r && f < n_frames) {
      valid = true;
      const T* pa = a + i * channels;
      const T* pb = b + r * channels;
      e0 = nn_sq(pa[0], pb[0]);
      if (channels > 1) e1 = nn_sq(pa[1], pb[1]);
      if (channels > 2) e2 = nn_sq(pa[2], pb[2]);
      if (channels > 3) e3 = nn_sq(pa[3], pb[3]);
    }
  }
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int f0 = __shfl(f, leader);
    const bool mine = valid && f == f0;
    unsigned long long s0 = mine ? e0 : 0ull, s1 = mine ? e1 : 0ull, s2 = mine ? e2 : 0ull, s3 = mine ? e3 : 0ull;
    for (int off = 32; off; off >>= 1) {
      s0 += __shfl_xor(s0, off);
      s1 += __shfl_xor(s1, off);
      s2 += __shfl_xor(s2, off);
      s3 += __shfl_xor(s3, off);
    }
    if (lane == leader) {
      unsigned long long* out = sse + (size_t)f0 * channels;
      atomicAdd(&out[0], s0);
      if (channels > 1) atomicAdd(&out[1], s1);
      if (channels > 2) atomicAdd(&out[2], s2);
      if (channels > 3) atomicAdd(&out[3], s3);
    }
    todo &= ~__ballot(mine);
  }
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
extern "C" int pcc_nn_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, int64_t n_q, const uint64_t* d_rkeys, int64_t n_r,
                             int n_frames, uint64_t* d_sqdist, int32_t* d_row, uint64_t* d_stats) {
  const int64_t kMax = (int64_t)1 << 27;
  PCC_REQUIRE(ctx && n_frames >= 1 && n_frames <= 65535 && n_q >= 0 && n_q <= kMax && n_r >= 0 && n_r <= kMax, PCC_E_ARG,
              "pcc_nn_frames: bad argument (n_q=%lld n_r=%lld n_frames=%d; at most 2^27 keys a side, 1 .. 65535 frames)",
              (long long)n_q, (long long)n_r, n_frames);
  PCC_REQUIRE((n_q == 0 || d_qkeys) && (n_r == 0 || d_rkeys), PCC_E_ARG, "pcc_nn_frames: null keys");
  hipStream_t st = ctx->stream;
  if (d_stats) PCC_HIP(hipMemsetAsync(d_stats, 0, (size_t)n_frames * 24, st));
  if (n_q == 0 && n_r == 0) return PCC_OK;
  const size_t offs_b = (size_t)(n_frames + 1) * 8;
  PCC_TRY(pcc_arena_reserve(ctx, pcc_align(offs_b) + 512));
  int64_t* offs = (int64_t*)pcc_arena_alloc(ctx, offs_b);
  int32_t* flag = (int32_t*)pcc_arena_alloc(ctx, 4);
  if (!offs || !flag) return PCC_E_NOMEM;
  PCC_HIP(hipMemsetAsync(flag, 0, 4, st));
  const int64_t n_chk = n_q > n_r ? n_q : n_r;
  hipLaunchKernelGGL(k_nn_check, dim3(nblk(n_chk, 256)), dim3(256), 0, st, d_rkeys, n_r, d_qkeys, n_q, n_frames, flag);
  PCC_CHECK_LAUNCH();
  if (n_r > 0) {
    hipLaunchKernelGGL(k_nn_offsets, dim3(nblk(n_frames + 1, 64)), dim3(64), 0, st, d_rkeys, n_r, n_frames, offs);
    PCC_CHECK_LAUNCH();
  }
  int32_t* h = (int32_t*)ctx->pinned;
  PCC_HIP(hipMemcpyAsync(h, flag, 4, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipStreamSynchronize(st));
  const int32_t bits = h[0];
  PCC_REQUIRE(!(bits & 4), PCC_E_RANGE, "pcc_nn_frames: a reference key's frame index is not below n_frames=%d", n_frames);
  PCC_REQUIRE(!(bits & 8), PCC_E_RANGE, "pcc_nn_frames: a query key's frame index is not below n_frames=%d", n_frames);
  PCC_REQUIRE(!(bits & 2), PCC_E_ARG, "pcc_nn_frames: reference keys not sorted (pcc_sort_pairs)");
  PCC_REQUIRE(!(bits & 1), PCC_E_DUP, "pcc_nn_frames: duplicate reference keys");
  if (n_q == 0) return PCC_OK;
  if (n_r == 0) {      // no candidate anywhere: d2 = 2^64 - 1, row = -1, statistics 0; no search kernel
    if (d_sqdist) PCC_HIP(hipMemsetAsync(d_sqdist, 0xFF, (size_t)n_q * 8, st));
    if (d_row) PCC_HIP(hipMemsetAsync(d_row, 0xFF, (size_t)n_q * 4, st));
    return PCC_OK;
  }
  if (!d_sqdist && !d_row && !d_stats) return PCC_OK;
  PccProfScope prof(ctx, "nn_frames", n_q, n_r, n_frames, 0);
  hipLaunchKernelGGL(k_nn_frames, dim3(nblk(n_q, 256)), dim3(256), 0, st, d_qkeys, n_q, d_rkeys, (const int64_t*)offs, d_sqdist,
                     d_row, (unsigned long long*)d_stats);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_nn_attr_sse_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, const int32_t* d_row, int64_t n_q,
                                      const void* d_a, const void* d_b, int64_t n_r, int bpv, int channels, int n_frames,
                                      uint64_t* d_sse) {
  const int64_t kMax = (int64_t)1 << 27;
  PCC_REQUIRE(ctx && d_sse && n_frames >= 1 && n_frames <= 65535 && n_q >= 0 && n_q <= kMax && n_r >= 0 && n_r <= kMax &&
                  (bpv == 1 || bpv == 2) && channels >= 1 && channels <= 4,
              PCC_E_ARG, "pcc_nn_attr_sse_frames: bad argument (n_q=%lld n_r=%lld n_frames=%d bpv=%d channels=%d)", (long long)n_q,
              (long long)n_r, n_frames, bpv, channels);
  PCC_REQUIRE(n_q == 0 || (d_qkeys && d_row && d_a), PCC_E_ARG, "pcc_nn_attr_sse_frames: null query arrays");
  PCC_REQUIRE(n_r == 0 || d_b, PCC_E_ARG, "pcc_nn_attr_sse_frames: null reference values");
  hipStream_t st = ctx->stream;
  PCC_HIP(hipMemsetAsync(d_sse, 0, (size_t)n_frames * channels * 8, st));
  if (n_q == 0 || n_r == 0) return PCC_OK;
  PccProfScope prof(ctx, "nn_attr_sse", n_q, n_r, channels, bpv);
  if (bpv == 1)
    hipLaunchKernelGGL(k_nn_attr_sse<uint8_t>, dim3(nblk(n_q, 256)), dim3(256), 0, st, d_qkeys, d_row, n_q, (const uint8_t*)d_a,
                       (const uint8_t*)d_b, n_r, channels, n_frames, (unsigned long long*)d_sse);
  else
    hipLaunchKernelGGL(k_nn_attr_sse<uint16_t>, dim3(nblk(n_q, 256)), dim3(256), 0, st, d_qkeys, d_row, n_q, (const uint16_t*)d_a,
                       (const uint16_t*)d_b, n_r, channels, n_frames, (unsigned long long*)d_sse);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// host only, no ctx: nn_search for every query on the calling thread — the kernel's traversal, for counting the nodes
// it tries and for checks where there is no device.  Not a product path.
extern "C" int pcc_nn_replay_host(const uint64_t* h_qkeys, int64_t n_q, const uint64_t* h_rkeys, int64_t n_r, uint64_t* h_sqdist,
                                  int32_t* h_row, uint32_t* h_nodes) {
  const int64_t kMax = (int64_t)1 << 27;
  PCC_REQUIRE(n_q >= 0 && n_q <= kMax && n_r >= 0 && n_r <= kMax && (n_q == 0 || h_qkeys) && (n_r == 0 || h_rkeys), PCC_E_ARG,
              "pcc_nn_replay_host: bad argument (n_q=%lld n_r=%lld)", (long long)n_q, (long long)n_r);
  for (int64_t i = 1; i < n_r; ++i) {
    PCC_REQUIRE(h_rkeys[i - 1] <= h_rkeys[i], PCC_E_ARG, "pcc_nn_replay_host: reference keys not sorted (pcc_sort_pairs)");
    PCC_REQUIRE(h_rkeys[i - 1] != h_rkeys[i], PCC_E_DUP, "pcc_nn_replay_host: duplicate reference keys");
  }
  for (int64_t i = 0; i < n_q; ++i) {
    const uint64_t qk = h_qkeys[i], frame = qk & ~NN_KEY48;
    const int64_t flo = std::lower_bound(h_rkeys, h_rkeys + n_r, frame) - h_rkeys;
    const int64_t fhi = std::upper_bound(h_rkeys, h_rkeys + n_r, frame | NN_KEY48) - h_rkeys;
    uint64_t best = ~0ull;
    int64_t best_row = -1;
    uint32_t nodes = 0;
    if (fhi > flo) nodes = nn_search(h_rkeys, flo, fhi, qk, &best, &best_row);
    if (h_sqdist) h_sqdist[i] = best;
    if (h_row) h_row[i] = (int32_t)best_row;
    if (h_nodes) h_nodes[i] = nodes;
  }
  return PCC_OK;
}
