// nn.hip — exact nearest neighbours on the int16 lattice, frame by frame: the search behind the D1 (point-to-point)
// distortion of GeometryCodec.distortion, and what consumes its pairing: the attribute error and the D2
// (point-to-plane) projection onto normals (knn.hip estimates those).  include/pcc.h has the rules; tests/nn_ref.py and
// tests/normals_ref.py restate them in numpy.  The key checks and frame offsets in front of this search and of
// knn.hip's are here too (nn_cells.h declares them).
//
// The reference of a call is what pcc_octree_encode_frames takes: Morton keys, sorted and distinct, the frame index
// above bit 48.  One thread per query searches the rows of its own frame:
//
//   seed   the two rows around the query's place in key order (clamped to the frame's rows: the neighbour in key order
//          may belong to the next frame) give the first `best`; an equal key ends the search, keys being distinct.
//   walk   nn_walk (nn_cells.h has the walk and why it ends) with `best` as its bound.  It starts at the frame's first
//          row whatever the seed was, so it measures the two seed rows again and counts them.
//
// Coordinates are the biased ones of the keys, 0 .. 65535; a per-axis difference squared fits 32 bits, the sum of
// three is formed in 64.
//
// Statistics: after the walk the wave's lanes meet again; per frame present in the wave one reduction over the lanes
// (shuffles) and then three 64-bit atomics from one lane (nn_per_frame).
#include "common.h"
#include "nn_cells.h"
#include <algorithm>

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
  offs[f] = f == n_frames ? n_r : nn_lower_bound(rkeys, 0, n_r, (uint64_t)f << 48);
}

// the 1-NN bound of nn_walk: the best (d2, row) so far; no row is left out of the walk
struct NnBest {
  uint64_t best;
  int64_t row;
  __host__ __device__ uint64_t bound() const { return best; }
  __host__ __device__ int64_t bound_row() const { return row; }
  __host__ __device__ bool seeded(int64_t) const { return false; }
  __host__ __device__ void offer(uint64_t d, int64_t r) {
    if (d < best || (d == best && r < row)) {
      best = d;
      row = r;
    }
  }
};

// the search of one query among the rows [flo, fhi) of its frame, flo < fhi: seed and walk as described above.
// Returns the nodes tried (cells tested and points measured, the two seeds included): pcc_nn_replay_host reports
// it, the kernel drops it.
__host__ __device__ static inline uint32_t nn_search(const uint64_t* __restrict__ rkeys, int64_t flo, int64_t fhi, uint64_t qk,
                                                     uint64_t* out_best, int64_t* out_row) {
  const uint32_t qx = pcc_compact3(qk >> 2), qy = pcc_compact3(qk >> 1), qz = pcc_compact3(qk);
  NnBest b = {~0ull, -1};
  uint32_t nodes = 0;
  const int64_t lo = nn_lower_bound(rkeys, flo, fhi, qk);      // the first row of the frame whose key is not below the query's
  if (lo < fhi) {
    b.best = nn_d2(qx, qy, qz, rkeys[lo]);
    b.row = lo;
    ++nodes;
  }
  if (lo > flo) {
    const uint64_t d = nn_d2(qx, qy, qz, rkeys[lo - 1]);
    ++nodes;
    if (d <= b.best) {      // the smaller row wins a tie
      b.best = d;
      b.row = lo - 1;
    }
  }
  // (0: the query's own key is in the reference, and no other point is as near)
  if (b.best != 0) nodes += nn_walk(rkeys, flo, fhi, qx, qy, qz, b);
  *out_best = b.best;
  *out_row = b.row;
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
  // every lane of the wave is here again
  nn_per_frame(valid, f, [&](int f0, bool mine, bool leader) {
    const unsigned long long d = mine ? best : 0ull, s = nn_wave_sum(d), c = nn_wave_sum(mine ? 1ull : 0ull);
    unsigned long long m = d;
    for (int off = 32; off; off >>= 1) {
      const unsigned long long o = __shfl_xor(m, off);
      m = o > m ? o : m;
    }
    if (leader) {
      atomicAdd(&stats[3 * (size_t)f0], c);
      atomicAdd(&stats[3 * (size_t)f0 + 1], s);
      atomicMax(&stats[3 * (size_t)f0 + 2], m);
    }
  });
}

// sse[f][ch] += (a[i][ch] - b[row[i]][ch])^2 over the queries i of frame f; a query without a row (-1), a row outside
// the reference or a frame index outside the call adds nothing.
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
  nn_per_frame(valid, f, [&](int f0, bool mine, bool leader) {
    const unsigned long long s0 = nn_wave_sum(mine ? e0 : 0ull), s1 = nn_wave_sum(mine ? e1 : 0ull),
                             s2 = nn_wave_sum(mine ? e2 : 0ull), s3 = nn_wave_sum(mine ? e3 : 0ull);
    if (leader) {
      unsigned long long* out = sse + (size_t)f0 * channels;
      atomicAdd(&out[0], s0);
      if (channels > 1) atomicAdd(&out[1], s1);
      if (channels > 2) atomicAdd(&out[2], s2);
      if (channels > 3) atomicAdd(&out[3], s3);
    }
  });
}

// proj[i] = ((q_i - r_row[i]) . n)^2 in float64, n = row normal_row[i] (row i without normal_row) of normals, the dot
// product as (ex nx + ey ny) + ez nz; sum[f] += proj over the queries i of frame f.  A query without a row (-1), a
// row outside the reference, a negative normal row or a frame index outside the call adds nothing (proj 0).
__global__ __launch_bounds__(256) void k_nn_d2(const uint64_t* __restrict__ qkeys, const int32_t* __restrict__ row, int64_t n_q,
                                               const uint64_t* __restrict__ rkeys, int64_t n_r, const float* __restrict__ normals,
                                               const int32_t* __restrict__ normal_row, int n_frames, double* __restrict__ proj,
                                               double* __restrict__ sum) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  int f = 0;
  double p = 0.0;
  if (i < n_q) {
    const int64_t r = row[i];
    const uint64_t qk = qkeys[i];
    const int64_t nr = normal_row ? (int64_t)normal_row[i] : i;
    f = (int)(qk >> 48);
    if (r >= 0 && r < n_r && nr >= 0 && f < n_frames) {
      valid = true;
      const uint64_t rk = rkeys[r];
      const double ex = (double)((int)pcc_compact3(qk >> 2) - (int)pcc_compact3(rk >> 2)),
                   ey = (double)((int)pcc_compact3(qk >> 1) - (int)pcc_compact3(rk >> 1)),
                   ez = (double)((int)pcc_compact3(qk) - (int)pcc_compact3(rk));
      const float* n = normals + nr * 3;
      const double d = (ex * (double)n[0] + ey * (double)n[1]) + ez * (double)n[2];
      p = d * d;
    }
    if (proj) proj[i] = p;
  }
  if (!sum) return;      // the same in every lane
  nn_per_frame(valid, f, [&](int f0, bool mine, bool leader) {
    const double s = nn_wave_sum(mine ? p : 0.0);
    if (leader) atomicAdd(&sum[f0], s);
  });
}

// ---------------------------------------------------------------- in front of both searches (nn_cells.h)
int nn_check_and_offsets(pcc_ctx* ctx, const char* who, const char* a_key, const char* keys, const uint64_t* d_rkeys, int64_t n_r,
                         const uint64_t* d_qkeys, int64_t n_q, int n_frames, const int64_t** out_offs) {
  hipStream_t st = ctx->stream;
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
  PCC_REQUIRE(!(bits & 4), PCC_E_RANGE, "%s: %s frame index is not below n_frames=%d", who, a_key, n_frames);
  PCC_REQUIRE(!(bits & 8), PCC_E_RANGE, "%s: a query key's frame index is not below n_frames=%d", who, n_frames);
  PCC_REQUIRE(!(bits & 2), PCC_E_ARG, "%s: %s not sorted (pcc_sort_pairs)", who, keys);
  PCC_REQUIRE(!(bits & 1), PCC_E_DUP, "%s: duplicate %s", who, keys);
  *out_offs = offs;
  return PCC_OK;
}

int nn_host_sorted_distinct(const char* who, const char* keys, const uint64_t* h_keys, int64_t n) {
  for (int64_t i = 1; i < n; ++i) {
    PCC_REQUIRE(h_keys[i - 1] <= h_keys[i], PCC_E_ARG, "%s: %s not sorted (pcc_sort_pairs)", who, keys);
    PCC_REQUIRE(h_keys[i - 1] != h_keys[i], PCC_E_DUP, "%s: duplicate %s", who, keys);
  }
  return PCC_OK;
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
extern "C" int pcc_nn_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, int64_t n_q, const uint64_t* d_rkeys, int64_t n_r,
                             int n_frames, uint64_t* d_sqdist, int32_t* d_row, uint64_t* d_stats) {
  PCC_REQUIRE(ctx && n_frames >= 1 && n_frames <= 65535 && n_q >= 0 && n_q <= NN_MAX_KEYS && n_r >= 0 && n_r <= NN_MAX_KEYS, PCC_E_ARG,
              "pcc_nn_frames: bad argument (n_q=%lld n_r=%lld n_frames=%d; at most 2^27 keys a side, 1 .. 65535 frames)",
              (long long)n_q, (long long)n_r, n_frames);
  PCC_REQUIRE((n_q == 0 || d_qkeys) && (n_r == 0 || d_rkeys), PCC_E_ARG, "pcc_nn_frames: null keys");
  hipStream_t st = ctx->stream;
  if (d_stats) PCC_HIP(hipMemsetAsync(d_stats, 0, (size_t)n_frames * 24, st));
  if (n_q == 0 && n_r == 0) return PCC_OK;
  const int64_t* offs;
  PCC_TRY(nn_check_and_offsets(ctx, "pcc_nn_frames", "a reference key's", "reference keys", d_rkeys, n_r, d_qkeys, n_q, n_frames,
                               &offs));
  if (n_q == 0) return PCC_OK;
  if (n_r == 0) {      // no candidate anywhere: d2 = 2^64 - 1, row = -1, statistics 0; no search kernel
    if (d_sqdist) PCC_HIP(hipMemsetAsync(d_sqdist, 0xFF, (size_t)n_q * 8, st));
    if (d_row) PCC_HIP(hipMemsetAsync(d_row, 0xFF, (size_t)n_q * 4, st));
    return PCC_OK;
  }
  if (!d_sqdist && !d_row && !d_stats) return PCC_OK;
  PccProfScope prof(ctx, "nn_frames", n_q, n_r, n_frames, 0);
  hipLaunchKernelGGL(k_nn_frames, dim3(nblk(n_q, 256)), dim3(256), 0, st, d_qkeys, n_q, d_rkeys, offs, d_sqdist, d_row,
                     (unsigned long long*)d_stats);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_nn_attr_sse_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, const int32_t* d_row, int64_t n_q,
                                      const void* d_a, const void* d_b, int64_t n_r, int bpv, int channels, int n_frames,
                                      uint64_t* d_sse) {
  PCC_REQUIRE(ctx && d_sse && n_frames >= 1 && n_frames <= 65535 && n_q >= 0 && n_q <= NN_MAX_KEYS && n_r >= 0 && n_r <= NN_MAX_KEYS &&
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

extern "C" int pcc_nn_d2_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, const int32_t* d_row, int64_t n_q, const uint64_t* d_rkeys,
                                int64_t n_r, const float* d_normals, const int32_t* d_normal_row, int n_frames, double* d_proj,
                                double* d_sum) {
  PCC_REQUIRE(ctx && n_frames >= 1 && n_frames <= 65535 && n_q >= 0 && n_q <= NN_MAX_KEYS && n_r >= 0 && n_r <= NN_MAX_KEYS, PCC_E_ARG,
              "pcc_nn_d2_frames: bad argument (n_q=%lld n_r=%lld n_frames=%d)", (long long)n_q, (long long)n_r, n_frames);
  PCC_REQUIRE(n_q == 0 || (d_qkeys && d_row), PCC_E_ARG, "pcc_nn_d2_frames: null query arrays");
  PCC_REQUIRE(n_q == 0 || n_r == 0 || (d_rkeys && d_normals), PCC_E_ARG, "pcc_nn_d2_frames: null reference keys or normals");
  hipStream_t st = ctx->stream;
  if (d_sum) PCC_HIP(hipMemsetAsync(d_sum, 0, (size_t)n_frames * 8, st));
  if (n_q == 0 || (!d_proj && !d_sum)) return PCC_OK;
  if (n_r == 0) {      // no row can be valid
    if (d_proj) PCC_HIP(hipMemsetAsync(d_proj, 0, (size_t)n_q * 8, st));
    return PCC_OK;
  }
  PccProfScope prof(ctx, "nn_d2", n_q, n_r, n_frames, 0);
  hipLaunchKernelGGL(k_nn_d2, dim3(nblk(n_q, 256)), dim3(256), 0, st, d_qkeys, d_row, n_q, d_rkeys, n_r, d_normals, d_normal_row,
                     n_frames, d_proj, d_sum);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// host only, no ctx: nn_search for every query on the calling thread — the kernel's traversal, for counting the nodes
// it tries and for checks where there is no device.  Not a product path.
extern "C" int pcc_nn_replay_host(const uint64_t* h_qkeys, int64_t n_q, const uint64_t* h_rkeys, int64_t n_r, uint64_t* h_sqdist,
                                  int32_t* h_row, uint32_t* h_nodes) {
  PCC_REQUIRE(n_q >= 0 && n_q <= NN_MAX_KEYS && n_r >= 0 && n_r <= NN_MAX_KEYS && (n_q == 0 || h_qkeys) && (n_r == 0 || h_rkeys), PCC_E_ARG,
              "pcc_nn_replay_host: bad argument (n_q=%lld n_r=%lld)", (long long)n_q, (long long)n_r);
  PCC_TRY(nn_host_sorted_distinct("pcc_nn_replay_host", "reference keys", h_rkeys, n_r));
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
