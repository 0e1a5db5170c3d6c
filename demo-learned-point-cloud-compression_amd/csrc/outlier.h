// outlier.h — outlier removal behind knn.hip's search (included by it): the statistical rule (a score fused behind the
// k-NN search, exact frame sums, a threshold formed on the host between two kernels) and the radius rule (the same walk
// under a bound that never passes the radius).  include/pcc.h has both rules; tests/outlier_ref.py restates them.
//
//   k_outlier_scores   one thread per point: knn_search, then q = sum of floor(16 sqrt(d2)) over the list, in the same
//                      thread; q (8 B per point) is all that reaches memory beside the frame's sums — nothing of shape
//                      [n][k].  The sums (q, the two halves of q^2, the count) are reduced per frame inside the wave
//                      (nn_per_frame: a wave across a frame boundary takes one round per frame) and then added by one
//                      lane with 64-bit atomics; they are integers, so the order does not matter.
//   k_outlier_mask     keep = q <= T[frame], and the frame's kept count the same way.
//   k_outlier_radius   the list holds m + 1 entries (the point itself first) and the walk's bound is
//                      min(last slot, radius2 + 1) (KnnBest<CAP, true>): a cell farther than the radius is never
//                      entered, so an isolated point stops after the cells inside its radius.  Seeds enter the list wherever they lie; beyond
//                      the radius they leave the bound at radius2 + 1.  Every point within the radius lies in cells
//                      whose box distance is at most radius2, below that bound, so it is pruned only by a list whose
//                      last slot is already nearer: slot m ends at d2 <= radius2 exactly when the unbounded search's does.
//   compaction         flags of the input rows (through pcc_rows_index' index), pcc_scan_exclusive_u32, the kept rows'
//                      places inside their frames, the kept rows before every frame.
#pragma once

#define OUTLIER_D2_MAX (3ull * 65535ull * 65535ull)

// floor(sqrt(x)) for x < 2^42: float64's root, then the integer fix-up, so no rounding of sqrt decides it
__host__ __device__ static inline uint64_t outlier_isqrt(uint64_t x) {
  uint64_t r = (uint64_t)sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// q of a finished list: sum over its entries of floor(16 sqrt(d2)) = isqrt(d2 << 8); below 32 * 2^21 = 2^26
template <int CAP>
__host__ __device__ static inline uint64_t outlier_score(const KnnList<CAP>& L, int k) {
  uint64_t q = 0;
#pragma unroll
  for (int j = 0; j < CAP; ++j)
    if (j >= CAP - k && L.d[j] != KNN_NO_DIST) q += outlier_isqrt(L.d[j] << 8);
  return q;
}

template <int CAP>
__host__ __device__ static inline uint64_t outlier_score_point(const uint64_t* __restrict__ keys, int64_t flo, int64_t fhi,
                                                               int64_t i, int k, uint32_t* nodes) {
  KnnList<CAP> L;
  knn_init(L, k);
  const uint32_t tried = knn_search(keys, flo, fhi, keys[i], k, L);
  if (nodes) *nodes = tried;
  return outlier_score(L, k);
}

__host__ __device__ static inline bool outlier_keep(uint64_t q, uint64_t threshold) { return q <= threshold; }

// whether row i has at least m other points of its frame [flo, fhi) within radius2 (<= OUTLIER_D2_MAX): slot m of its
// list of m + 1.  bounded: knn_search's seed and walk under KnnBest<CAP, true>, written out here — through the shared
// function k_outlier_radius<8> took two more registers and lost a wave of occupancy; else knn_search itself.
// *nodes: the nodes tried, as knn_search counts.
template <int CAP>
__host__ __device__ static inline bool outlier_radius_point(const uint64_t* __restrict__ keys, int64_t flo, int64_t fhi, int64_t i,
                                                            int m, uint64_t radius2, bool bounded, uint32_t* nodes) {
  const int k = m + 1;
  const uint64_t qk = keys[i];
  KnnList<CAP> L;
  knn_init(L, k);
  uint32_t tried;
  if (!bounded) {
    tried = knn_search(keys, flo, fhi, qk, k, L);
  } else {
    const uint32_t qx = pcc_compact3(qk >> 2), qy = pcc_compact3(qk >> 1), qz = pcc_compact3(qk);
    const int64_t n_f = fhi - flo;
    const int64_t k_eff = n_f < k ? n_f : k;
    const int64_t lo = nn_lower_bound(keys, flo, fhi, qk);
    int64_t s0 = lo - k_eff / 2;      // knn_search's seed rows
    if (s0 > fhi - k_eff) s0 = fhi - k_eff;
    if (s0 < flo) s0 = flo;
    KnnBest<CAP, true> b = {L, s0, s0 + k_eff, radius2 + 1};
    for (int64_t r = b.s0; r < b.s1; ++r) knn_insert(L, nn_d2(qx, qy, qz, keys[r]), (int32_t)r);
    tried = (uint32_t)k_eff;
    if (k_eff != n_f) tried += nn_walk(keys, flo, fhi, qx, qy, qz, b);
  }
  if (nodes) *nodes = tried;
  return L.d[CAP - 1] <= radius2;      // a free slot holds 2^64 - 1: a frame of at most m points keeps nothing
}

// radius2 as the searches take it: no two points lie farther apart than OUTLIER_D2_MAX
static inline uint64_t outlier_radius2(uint64_t radius2) { return radius2 < OUTLIER_D2_MAX ? radius2 : OUTLIER_D2_MAX; }

// ---------------------------------------------------------------- kernels
template <int CAP>
__global__ __launch_bounds__(256) void k_outlier_scores(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ offs,
                                                        int k, uint64_t* __restrict__ q, unsigned long long* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int f = 0;
  unsigned long long qi = 0;
  if (valid) {
    f = (int)(keys[i] >> 48);      // below n_frames: k_nn_check
    qi = outlier_score_point<CAP>(keys, offs[f], offs[f + 1], i, k, nullptr);
    q[i] = qi;
  }
  // every lane of the wave is here again
  nn_per_frame(valid, f, [&](int f0, bool mine, bool leader) {
    const unsigned long long v = mine ? qi : 0ull, sq = v * v;      // q < 2^26: the square fits
    const unsigned long long s1 = nn_wave_sum(v), lo = nn_wave_sum(sq & 0xFFFFFFFFull), hi = nn_wave_sum(sq >> 32),
                             c = nn_wave_sum(mine ? 1ull : 0ull);
    if (leader) {
      unsigned long long* out = sums + 4 * (size_t)f0;
      atomicAdd(&out[0], s1);
      atomicAdd(&out[1], lo);
      atomicAdd(&out[2], hi);
      atomicAdd(&out[3], c);
    }
  });
}

__global__ __launch_bounds__(256) void k_outlier_mask(const uint64_t* __restrict__ keys, int64_t n, const uint64_t* __restrict__ q,
                                                      const uint64_t* __restrict__ threshold, uint8_t* __restrict__ keep,
                                                      unsigned long long* __restrict__ kept) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int f = 0;
  bool k = false;
  if (valid) {
    f = (int)(keys[i] >> 48);
    k = outlier_keep(q[i], threshold[f]);
    keep[i] = k ? 1 : 0;
  }
  nn_per_frame(valid, f, [&](int f0, bool mine, bool leader) {
    const unsigned long long c = nn_wave_sum(mine && k ? 1ull : 0ull);
    if (leader) atomicAdd(&kept[f0], c);
  });
}

template <int CAP>
__global__ __launch_bounds__(256) void k_outlier_radius(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ offs,
                                                        int m, uint64_t radius2, uint8_t* __restrict__ keep,
                                                        unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int f = 0;
  bool k = false;
  if (valid) {
    f = (int)(keys[i] >> 48);
    k = outlier_radius_point<CAP>(keys, offs[f], offs[f + 1], i, m, radius2, true, nullptr);
    keep[i] = k ? 1 : 0;
  }
  nn_per_frame(valid, f, [&](int f0, bool mine, bool leader) {
    const unsigned long long c = nn_wave_sum(mine ? 1ull : 0ull), kc = nn_wave_sum(mine && k ? 1ull : 0ull);
    if (leader) {
      atomicAdd(&counts[2 * (size_t)f0], c);
      atomicAdd(&counts[2 * (size_t)f0 + 1], kc);
    }
  });
}

// flag and mask of input row i: its distinct row's keep byte; a dropped row (index -1) or an index outside the keys: 0
__global__ void k_outlier_row_flags(const int32_t* __restrict__ index, int64_t n, const uint8_t* __restrict__ keep, int64_t n_keys,
                                    uint32_t* __restrict__ flags, uint8_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t r = index[i];
  const uint32_t k = r >= 0 && r < n_keys && keep[r] ? 1u : 0u;
  flags[i] = k;
  if (mask) mask[i] = (uint8_t)k;
}

// a kept row's place inside its own frame, written at its rank among the call's kept rows
__global__ void k_outlier_kept_rows(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ excl, int64_t n,
                                    const int64_t* __restrict__ offs, int n_frames, uint32_t* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flags[i]) return;
  int a = 0, b = n_frames;      // the last frame f with offs[f] <= i: inside [0, n_frames)
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (offs[mid] <= i) a = mid; else b = mid;
  }
  rows[excl[i]] = (uint32_t)(i - offs[a]);
}

// kept_offs[f] = the kept rows in front of frame f; kept_offs[n_frames] = all of them
__global__ void k_outlier_kept_offsets(const uint32_t* __restrict__ excl, const uint32_t* __restrict__ total, int64_t n,
                                       const int64_t* __restrict__ offs, int n_frames, int64_t* __restrict__ kept_offs) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_frames) return;
  const int64_t o = offs[f];
  kept_offs[f] = o >= 0 && o < n ? (int64_t)excl[o] : (o >= n ? (int64_t)total[0] : 0);
}

// dst row t = src row rows[t], rows of row_units units of T that lie pitch_units apart in src and tight in dst: what
// pcc_gather_rows does for rows it refuses (6-byte int16 points, 3-byte colours, views with a pitch).  A row outside
// the n_src source rows is left as zeros.
template <typename T>
__global__ void k_gather_rows_pitched(const T* __restrict__ src, int64_t n_src, int64_t pitch_units, const uint32_t* __restrict__ rows,
                                      int64_t n, int row_units, T* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = t / row_units;
  if (row >= n) return;
  const int j = (int)(t - row * row_units);
  const int64_t from = rows[row];
  dst[t] = from < n_src ? src[from * pitch_units + j] : (T)0;
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
extern "C" int pcc_outlier_scores_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int k, uint64_t* d_scores,
                                         uint64_t* d_sums) {
  const int64_t* offs;
  PCC_TRY(knn_entry(ctx, "pcc_outlier_scores_frames", {"k", k, 3, 32}, d_keys, n, n_frames,
                    {"null keys", d_sums && (n == 0 || d_scores), "null output"}, d_sums, 32, 0, &offs));
  if (!offs) return PCC_OK;
  PccProfScope prof(ctx, "outlier_scores", n, k, n_frames, 0);
  knn_with_cap(k, [&](auto cap) {
    hipLaunchKernelGGL(k_outlier_scores<decltype(cap)::value>, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, d_keys, n, offs, k,
                       d_scores, (unsigned long long*)d_sums);
  });
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_outlier_mask_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, const uint64_t* d_scores,
                                       const uint64_t* d_threshold, uint8_t* d_keep, uint64_t* d_kept) {
  const int64_t* offs;      // the checks: a frame index indexes d_threshold and d_kept
  PCC_TRY(knn_entry(ctx, "pcc_outlier_mask_frames", KNN_NO_RANGE, d_keys, n, n_frames,
                    {"null arg", d_kept && d_threshold && (n == 0 || (d_scores && d_keep)), "null arg"}, d_kept, 8, 0, &offs));
  if (!offs) return PCC_OK;
  PccProfScope prof(ctx, "outlier_mask", n, n_frames, 0, 0);
  hipLaunchKernelGGL(k_outlier_mask, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, d_keys, n, d_scores, d_threshold, d_keep,
                     (unsigned long long*)d_kept);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// the radius rule's kernel for a list of m + 1: the entry below, and the core flags of cluster.h; counts is zeroed
static void outlier_radius_launch(hipStream_t st, const uint64_t* d_keys, int64_t n, const int64_t* offs, int m, uint64_t radius2,
                                  uint8_t* d_keep, uint64_t* d_counts) {
  knn_with_cap(m + 1, [&](auto cap) {
    hipLaunchKernelGGL(k_outlier_radius<decltype(cap)::value>, dim3(nblk(n, 256)), dim3(256), 0, st, d_keys, n, offs, m, radius2,
                       d_keep, (unsigned long long*)d_counts);
  });
}

extern "C" int pcc_outlier_radius_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int min_neighbours,
                                         uint64_t radius2, uint8_t* d_keep, uint64_t* d_counts) {
  const int64_t* offs;
  PCC_TRY(knn_entry(ctx, "pcc_outlier_radius_frames", {"min_neighbours", min_neighbours, 1, 31}, d_keys, n, n_frames,
                    {"null keys", d_counts && (n == 0 || d_keep), "null output"}, d_counts, 16, 0, &offs));
  if (!offs) return PCC_OK;
  PccProfScope prof(ctx, "outlier_radius", n, min_neighbours, n_frames, 0);
  outlier_radius_launch(ctx->stream, d_keys, n, offs, min_neighbours, outlier_radius2(radius2), d_keep, d_counts);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_outlier_compact_rows(pcc_ctx* ctx, const int32_t* d_index, int64_t n, const uint8_t* d_keep, int64_t n_keys,
                                        const int64_t* d_offsets, int n_frames, uint8_t* d_mask, uint32_t* d_kept_rows,
                                        int64_t* d_kept_offsets) {
  PCC_REQUIRE(ctx && n >= 0 && n < ((int64_t)1 << 31) && n_keys >= 0 && n_frames >= 1 && n_frames <= 65535, PCC_E_ARG,
              "pcc_outlier_compact_rows: bad argument (n=%lld keys=%lld n_frames=%d)", (long long)n, (long long)n_keys, n_frames);
  PCC_REQUIRE(d_offsets && d_kept_offsets && (n == 0 || (d_index && d_kept_rows)) && (n_keys == 0 || d_keep), PCC_E_ARG,
              "pcc_outlier_compact_rows: null arg");
  hipStream_t st = ctx->stream;
  if (n == 0) {
    PCC_HIP(hipMemsetAsync(d_kept_offsets, 0, (size_t)(n_frames + 1) * 8, st));
    return PCC_OK;
  }
  PCC_TRY(pcc_arena_reserve(ctx, 2 * pcc_align((size_t)n * 4) + pcc_scan_scratch_bytes(n) + 512));
  uint32_t* flags = (uint32_t*)pcc_arena_alloc(ctx, (size_t)n * 4);
  uint32_t* excl = (uint32_t*)pcc_arena_alloc(ctx, (size_t)n * 4);
  uint32_t* total = (uint32_t*)pcc_arena_alloc(ctx, 4);
  if (!flags || !excl || !total) return PCC_E_NOMEM;
  PccProfScope prof(ctx, "outlier_compact", n, n_keys, n_frames, 0);
  hipLaunchKernelGGL(k_outlier_row_flags, dim3(nblk(n, 256)), dim3(256), 0, st, d_index, n, d_keep, n_keys, flags, d_mask);
  PCC_CHECK_LAUNCH();
  PCC_TRY(pcc_scan_exclusive_u32(ctx, flags, excl, n, total));
  hipLaunchKernelGGL(k_outlier_kept_rows, dim3(nblk(n, 256)), dim3(256), 0, st, (const uint32_t*)flags, (const uint32_t*)excl, n,
                     d_offsets, n_frames, d_kept_rows);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_outlier_kept_offsets, dim3(nblk(n_frames + 1, 64)), dim3(64), 0, st, (const uint32_t*)excl,
                     (const uint32_t*)total, n, d_offsets, n_frames, d_kept_offsets);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}
template <typename T>
static void gather_pitched_launch(hipStream_t st, const void* d_src, int64_t n_src, int64_t pitch_bytes, const uint32_t* d_rows,
                                  int64_t n, int row_bytes, void* d_dst) {
  const int units = row_bytes / (int)sizeof(T);
  hipLaunchKernelGGL(k_gather_rows_pitched<T>, dim3(nblk(n * units, 256)), dim3(256), 0, st, (const T*)d_src, n_src,
                     pitch_bytes / (int64_t)sizeof(T), d_rows, n, units, (T*)d_dst);
}

extern "C" int pcc_gather_rows_pitched(pcc_ctx* ctx, const void* d_src, int64_t n_src, int64_t pitch_bytes, const uint32_t* d_rows,
                                       int64_t n, int row_bytes, void* d_dst) {
  PCC_REQUIRE(ctx && n >= 0 && n_src >= 0 && row_bytes > 0 && row_bytes <= 4096 && pitch_bytes >= row_bytes, PCC_E_ARG,
              "pcc_gather_rows_pitched: bad argument (n=%lld n_src=%lld row_bytes=%d pitch_bytes=%lld)", (long long)n,
              (long long)n_src, row_bytes, (long long)pitch_bytes);
  PCC_REQUIRE(n == 0 || (d_src && d_rows && d_dst), PCC_E_ARG, "pcc_gather_rows_pitched: null arg");
  if (n == 0) return PCC_OK;
  PccProfScope prof(ctx, "gather_rows_pitched", n, row_bytes, pitch_bytes, 0);
  const uintptr_t all = (uintptr_t)d_src | (uintptr_t)d_dst | (uintptr_t)pitch_bytes | (uintptr_t)row_bytes;      // the widest unit all share
  if (all % 4 == 0) gather_pitched_launch<uint32_t>(ctx->stream, d_src, n_src, pitch_bytes, d_rows, n, row_bytes, d_dst);
  else if (all % 2 == 0) gather_pitched_launch<uint16_t>(ctx->stream, d_src, n_src, pitch_bytes, d_rows, n, row_bytes, d_dst);
  else gather_pitched_launch<uint8_t>(ctx->stream, d_src, n_src, pitch_bytes, d_rows, n, row_bytes, d_dst);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// ---------------------------------------------------------------- the host replay
// host only, no ctx: the kernels' functions for every row on the calling thread.  Not a product path.
extern "C" uint64_t pcc_outlier_isqrt_host(uint64_t x) { return x < (1ull << 42) ? outlier_isqrt(x) : ~0ull; }

extern "C" int pcc_outlier_replay_host(const uint64_t* h_keys, int64_t n, int n_frames, int k, int min_neighbours, uint64_t radius2,
                                       const uint64_t* h_threshold, uint64_t* h_scores, uint64_t* h_sums, uint8_t* h_keep,
                                       uint32_t* h_nodes, uint8_t* h_keep_radius, uint32_t* h_nodes_radius,
                                       uint8_t* h_keep_unbounded, uint32_t* h_nodes_unbounded) {
  const int m = min_neighbours;
  PCC_REQUIRE(k >= 3 && k <= 32 && m >= 1 && m <= 31 && n >= 0 && n <= NN_MAX_KEYS && n_frames >= 1 && n_frames <= 65535 &&
                  (n == 0 || h_keys),
              PCC_E_ARG,
              "pcc_outlier_replay_host: bad argument (n=%lld n_frames=%d k=%d min_neighbours=%d; k in 3 .. 32, min_neighbours in "
              "1 .. 31, at most 2^27 keys, 1 .. 65535 frames)",
              (long long)n, n_frames, k, m);
  PCC_REQUIRE(!h_keep || (h_threshold && h_scores), PCC_E_ARG, "pcc_outlier_replay_host: keep bytes need thresholds and scores");
  PCC_TRY(nn_host_sorted_distinct("pcc_outlier_replay_host", "keys", h_keys, n));
  const uint64_t r2 = outlier_radius2(radius2);
  const auto ready = [&] {
    if (h_sums) std::fill(h_sums, h_sums + 4 * (size_t)n_frames, 0ull);
  };
  return knn_host_frames("pcc_outlier_replay_host", h_keys, n, n_frames, ready, [&](int f, int64_t flo, int64_t fhi) {
    uint64_t* sums = h_sums ? h_sums + 4 * (size_t)f : nullptr;
    if (h_scores || h_sums || h_nodes)
      knn_with_cap(k, [&](auto cap) {
        for (int64_t i = flo; i < fhi; ++i) {
          uint32_t nodes;
          const uint64_t q = outlier_score_point<decltype(cap)::value>(h_keys, flo, fhi, i, k, &nodes), sq = q * q;
          if (h_scores) h_scores[i] = q;
          if (h_nodes) h_nodes[i] = nodes;
          if (sums) {
            sums[0] += q; sums[1] += sq & 0xFFFFFFFFull; sums[2] += sq >> 32; sums[3] += 1;
          }
        }
      });
    if (h_keep)
      for (int64_t i = flo; i < fhi; ++i) h_keep[i] = outlier_keep(h_scores[i], h_threshold[f]) ? 1 : 0;
    for (int pass = 0; pass < 2; ++pass) {
      const bool bounded = pass == 0;
      uint8_t* keep = bounded ? h_keep_radius : h_keep_unbounded;
      uint32_t* tried = bounded ? h_nodes_radius : h_nodes_unbounded;
      if (!keep && !tried) continue;
      knn_with_cap(m + 1, [&](auto cap) {
        for (int64_t i = flo; i < fhi; ++i) {
          uint32_t nodes;
          const bool kept = outlier_radius_point<decltype(cap)::value>(h_keys, flo, fhi, i, m, r2, bounded, &nodes);
          if (keep) keep[i] = kept ? 1 : 0;
          if (tried) tried[i] = nodes;
        }
      });
    }
  });
}
