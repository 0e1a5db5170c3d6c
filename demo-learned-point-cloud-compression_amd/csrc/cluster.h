// cluster.h — DBSCAN clusters behind knn.hip's search (included by it, after outlier.h): connected components of the
// implicit neighbourhood graph by a lock-free union-find.  include/pcc.h has the rule; tests/cluster_ref.py restates it.
// cluster.hip has the entry point, with the checks, the arena and the sort.
//
//   core flags         m >= 1: k_outlier_radius<CAP> as it stands (the radius rule is the core-point test); m = 0: a fill.
//   k_cluster_init     parent[x] = x, size[x] = 0.
//   k_cluster_walk     one thread per point, one nn_walk under the constant bound radius2 (a cell AT the radius is
//                      entered).  A core point walks the rows in front of its own, [flo, i) — the edge is symmetric, the
//                      smaller side does nothing — and unites with every core point it measures within the radius.  A
//                      point that is not core walks the whole frame and keeps the nearest core point within the radius
//                      (rows come in order: among equidistant ones the first met, the smallest row, stays).  No list of
//                      neighbours is written: 4 B per point leave the kernel, beside the hooks.
//   k_cluster_flatten  behind the kernel boundary: root = find(own row or nearest core's), and the size counted at the root.
//   numbering          a sort key per point — frame | 2^28 - size for a root that survives min_points, frame n_frames
//                      for everything else — one stable radix sort (rows are in order, so equal sizes stay in root
//                      order), and the place behind the frame's first key is the label.
//   k_cluster_labels   the label of every point through its root, and the frame's counts inside the wave (nn_per_frame).
//
// This is the one kernel family here in which threads of different workgroups write to each other's data inside a
// launch (parent[]).  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so
// cluster_find / cluster_unite below are built to need no fresh read: see the comment above them.
#pragma once

#define CLUSTER_R2_MAX 4096ull                  // a walk visits every point within the radius: radius 64 bounds that
#define CLUSTER_MIN_POINTS_MAX ((int64_t)1 << 27)
#define CLUSTER_SIZE_BITS 29                    // 2^28 - size, size in 1 .. 2^27
#define CLUSTER_NO_ROW 0x7FFFFFFFFFFFFFFFll

// ---------------------------------------------------------------- the union-find
// parent[] as other threads of the launch may be changing it.  Device: relaxed agent-scope atomics, which never sit in
// L1; the compare-and-swap and the minimum execute at the memory side.  Host (the replay): one thread, plain words.
__host__ __device__ static inline uint32_t cluster_load(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
// *p = desired if *p == expected; returns what *p held
__host__ __device__ static inline uint32_t cluster_cas(uint32_t* p, uint32_t expected, uint32_t desired) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expected, desired);
#else
  const uint32_t old = *p;
  if (old == expected) *p = desired;
  return old;
#endif
}
// *p = min(*p, v)
__host__ __device__ static inline void cluster_lower(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}

// Invariant: parent[x] <= x at all times, parent[x] == x exactly for a root, and an entry only ever goes DOWN, to an
// ancestor of x: a hook (cluster_unite) changes a root's entry from x to a smaller root, the compression below lowers
// an entry to what was read as its parent's parent.  A point that has stopped being a root never is one again, and an
// ancestor stays an ancestor.
//
// So a STALE read is still an ancestor or x itself: it costs steps, never correctness.  A read that still shows x as a
// root after it was hooked leads to a compare-and-swap that fails and returns the present entry, or to "same root",
// which is true of two points that share an ancestor.
//
// Termination: cluster_find moves to a strictly smaller index with every step or ends; in cluster_unite the larger of
// the two roots strictly decreases with every failed compare-and-swap (the value returned is below it, and so is the
// other root).  Indexes are bounded below by the frame's first row.  No step waits for another thread: no fence, no
// spinning on a flag, nothing that needs another workgroup to be resident or to have run.  Keep all of that: a loop
// that can stand still is a hang (nn_cells.h says the same of its walk).
__host__ __device__ static inline uint32_t cluster_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = cluster_load(parent + x);
    if (p == x) return x;      // p < x from here on
    const uint32_t g = cluster_load(parent + p);      // g <= p: an ancestor of p, hence of x
    if (g != p) cluster_lower(parent + x, g);      // path halving: only ever an ancestor, only ever downwards
    x = g;
  }
}

// the sets of a and b become one; the LARGER root goes under the SMALLER, so a component's root is its smallest row
__host__ __device__ static inline void cluster_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cluster_find(parent, a);
    b = cluster_find(parent, b);
    if (a == b) return;
    const uint32_t big = a > b ? a : b, small = a > b ? b : a;
    const uint32_t old = cluster_cas(parent + big, big, small);
    if (old == big) return;
    a = old;      // big was hooked meanwhile: old < big is its parent now
    b = small;
  }
}

// ---------------------------------------------------------------- one point's walk
// the Best of nn_walk whose bound never moves: every point at d2 <= radius2 is measured, a cell at box distance
// radius2 is entered (bound_row is beyond every row)
struct ClusterBest {
  const uint8_t* __restrict__ core;
  uint32_t* parent;
  int64_t i;
  uint64_t radius2;
  bool is_core;
  uint64_t best_d;
  int64_t best_r;
  __host__ __device__ uint64_t bound() const { return radius2; }
  __host__ __device__ int64_t bound_row() const { return CLUSTER_NO_ROW; }
  __host__ __device__ bool seeded(int64_t r) const { return r == i; }
  __host__ __device__ void offer(uint64_t d, int64_t r) {
    if (d > radius2 || !core[r]) return;
    if (is_core) {
      cluster_unite(parent, (uint32_t)i, (uint32_t)r);      // r < i: a core point walks [flo, i)
    } else if (d < best_d) {      // rows ascend: an equidistant later row does not replace an earlier one
      best_d = d;
      best_r = r;
    }
  }
};

// row i of the frame [flo, fhi): a core point's unions; else near[i] = its nearest core point within the radius, or -1
// (near[i] = i for a core point).  Returns the nodes tried, as nn_walk counts.
__host__ __device__ static inline uint32_t cluster_point(const uint64_t* __restrict__ keys, int64_t flo, int64_t fhi, int64_t i,
                                                         const uint8_t* __restrict__ core, uint32_t* parent, uint64_t radius2,
                                                         int32_t* __restrict__ near) {
  const uint64_t qk = keys[i];
  const uint32_t qx = pcc_compact3(qk >> 2), qy = pcc_compact3(qk >> 1), qz = pcc_compact3(qk);
  ClusterBest b = {core, parent, i, radius2, core[i] != 0, ~0ull, -1};
  uint32_t tried = 0;
  if (b.is_core) {
    if (i > flo) tried = nn_walk(keys, flo, i, qx, qy, qz, b);
    near[i] = (int32_t)i;
  } else {
    tried = nn_walk(keys, flo, fhi, qx, qy, qz, b);
    near[i] = (int32_t)b.best_r;
  }
  return tried;
}

// the sort key of row i: a root whose component has at least min_points points sorts by (frame, size descending);
// everything else behind every frame
__host__ __device__ static inline uint64_t cluster_sort_key(int64_t i, int32_t root, uint32_t size, int64_t min_points, int f,
                                                            int n_frames) {
  const bool survives = root == (int32_t)i && (int64_t)size >= min_points;
  return survives ? ((uint64_t)f << CLUSTER_SIZE_BITS) | (uint64_t)((1u << 28) - size) : (uint64_t)n_frames << CLUSTER_SIZE_BITS;
}

// ---------------------------------------------------------------- kernels
__global__ void k_cluster_init(int64_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ size, uint8_t* __restrict__ core_fill) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  parent[i] = (uint32_t)i;
  size[i] = 0u;
  if (core_fill) core_fill[i] = 1;      // m = 0: every point is a core point
}

__global__ __launch_bounds__(256) void k_cluster_walk(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ offs,
                                                      const uint8_t* __restrict__ core, uint32_t* parent, uint64_t radius2,
                                                      int32_t* __restrict__ near) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(keys[i] >> 48);      // below n_frames: k_nn_check
  (void)cluster_point(keys, offs[f], offs[f + 1], i, core, parent, radius2, near);
}

// a launch of its own: the kernel boundary is what makes every hook visible.  root[i] (in place of near[i]): the root
// of the point's component, -1 for a point without one; the component's size is counted at its root.
__global__ void k_cluster_flatten(int64_t n, uint32_t* parent, int32_t* __restrict__ root, uint32_t* __restrict__ size) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t at = root[i];      // near[i]: inside [0, n) or -1
  if (at < 0) return;
  const uint32_t r = cluster_find(parent, (uint32_t)at);
  root[i] = (int32_t)r;
  atomicAdd(&size[r], 1u);
}

__global__ void k_cluster_sort_keys(const uint64_t* __restrict__ keys, int64_t n, const int32_t* __restrict__ root,
                                    const uint32_t* __restrict__ size, int64_t min_points, int n_frames, uint64_t* __restrict__ skeys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  skeys[i] = cluster_sort_key(i, root[i], size[i], min_points, (int)(keys[i] >> 48), n_frames);
}

// sorted place p holds a surviving root: its label is its place behind the frame's first key.  label_of[row] (filled
// with -1 by the host) takes it, and sizes (nullable, zeroed by the host) the size at the frame's first row + label.
__global__ void k_cluster_number(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ perm, int64_t n, int n_frames,
                                 const int64_t* __restrict__ offs, int32_t* __restrict__ label_of, uint32_t* __restrict__ sizes) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint64_t k = skeys[p];
  const int f = (int)(k >> CLUSTER_SIZE_BITS);
  if (f >= n_frames) return;
  const int64_t first = nn_lower_bound(skeys, 0, p, (uint64_t)f << CLUSTER_SIZE_BITS);      // inside [0, p]
  const int64_t label = p - first;      // below the frame's points: every label belongs to a root of the frame
  label_of[perm[p]] = (int32_t)label;      // perm[p] < n: a permutation of the rows
  if (sizes) sizes[offs[f] + label] = (1u << 28) - (uint32_t)(k & ((1ull << CLUSTER_SIZE_BITS) - 1ull));
}

// labels (in place of root) and the frame's counts: points, core points, clusters, noise points
__global__ __launch_bounds__(256) void k_cluster_labels(const uint64_t* __restrict__ keys, int64_t n, const uint8_t* __restrict__ core,
                                                        const int32_t* __restrict__ label_of, int32_t* __restrict__ labels,
                                                        unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int f = 0;
  bool is_core = false, is_root = false, noise = false;
  if (valid) {
    f = (int)(keys[i] >> 48);
    const int32_t r = labels[i];      // the root's row, or -1
    const int32_t label = r >= 0 ? label_of[r] : -1;
    labels[i] = label;
    is_core = core[i] != 0;
    is_root = r == (int32_t)i && label >= 0;
    noise = label < 0;
  }
  // every lane of the wave is here again
  nn_per_frame(valid, f, [&](int f0, bool mine, bool leader) {
    const unsigned long long c = nn_wave_sum(mine ? 1ull : 0ull), cc = nn_wave_sum(mine && is_core ? 1ull : 0ull),
                             ck = nn_wave_sum(mine && is_root ? 1ull : 0ull), cn = nn_wave_sum(mine && noise ? 1ull : 0ull);
    if (leader) {
      unsigned long long* out = counts + 4 * (size_t)f0;
      atomicAdd(&out[0], c);
      atomicAdd(&out[1], cc);
      atomicAdd(&out[2], ck);
      atomicAdd(&out[3], cn);
    }
  });
}

// ---------------------------------------------------------------- behind the C-ABI (include/pcc.h)
// the ranges of the rule's parameters and of a call, for the entry point and the replay
int cluster_args(const char* who, int64_t n, int n_frames, int m, uint64_t radius2, int64_t min_points) {
  PCC_REQUIRE(n >= 0 && n <= NN_MAX_KEYS && n_frames >= 1 && n_frames <= 65535, PCC_E_ARG,
              "%s: bad argument (n=%lld n_frames=%d; at most 2^27 keys, 1 .. 65535 frames)", who, (long long)n, n_frames);
  PCC_REQUIRE(m >= 0 && m <= 31, PCC_E_ARG, "%s: min_neighbours=%d, min_neighbours in 0 .. 31", who, m);
  PCC_REQUIRE(radius2 <= CLUSTER_R2_MAX, PCC_E_ARG, "%s: radius2=%llu, radius2 in 0 .. 4096 (cluster coarser points, p >> k, beyond)",
              who, (unsigned long long)radius2);
  PCC_REQUIRE(min_points >= 1 && min_points <= CLUSTER_MIN_POINTS_MAX, PCC_E_ARG, "%s: min_points=%lld, min_points in 1 .. 2^27", who,
              (long long)min_points);
  return PCC_OK;
}

// the launches of pcc_cluster_frames (cluster.hip has the entry point, the arena and the sort between the two halves;
// nn_cells.h declares both).  Everything runs on ctx->stream; nothing synchronises.
//   cluster_components: core flags, unions, flatten -> root (the root row of every point, -1 without), size (at the
//   roots) and skeys, the numbering's sort keys.  core_counts: n_frames x 2 words of scratch for the radius kernel.
int cluster_components(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, const int64_t* offs, int n_frames, int m, uint64_t radius2,
                       int64_t min_points, uint8_t* core, uint32_t* parent, uint32_t* size, uint64_t* core_counts, int32_t* root,
                       uint64_t* skeys) {
  hipStream_t st = ctx->stream;
  const dim3 grid(nblk(n, 256)), block(256);
  hipLaunchKernelGGL(k_cluster_init, grid, block, 0, st, n, parent, size, m == 0 ? core : (uint8_t*)nullptr);
  PCC_CHECK_LAUNCH();
  if (m > 0) {      // the radius rule is the core-point test, word for word
    PCC_HIP(hipMemsetAsync(core_counts, 0, (size_t)n_frames * 16, st));
    outlier_radius_launch(st, d_keys, n, offs, m, radius2, core, core_counts);
    PCC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_cluster_walk, grid, block, 0, st, d_keys, n, offs, (const uint8_t*)core, parent, radius2, root);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cluster_flatten, grid, block, 0, st, n, parent, root, size);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cluster_sort_keys, grid, block, 0, st, d_keys, n, (const int32_t*)root, (const uint32_t*)size, min_points,
                     n_frames, skeys);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

//   cluster_finish: skeys sorted, perm the sort's permutation -> labels in place of the roots, sizes (nullable, zeroed
//   here) and counts (zeroed by the entry).  label_of: n words of scratch (the parents' array: the flatten is behind us).
int cluster_finish(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, const int64_t* offs, int n_frames, const uint64_t* skeys,
                   const uint32_t* perm, const uint8_t* core, int32_t* label_of, int32_t* d_labels, uint32_t* d_sizes,
                   uint64_t* d_counts) {
  hipStream_t st = ctx->stream;
  const dim3 grid(nblk(n, 256)), block(256);
  if (d_sizes) PCC_HIP(hipMemsetAsync(d_sizes, 0, (size_t)n * 4, st));
  PCC_HIP(hipMemsetAsync(label_of, 0xFF, (size_t)n * 4, st));
  hipLaunchKernelGGL(k_cluster_number, grid, block, 0, st, skeys, perm, n, n_frames, offs, label_of, d_sizes);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cluster_labels, grid, block, 0, st, d_keys, n, core, (const int32_t*)label_of, d_labels,
                     (unsigned long long*)d_counts);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// ---------------------------------------------------------------- the host replay
// host only, no ctx: the kernels' functions row by row on the calling thread.  Not a product path.
static int cluster_replay(const char* who, const uint64_t* h_keys, int64_t n, int n_frames, int m, uint64_t radius2, int64_t min_points,
                          bool reversed, int32_t* h_labels, uint32_t* h_sizes, uint64_t* h_counts, uint8_t* h_core, int32_t* h_root,
                          uint32_t* h_nodes) {
  PCC_TRY(cluster_args(who, n, n_frames, m, radius2, min_points));
  PCC_REQUIRE(n == 0 || h_keys, PCC_E_ARG, "%s: null keys", who);
  PCC_TRY(nn_host_sorted_distinct(who, "keys", h_keys, n));
  std::vector<uint8_t> core;
  std::vector<uint32_t> parent, size;
  std::vector<int32_t> root, label_of;
  std::vector<int64_t> order;
  const auto ready = [&] {
    if (h_counts) std::fill(h_counts, h_counts + 4 * (size_t)n_frames, 0ull);
    if (h_sizes) std::fill(h_sizes, h_sizes + n, 0u);
    core = std::vector<uint8_t>((size_t)n, 1);
    parent = std::vector<uint32_t>((size_t)n);
    size = std::vector<uint32_t>((size_t)n, 0u);
    root = std::vector<int32_t>((size_t)n);
    label_of = std::vector<int32_t>((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
  };
  return knn_host_frames(who, h_keys, n, n_frames, ready, [&](int f, int64_t flo, int64_t fhi) {
    if (m > 0)
      knn_with_cap(m + 1, [&](auto cap) {
        for (int64_t i = flo; i < fhi; ++i)
          core[i] = outlier_radius_point<decltype(cap)::value>(h_keys, flo, fhi, i, m, radius2, true, nullptr) ? 1 : 0;
      });
    for (int64_t t = flo; t < fhi; ++t) {      // reversed: the unions arrive in the opposite order
      const int64_t i = reversed ? fhi - 1 - (t - flo) : t;
      const uint32_t nodes = cluster_point(h_keys, flo, fhi, i, core.data(), parent.data(), radius2, root.data());
      if (h_nodes) h_nodes[i] = nodes;
    }
    for (int64_t i = flo; i < fhi; ++i) {      // k_cluster_flatten
      if (root[i] < 0) continue;
      root[i] = (int32_t)cluster_find(parent.data(), (uint32_t)root[i]);
      ++size[root[i]];
    }
    // the numbering: the surviving roots in row order, stably by their key (what the device's sort does)
    order.clear();
    for (int64_t i = flo; i < fhi; ++i)
      if (cluster_sort_key(i, root[i], size[i], min_points, f, n_frames) >> CLUSTER_SIZE_BITS == (uint64_t)f) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return size[a] > size[b]; });
    for (size_t k = 0; k < order.size(); ++k) {
      label_of[order[k]] = (int32_t)k;
      if (h_sizes) h_sizes[flo + (int64_t)k] = size[order[k]];
    }
    uint64_t n_core = 0, n_noise = 0;
    for (int64_t i = flo; i < fhi; ++i) {
      const int32_t label = root[i] >= 0 ? label_of[root[i]] : -1;
      if (h_labels) h_labels[i] = label;
      if (h_core) h_core[i] = core[i];
      if (h_root) h_root[i] = root[i];
      n_core += core[i];
      n_noise += label < 0;
    }
    if (h_counts) {
      uint64_t* out = h_counts + 4 * (size_t)f;
      out[0] = (uint64_t)(fhi - flo); out[1] = n_core; out[2] = order.size(); out[3] = n_noise;
    }
  });
}

extern "C" int pcc_cluster_replay_host(const uint64_t* h_keys, int64_t n, int n_frames, int min_neighbours, uint64_t radius2,
                                       int64_t min_points, int32_t* h_labels, uint32_t* h_sizes, uint64_t* h_counts, uint8_t* h_core,
                                       int32_t* h_root, uint32_t* h_nodes) {
  return cluster_replay("pcc_cluster_replay_host", h_keys, n, n_frames, min_neighbours, radius2, min_points, false, h_labels, h_sizes,
                        h_counts, h_core, h_root, h_nodes);
}

extern "C" int pcc_cluster_replay_host_reversed(const uint64_t* h_keys, int64_t n, int n_frames, int min_neighbours, uint64_t radius2,
                                                int64_t min_points, int32_t* h_labels, uint32_t* h_sizes, uint64_t* h_counts,
                                                uint8_t* h_core, int32_t* h_root, uint32_t* h_nodes) {
  return cluster_replay("pcc_cluster_replay_host_reversed", h_keys, n, n_frames, min_neighbours, radius2, min_points, true, h_labels,
                        h_sizes, h_counts, h_core, h_root, h_nodes);
}
