// nn_cells.h — what the 1-NN search (nn.hip) and the k-NN search (knn.hip) share: distances on the biased lattice of
// the Morton keys, the lower-bound search over sorted keys, the walk over the implicit octree, the per-frame rounds
// of a wave, and the declarations of the key checks that nn.hip defines for both and of what knn.hip
// defines for cluster.hip.
#pragma once
#include "common.h"

#define NN_KEY48 0xFFFFFFFFFFFFull
#define NN_MAX_KEYS ((int64_t)1 << 27)      // keys a side of one call

__host__ __device__ static inline uint32_t nn_sq(uint32_t a, uint32_t b) {
  const uint32_t d = a > b ? a - b : b - a;      // at most 65535: the square fits 32 bits
  return d * d;
}
// the gap between coordinate q and the cell of edge 2^L that holds coordinate c, squared
__host__ __device__ static inline uint32_t nn_gap_sq(uint32_t q, uint32_t c, int L) {
  const uint32_t lo = (c >> L) << L, hi = lo | ((1u << L) - 1u);
  const uint32_t g = q < lo ? lo - q : (q > hi ? q - hi : 0u);
  return g * g;
}
__host__ __device__ static inline uint64_t nn_d2(uint32_t qx, uint32_t qy, uint32_t qz, uint64_t k) {
  return (uint64_t)nn_sq(qx, pcc_compact3(k >> 2)) + nn_sq(qy, pcc_compact3(k >> 1)) + nn_sq(qz, pcc_compact3(k));
}

// the first row of [a, b) whose key is not below want, b if there is none: at most 47 halvings, all inside [a, b)
__host__ __device__ static inline int64_t nn_lower_bound(const uint64_t* __restrict__ keys, int64_t a, int64_t b, uint64_t want) {
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (keys[mid] < want) a = mid + 1; else b = mid;
  }
  return a;
}

// the level of the largest cell that holds one of two distinct keys of a frame and not the other
__host__ __device__ static inline int nn_split_level(uint64_t a, uint64_t b) {
  return (63 - __builtin_clzll(((a ^ b) & NN_KEY48) | 1ull)) / 3;
}

// ---------------------------------------------------------------- the walk
// Sorted distinct keys are an implicit octree: the points of a cell of edge 2^L share the key bits above 3 L and lie in
// one contiguous range of rows.  One query walks the rows [flo, fhi) of its own frame in order, flo < fhi:
//
//   walk   at row r the cells that BEGIN at r are those of levels 0 .. b / 3, b the highest bit in which keys r - 1 and
//          r differ (levels 0 .. 15 at the frame's first row).  They are tried from the largest down: a cell whose box
//          distance exceeds the bound, or equals it while r > the bound's row, is left out whole — r jumps to the first
//          row behind the cell's key range (a binary search in the rest of the frame).  Cells that hold row r alone are
//          not tried: the point is measured instead, and r advances by one.  Only cells that hold points are ever
//          tried, each once, so a query tries no more nodes than its frame's octree has.
//   best   what differs between the searches.  bound() and bound_row(): the (d2, row) a candidate has to beat, read
//          once per row; seeded(r): row r was measured by the caller's seed and is neither measured nor counted again;
//          offer(d, r): a measured point.  Rows come in order, so among equidistant points the first met wins unless a
//          seed was a later row: every comparison carries the row as its tie-break.
//   state  r, the previous key and the query's three coordinates beside Best's own: scalars and static indexes, no
//          stack and no array indexed at run time, so nothing lives in scratch (DESIGN.md 6c has the register figures).
//
// Termination: every iteration moves r forward — a skip lands on a row of [r + 1, fhi], a measured or seeded point on
// r + 1 — and every binary search runs inside the frame's rows.  No step waits for another thread.  Keep both
// properties: a walk that can stand still is a hang.
//
// Returns the nodes tried: cells tested and points measured.  One function for the device and the host, so the
// replays (pcc_nn_replay_host, pcc_knn_replay_host) are the kernels' traversal.
template <typename Best>
__host__ __device__ static inline uint32_t nn_walk(const uint64_t* __restrict__ keys, int64_t flo, int64_t fhi, uint32_t qx,
                                                   uint32_t qy, uint32_t qz, Best& best) {
  uint32_t nodes = 0;
  int64_t r = flo;
  uint64_t prev = 0;
  while (r < fhi) {
    const uint64_t k = keys[r];
    int L = r == flo ? 15 : nn_split_level(prev, k);
    const uint32_t cx = pcc_compact3(k >> 2), cy = pcc_compact3(k >> 1), cz = pcc_compact3(k);
    // the cells of levels 0 .. l1 hold row r alone (key r + 1 leaves them): measuring the point is their test
    const int l1 = r + 1 < fhi ? nn_split_level(k, keys[r + 1]) : 15;
    const uint64_t bound = best.bound();
    const int64_t bound_row = best.bound_row();
    bool skipped = false;
    for (; L > l1; --L) {
      const uint64_t bd = (uint64_t)nn_gap_sq(qx, cx, L) + nn_gap_sq(qy, cy, L) + nn_gap_sq(qz, cz, L);
      ++nodes;
      if (bd > bound || (bd == bound && r > bound_row)) {
        // the first row behind the cell, whose keys are [p << 3L, (p + 1) << 3L)
        const uint64_t end = (((k & NN_KEY48) >> (3 * L)) + 1ull) << (3 * L);
        r = end <= NN_KEY48 ? nn_lower_bound(keys, r + 1, fhi, (k & ~NN_KEY48) | end)
                            : fhi;      // the cell reaches the end of the key range
        skipped = true;
        break;
      }
    }
    if (skipped) {
      if (r < fhi) prev = keys[r - 1];
      continue;
    }
    if (!best.seeded(r)) {
      best.offer((uint64_t)nn_sq(qx, cx) + nn_sq(qy, cy) + nn_sq(qz, cz), r);
      ++nodes;
    }
    prev = k;
    ++r;
  }
  return nodes;
}

// ---------------------------------------------------------------- per-frame rounds of a wave (device only)
// v summed over the wave's 64 lanes, in every lane: the xor butterfly from offset 32 down, which fixes the order in
// which a float64 sum is added up
template <typename T>
__device__ static inline T nn_wave_sum(T v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Every lane of the wave calls this, `valid` or not.  One round per frame present among the valid lanes:
// body(f0, mine, leader) runs in all 64 lanes, f0 the round's frame, `mine` whether this lane is valid and of that
// frame (the others contribute the neutral element to the body's reductions), `leader` true in the one lane that then
// issues the round's atomics.  Sorted queries of one frame: one round per wave.
template <typename Body>
__device__ static inline void nn_per_frame(bool valid, int f, Body body) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int f0 = __shfl(f, leader);
    const bool mine = valid && f == f0;
    body(f0, mine, lane == leader);
    todo &= ~__ballot(mine);      // the leader is among them: every round clears at least one bit
  }
}

// ---------------------------------------------------------------- defined in nn.hip, for both searches
// The checks in front of a search and the first row of every frame.  Reserves the arena, runs k_nn_check and
// k_nn_offsets on ctx->stream, reads the 4-byte flag back (one wait) and refuses a frame index not below n_frames
// (PCC_E_RANGE), unsorted (PCC_E_ARG) or equal (PCC_E_DUP) reference keys.  *offs (arena, n_frames + 1 rows) is filled
// only where n_r > 0.  who: the entry point's name; a_key, keys: its words for the reference side ("a reference
// key's" / "reference keys").  The query side may be empty (null, 0).
int nn_check_and_offsets(pcc_ctx* ctx, const char* who, const char* a_key, const char* keys, const uint64_t* d_rkeys, int64_t n_r,
                         const uint64_t* d_qkeys, int64_t n_q, int n_frames, const int64_t** offs);
// the same refusals for the host replays: PCC_E_ARG for unsorted, PCC_E_DUP for equal keys
int nn_host_sorted_distinct(const char* who, const char* keys, const uint64_t* h_keys, int64_t n);

// ---------------------------------------------------------------- defined in knn.hip (cluster.h), for cluster.hip
// what every entry on one key array does in front of its launches (knn.hip has the order and the arguments)
struct KnnRange {      // the rule's integer of an entry as its refusal names it, and the range it must lie in
  const char* name;
  int v, lo, hi;
};
#define KNN_NO_RANGE KnnRange{nullptr, 0, 0, 0}      // an entry without such an integer, or one that has checked its own
struct KnnNulls {      // the entry's words for null keys; whether its own pointers are there, and its words where not
  const char* keys;
  bool others_ok;
  const char* others;
};
__attribute__((visibility("hidden")))      // the library's own: no new name among its dynamic symbols
int knn_entry(pcc_ctx* ctx, const char* who, KnnRange k, const uint64_t* d_keys, int64_t n, int n_frames, KnnNulls nulls,
              void* d_frame, size_t frame_bytes, size_t reserve, const int64_t** offs);
// the parameter ranges of the clustering rule, and the two halves of its launches around the numbering's sort
int cluster_args(const char* who, int64_t n, int n_frames, int m, uint64_t radius2, int64_t min_points);
int cluster_components(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, const int64_t* offs, int n_frames, int m, uint64_t radius2,
                       int64_t min_points, uint8_t* core, uint32_t* parent, uint32_t* size, uint64_t* core_counts, int32_t* root,
                       uint64_t* skeys);
int cluster_finish(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, const int64_t* offs, int n_frames, const uint64_t* skeys,
                   const uint32_t* perm, const uint8_t* core, int32_t* label_of, int32_t* d_labels, uint32_t* d_sizes,
                   uint64_t* d_counts);
