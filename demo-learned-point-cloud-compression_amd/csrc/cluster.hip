// cluster.hip — pcc_cluster_frames (include/pcc.h has the rule): the checks, the arena and the sort around the kernels
// of cluster.h, which live with the search they share in knn.hip.
//
//   launches   checks (k_nn_check, k_nn_offsets) | init, core flags (m >= 1), walk + unions, flatten, sort keys | the
//              radix sort's passes | number, labels + counts.
//   waits      one, in front: the flag of the checks.  The counts are the caller's to read behind a wait of its own.
//   memory     per point 1 B core flag, 3 x 4 B (parents, later the roots' labels; sizes; the sort's permutation), 8 B
//              sort key, and the sort's own scratch; the roots pass through d_labels.  No host array of size n.
#include "common.h"
#include "nn_cells.h"

extern "C" int pcc_cluster_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int min_neighbours, uint64_t radius2,
                                  int64_t min_points, int32_t* d_labels, uint32_t* d_sizes, uint64_t* d_counts) {
  PCC_REQUIRE(ctx, PCC_E_ARG, "pcc_cluster_frames: null ctx");
  PCC_TRY(cluster_args("pcc_cluster_frames", n, n_frames, min_neighbours, radius2, min_points));
  // One reservation for the whole call in front: the checks reserve again (less, so the arena stays where it is) and
  // take the first rows; the arrays below follow them, and the sort runs inside what is left.
  const size_t n4 = pcc_align((size_t)n * 4);
  const size_t whole = pcc_align((size_t)(n_frames + 1) * 8) + 1024 + pcc_align((size_t)n) + 3 * n4 + pcc_align((size_t)n * 8) +
                       pcc_align((size_t)n_frames * 16) + pcc_sort_scratch_bytes(n);
  const int64_t* offs;      // the ranges are cluster_args' above; knn_entry zeroes d_counts and reserves before the key checks
  PCC_TRY(knn_entry(ctx, "pcc_cluster_frames", KNN_NO_RANGE, d_keys, n, n_frames,
                    {"null keys", d_counts && (n == 0 || d_labels), "null output"}, d_counts, 32, whole, &offs));
  if (!offs) return PCC_OK;
  uint8_t* core = (uint8_t*)pcc_arena_alloc(ctx, (size_t)n);
  uint32_t* parent = (uint32_t*)pcc_arena_alloc(ctx, (size_t)n * 4);      // behind the flatten: the labels of the roots
  uint32_t* size = (uint32_t*)pcc_arena_alloc(ctx, (size_t)n * 4);
  uint32_t* perm = (uint32_t*)pcc_arena_alloc(ctx, (size_t)n * 4);
  uint64_t* skeys = (uint64_t*)pcc_arena_alloc(ctx, (size_t)n * 8);
  uint64_t* core_counts = (uint64_t*)pcc_arena_alloc(ctx, (size_t)n_frames * 16);
  if (!core || !parent || !size || !perm || !skeys || !core_counts) return PCC_E_NOMEM;
  PccProfScope prof(ctx, "cluster_frames", n, min_neighbours, (int64_t)radius2, n_frames);
  PCC_TRY(cluster_components(ctx, d_keys, n, offs, n_frames, min_neighbours, radius2, min_points, core, parent, size, core_counts,
                             d_labels, skeys));
  // frame | 2^28 - size ends below bit 29 + 16: bytes 0 .. 3, byte 4 from 8 frames on (n_frames itself is a key), byte 5 from 2048
  PCC_TRY(pcc_sort_pairs_bytes_reserved(ctx, skeys, perm, n, 0x0Fu | (n_frames >= 8 ? 0x10u : 0u) | (n_frames >= 2048 ? 0x20u : 0u)));
  return cluster_finish(ctx, d_keys, n, offs, n_frames, skeys, perm, core, (int32_t*)parent, d_labels, d_sizes, d_counts);
}
