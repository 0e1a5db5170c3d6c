/*
 * pcc.h — C-ABI of libpcc_hip.so, the MI355X (gfx950) codec hot path.
 *
 * This is the drop-in boundary for the path
 *     CompressionPipeline.compress()    sender/encoder/codec_pipeline.py:196
 *     DecompressionPipeline.decompress() receiver/decoder/codec_parallel.py:141
 * of ikt-luh/Demo-Learned-Point-Cloud-Compression.  In the reference that path
 * crosses into native code through four third-party bindings that are NOT in
 * the reference tree (MinkowskiEngine pybind, CompressAI's rANS pybind, the
 * tmc3 subprocess, the `bitstream` Cython module).
 * Each entry point below names the reference call site it serves.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures;
 *   - `d_` prefix  = pointer into device (HBM) memory, `h_` = host memory;
 *   - every device op is enqueued on the ctx stream and is asynchronous unless
 *     it returns a count through a host pointer (then it synchronises the
 *     stream once before returning);
 *   - return value: 0 = ok, negative = error (pcc_last_error() has the text);
 *     the library never throws across the ABI;
 *   - caller owns inputs and outputs; scratch comes from a ctx-owned arena
 *     that is valid until the next call on the same ctx;
 *   - one ctx per in-flight compress()/decompress() call ("slot"): the
 *     reference runs up to 3 concurrent calls (sender/encoder/encoder.py:50).
 *
 * Data layout (HBM)
 *   coords  int32 [N,4]  rows (b,x,y,z), coordinates multiples of the tensor
 *                        stride, each in [-32768,32767], b in [0,65535]
 *   keys    uint64 [N]   Morton key: b<<48 | interleave(x+32768,y+32768,z+32768)
 *                        (x is the top bit of each triple).  Rows of every
 *                        sparse tensor are kept sorted by this key.
 *   feats   float32 [N,C] row-major
 *   nbr     int32 [K,N]  rule book, out-stationary: nbr[k*N+n] = input row
 *                        feeding output row n through kernel offset k, -1 if
 *                        absent.  3^3: k=(dx+1)*9+(dy+1)*3+(dz+1); 2^3: k=octant
 *                        = xbit<<2|ybit<<1|zbit.
 *   weights float32 [K,Cin,Cout], bias float32 [Cout]
 *
 * Arithmetic contract (what the parity tests check bit-for-bit)
 *   out[n][co] = bias[co]; for k ascending (present neighbours only), for ci
 *   ascending: out = fmaf(in[nbr[k][n]][ci], W[k][ci][co], out); then ReLU if
 *   asked.  Evaluated with v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32
 *   (exact k-ordered fmaf chains) or scalar fmaf; never atomics.
 *   The conv3 + occupancy-head layers of g_s (pcc_sparse_conv_head*, which run
 *   on the 8 N generative children of a level) visit the neighbours in
 *   SIBLINGS-FIRST order: first those inside the output row's own aligned block
 *   of 8 rows (nbr >> 3 == n >> 3: the children of the row's parent, itself
 *   included), k ascending, then the others, k ascending.  MinkowskiEngine's
 *   own order depends on atomics, so the order is this build's definition; it
 *   makes a parent's 8 x 8 sibling pairs one dense register-resident product
 *   (csrc/convup.h).  oracle/pcc_oracle.c states both orders.
 */
#ifndef PCC_H
#define PCC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCC_ABI_VERSION 1

/* error codes */
#define PCC_OK 0
#define PCC_E_ARG (-1)      /* bad argument / unsupported shape            */
#define PCC_E_HIP (-2)      /* HIP runtime error                           */
#define PCC_E_RANGE (-3)    /* coordinate / batch index out of range       */
#define PCC_E_DUP (-4)      /* duplicate coordinates in input              */
#define PCC_E_STREAM (-5)   /* corrupt or truncated bitstream              */
#define PCC_E_NOMEM (-6)

typedef struct pcc_ctx pcc_ctx;

int pcc_abi_version(void);
const char* pcc_last_error(void);

/* ctx = device + stream + scratch arena.  `stream` is a hipStream_t passed as
 * void* (NULL = default stream). */
pcc_ctx* pcc_create(int device, void* stream);
void pcc_destroy(pcc_ctx* ctx);
int pcc_set_stream(pcc_ctx* ctx, void* stream);
int pcc_sync(pcc_ctx* ctx);
/* start/stop a hipEvent pair on the ctx stream; elapsed returns ms of the last
 * completed pair (used by bench.py for the per-kernel roofline figure). */
int pcc_timer_start(pcc_ctx* ctx);
int pcc_timer_stop(pcc_ctx* ctx);
int pcc_timer_elapsed_ms(pcc_ctx* ctx, float* h_ms);

/* per-launch profiler: when enabled, every device entry point below brackets
 * its launches with a hipEvent pair on the ctx stream.  pcc_prof_get returns
 * the op name, its elapsed ms and four shape numbers (op-specific; for
 * sparse_conv: n_out, cin, cout, k_vol).  Used by bench.py for the roofline
 * figure of the dominant kernel. */
int pcc_prof_enable(pcc_ctx* ctx, int on);
/* restrict the records to entry points whose op name starts with the prefix
 * ("sparse_conv", "convT_gen", ...; NULL or "" = all) and, when d0 >= 0, whose
 * first recorded dimension (output rows) equals d0.  An event pair costs a few
 * microseconds of stream bubble, so a timed run brackets only what it reads. */
int pcc_prof_only(pcc_ctx* ctx, const char* h_op_prefix, int64_t d0);
int pcc_prof_count(pcc_ctx* ctx);
int pcc_prof_get(pcc_ctx* ctx, int i, char* h_op, int cap, float* h_ms,
                 int64_t* h_dims);
/* number of entries >= 0 (active pairs of a rule book) */
int pcc_count_nonneg(pcc_ctx* ctx, const int32_t* d_p, int64_t n,
                     int64_t* h_count);

/* ---- coordinate keys and ordering ------------------------------------- */

/* replaces: MinkowskiEngine coordinate-map insertion inside every
 * ME.SparseTensor(...) ctor (codec_pipeline.py:262,308; codec_parallel.py:296,
 * 309,411).  d_flag (int32[1], device) is OR-ed with 1 if any coordinate is
 * out of range. */
int pcc_morton_keys(pcc_ctx* ctx, const int32_t* d_coords, int64_t n,
                    uint64_t* d_keys, int32_t* d_flag);
/* the same for a sequence of frames as their rows come: d_xyz = the frames'
 * [n_f, 3] rows concatenated, int16 (elem_bytes 2) or int32 (4); frame f =
 * rows d_frame_offsets[f] .. d_frame_offsets[f+1] (n_frames+1 entries in
 * device memory, 1 <= n_frames <= 65535) gets batch index f.  *d_flag |= 1
 * for a coordinate outside [-32768, 32767]. */
int pcc_morton_keys_frames(pcc_ctx* ctx, const void* d_xyz, int elem_bytes,
                           int64_t n, const int64_t* d_frame_offsets,
                           int n_frames, uint64_t* d_keys, int32_t* d_flag);
/* THE METRIC RULE of the frame codec (GeometryCodec's voxel / origin), stated
 * here once; tests/metric_ref.py restates it in numpy.  With voxel v > 0 and
 * origin o = (ox, oy, oz), all float32, per coordinate in float32 arithmetic:
 *   forwards   q = rint((x - o) / v): one IEEE subtraction, one IEEE correctly
 *     rounded division, then round-half-to-even.  Not a multiplication by a
 *     reciprocal, nothing contracted; f32 denormals are kept.  q is tested ON
 *     THE FLOAT, !(q >= -32768 && q <= 32767), before it becomes an integer;
 *   backwards  x = o + t * v: one multiplication, then one addition, with
 *     t = c for a lattice point c and, for a cell c of level of detail k,
 *     t = (c << k) + (2^k - 1) / 2, the centre of the cell's lattice points: a
 *     half-integer, exact in float32 for every cell of the int16 range at
 *     every k <= 15.  (The integer centre (c << k) + ((1 << k) >> 1) of
 *     pcc_octree_decode_frames_lod's comment stays the centre in lattice
 *     units.)
 * v and o are not part of any blob: the caller carries the grid.
 *
 *   _keys_frames_f32 : pcc_morton_keys_frames for float32 rows d_xyz [n, 3] in
 *     the caller's unit, quantised by the rule in the same pass (12 B read,
 *     8 B written per row).  d_status (int32[2] in device memory, zeroed by
 *     the caller): d_status[0] |= 1 for a finite coordinate whose q is off the
 *     grid, |= 2 for a non-finite coordinate (NaN, +-Inf); the key of such a
 *     row is unspecified and the caller must not go on.  drop != 0: a row with
 *     a non-finite coordinate is DROPPED instead: its key is n_frames << 48,
 *     which sorts behind the keys of every frame (n_frames <= 65535 fits the
 *     batch index), bit 1 stays clear and d_status[1] counts such rows; after
 *     pcc_sort_pairs the kept rows are the first n - d_status[1] keys, and
 *     nothing behind them may be handed to pcc_unique_rows or a coder.  A
 *     finite coordinate off the grid is flagged under both settings.
 *     h_origin: 3 floats on the host.  voxel not positive and finite, or a
 *     non-finite origin: PCC_E_ARG.  No synchronisation.
 *   pcc_rows_index : which decoded row every input row of such a call became.
 *     d_perm = the permutation pcc_sort_pairs returned for the call's n keys,
 *     n_keep = the kept rows (n without drops), d_run_starts / n_unique what
 *     pcc_unique_rows returned for the first n_keep sorted keys,
 *     d_frame_offsets the frames' input rows (n_frames+1 entries, device, as
 *     for pcc_morton_keys_frames), d_first_run[f] (n_frames entries, device)
 *     the first run of frame f = the points of the frames in front of it.
 *     d_index[r] (int32 [n]) = the run of input row r counted from its frame's
 *     first run, i.e. its row in pcc_octree_decode_frames' result for that
 *     frame, or -1 for a dropped row.  One launch, a binary search among the
 *     run starts per row (at most 27 steps), no synchronisation.
 *   pcc_points_to_metric : int32 [n, 3] lattice points (lod 0) or cells of
 *     level of detail lod (0 .. 15) in device memory -> float32 [n, 3] by the
 *     rule backwards.  One launch, 12 B read and written per point, no
 *     synchronisation. */
int pcc_morton_keys_frames_f32(pcc_ctx* ctx, const float* d_xyz, int64_t n,
                               const int64_t* d_frame_offsets, int n_frames,
                               float voxel, const float* h_origin, int drop,
                               uint64_t* d_keys, int32_t* d_status);
int pcc_rows_index(pcc_ctx* ctx, const uint32_t* d_perm, int64_t n,
                   int64_t n_keep, const uint32_t* d_run_starts,
                   int64_t n_unique, const int64_t* d_frame_offsets,
                   const int64_t* d_first_run, int n_frames, int32_t* d_index);
int pcc_points_to_metric(pcc_ctx* ctx, const int32_t* d_points, int64_t n,
                         int lod, float voxel, const float* h_origin,
                         float* d_out);
/* inverse: keys -> (b,x,y,z) */
int pcc_keys_to_coords(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                       int32_t* d_coords);
/* replaces: the sortable value of shared/utils.py:131-132 / :160-161
 * (key = b*1e15 + x*1e10 + y*1e5 + z, int64) */
int pcc_linear_keys(pcc_ctx* ctx, const int32_t* d_coords, int64_t n,
                    int64_t* d_keys);
/* stable LSD radix sort of 64-bit keys (unsigned order; pass is_signed=1 for
 * int64 order) carrying the original row index.  d_keys is sorted in place,
 * d_perm[i] = original index of the i-th smallest key. */
int pcc_sort_pairs(pcc_ctx* ctx, uint64_t* d_keys, uint32_t* d_perm, int64_t n,
                   int is_signed);
/* replaces: utils.sort_tensor / utils.sort_points (shared/utils.py:116-165):
 * d_perm = argsort of the linear key. */
int pcc_sort_coords(pcc_ctx* ctx, const int32_t* d_coords, int64_t n,
                    uint32_t* d_perm);
/* dst[i,:] = src[perm[i],:], rows of row_bytes (multiple of 4) */
int pcc_gather_rows(pcc_ctx* ctx, const void* d_src, const uint32_t* d_perm,
                    int64_t n, int row_bytes, void* d_dst);
/* h_dup = 1 if two adjacent sorted keys are equal */
int pcc_check_unique(pcc_ctx* ctx, const uint64_t* d_sorted_keys, int64_t n,
                     int* h_dup);
/* per-batch row offsets of a key-sorted tensor: h_offsets[b] = first row with
 * batch >= b, for b in [0, n_batch]; (h_offsets[n_batch] == n) */
int pcc_batch_offsets(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                      int n_batch, int64_t* h_offsets);

/* ---- coordinate pyramid ------------------------------------------------ */

/* replaces: the output coordinate map of every stride-2 kernel-2 convolution
 * (g_a / h_a down stages, g_s.down_conv codec_parallel.py:302-303):
 * parents = unique(floor(c / 2ts) * 2ts).  child_shift = 3*log2(ts).
 * Outputs: d_pkeys (capacity n_cap >= n), d_nbr8 (capacity 8*n_cap) laid out
 * [8, M] with row pitch M = *h_n_out, d_parent_of[i] = parent row of input i.
 * Synchronises to return *h_n_out. */
int pcc_down_coords(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                    int child_shift, uint64_t* d_pkeys, int32_t* d_nbr8,
                    int64_t n_cap, int32_t* d_parent_of /* [n], nullable */,
                    int64_t* h_n_out);
/* The sizes of the pyramid above a sorted key set in one pass and one
 * synchronisation: h_counts[l] = number of distinct (key >> (child_shift +
 * 3 (l+1))), l = 0..levels-1, i.e. the *h_n_out of `levels` successive
 * pcc_down_coords calls; *h_dup (nullable) = 1 if two neighbouring keys are equal
 * (pcc_check_unique).  pcc_down_coords_known is pcc_down_coords with the parent
 * count m supplied, and does not synchronise. */
int pcc_level_counts(pcc_ctx* ctx, const uint64_t* d_sorted_keys, int64_t n,
                     int child_shift, int levels, int64_t* h_counts, int* h_dup);
int pcc_down_coords_known(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                          int child_shift, uint64_t* d_pkeys, int32_t* d_nbr8,
                          int64_t n_cap, int32_t* d_parent_of, int64_t m);
/* replaces: the generative transposed-convolution coordinate map (up stages
 * of h_s and g_s): children key = parent | o << (3*log2(ts/2)), row 8p+o. */
int pcc_up_coords(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                  int child_shift, uint64_t* d_ckeys);
/* the keys of the listed children only: d_ckeys[i] = key of row d_rows[i] = 8p + o of
 * pcc_up_coords' output (every d_rows[i] < 8n — the caller's contract, as for
 * pcc_gather_rows), without the 8n keys being written.  What the decoder keeps of
 * an up stage's candidates (codec_parallel.py:465-472: the pruned tensor's
 * coordinates). */
int pcc_up_coords_rows(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                       int child_shift, const uint32_t* d_rows, int64_t m,
                       uint64_t* d_ckeys);

/* ---- rule book (kernel map) and lookup --------------------------------- */

/* The same rule book WITHOUT hashing, derived from the parent level's rule
 * book: a child (parent p, octant o) has its neighbour at offset d in the child
 * o' of parent-neighbour p+D with, per axis, t = o+d, D = floor(t/2), o' = t&1.
 *  - up:   children are the 8 generative children of n_parents rows (child row
 *          8j+o).  If the parent level is a pruned subset of the level the
 *          rule book d_nbr_parent was built on, d_parent_rows[j] is its row
 *          there and d_remap maps rows of that level back to pruned rows (-1
 *          if dropped); pass both NULL when parent rows == rule-book rows.
 *  - down: children/parents linked by pcc_down_coords (d_parent_of, d_nbr8).
 *  - pcc_inverse_rows: remap[rows[j]] = j, -1 elsewhere (n entries; rows distinct,
 *    so with m == n every entry is written and nothing is preset). */
int pcc_derive_map_up(pcc_ctx* ctx, const int32_t* d_nbr_parent,
                      int64_t parent_pitch, const uint32_t* d_parent_rows,
                      const int32_t* d_remap, int64_t n_parents, int32_t* d_nbr);
int pcc_derive_map_down(pcc_ctx* ctx, const int32_t* d_nbr_parent,
                        int64_t n_parent, const int32_t* d_nbr8,
                        const int32_t* d_parent_of, const uint64_t* d_keys,
                        int64_t n, int child_shift, int32_t* d_nbr);
int pcc_inverse_rows(pcc_ctx* ctx, const uint32_t* d_rows, int64_t m, int64_t n,
                     int32_t* d_remap);

/* replaces: ME kernel-map generation for 3^3 stride-1 convolutions.
 * stride = tensor stride ts; d_nbr is [27, n].  d_keys = the rows of a coordinate
 * set: Morton-sorted, distinct (as pcc_sort_pairs / pcc_down_coords / pcc_up_coords
 * leave them); sets of <= 4096 rows are searched in LDS, larger ones hashed. */
int pcc_build_map(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int stride,
                  int32_t* d_nbr);
/* replaces: SparseTensor.features_at_coordinates (codec_pipeline.py:401,
 * codec_parallel.py:387) — exact-lattice lookup; d_rows[i] = row of query i in
 * the key set or -1. */
int pcc_lookup(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
               const uint64_t* d_qkeys, int64_t m, int32_t* d_rows);
/* dst[i,:] = rows[i] >= 0 ? src[rows[i],:] : 0 */
int pcc_gather_rows_or_zero(pcc_ctx* ctx, const float* d_src,
                            const int32_t* d_rows, int64_t m, int c,
                            float* d_dst);

/* ---- sparse network layers -------------------------------------------- */

/* replaces: MinkowskiConvolution forward (3^3 stride 1 with K=27 and a rule
 * book from pcc_build_map; 2^3 stride 2 with K=8 and the rule book from
 * pcc_down_coords).  On the matrix cores: cin = 4 or a multiple of 16 up to 128
 * with cout a multiple of 16 (pcc_conv_kernel_name); any (cin <= 128, cout <= 256)
 * on the scalar-fmaf path (same results). */
int pcc_sparse_conv(pcc_ctx* ctx, const float* d_in, int64_t n_in,
                    const int32_t* d_nbr, int k_vol, int64_t nbr_pitch,
                    int64_t n_out, const float* d_w, const float* d_bias,
                    int cin, int cout, int relu, float* d_out);
/* Diagnostic: name of the kernel pcc_sparse_conv (op 0), the siblings-first conv of
 * pcc_sparse_conv_head's generic form (op 1) or pcc_convT_gen (op 2) runs for a
 * shape with 16-byte aligned tensors: "k_gconv16" (32 -> 32 / 64; the name stands for
 * the family: op 0 launches of at most 2048 sixteen-row windows, 1024 for 32 -> 64, run
 * its no-compaction form k_gconv_rows16 — the name does not depend on the row count),
 * "k_gconv_gen"
 * (any widths that are multiples of 16: C_in <= 128, C_out <= 256), "k_gconv_first"
 * (4 -> multiples of 16), "k_convT16" (the up stage 32 -> 32), "k_convT_mfma" (other
 * multiples of 16 up to 128) — all on the
 * matrix cores — or the scalar-fmaf kernels ("k_gconv_scalar", "k_convT_scalar":
 * other shapes, PCC_FORCE_SCALAR=1).  Same results whichever runs. */
const char* pcc_conv_kernel_name(int op, int k_vol, int cin, int cout);
/* Layer weights, prepared once.  The (32,32) and (32,64) layers read their weights
 * as matrix-core operands from a copy in operand order (csrc/conv16.h).  A weight
 * tensor [k_vol][cin][cout] registered here — what load_model / model.to(device)
 * do once per layer (codec_pipeline.py:56-72) — is re-arranged now and found again
 * by its device pointer in every later pcc_sparse_conv* call on this ctx; for an
 * unregistered pointer the copy is made in front of each launch (same results).
 * Call again after the tensor's contents changed; pcc_conv_forget before its
 * memory is freed or reused.  Shapes without such a form: PCC_E_ARG. */
int pcc_conv_prepare(pcc_ctx* ctx, const float* d_w, int k_vol, int cin, int cout);
int pcc_conv_forget(pcc_ctx* ctx, const float* d_w);
/* the conv3 layer of a g_s stage (codec_parallel.py:469) with the 1x1 occupancy
 * head fused into its epilogue: d_head_out[n] = head_b[0] + sum_c fmaf(out[n][c],
 * head_w[c]) (c ascending) — bit-identical to pcc_linear(cout -> 1) applied to
 * d_out, without re-reading it.  Neighbours are visited SIBLINGS FIRST (the
 * arithmetic contract at the top of this file): first the pairs with
 * (input row >> 3) == (output row >> 3), k ascending, then the others, k
 * ascending.  On a generative level (input rows = output rows, in aligned blocks
 * of the 8 children of a parent — what g_s feeds it) that is "the row's own
 * parent first"; on any other input it is the same comparison of index values,
 * as deterministic, and what the oracle computes too — no check rejects it. */
int pcc_sparse_conv_head(pcc_ctx* ctx, const float* d_in, int64_t n_in,
                         const int32_t* d_nbr, int k_vol, int64_t nbr_pitch,
                         int64_t n_out, const float* d_w, const float* d_bias,
                         int cin, int cout, int relu, float* d_out,
                         const float* d_head_w, const float* d_head_b,
                         float* d_head_out);
/* building block of every compaction on the path (stride-2 parent dedup, top-k
 * pruning, radix-sort offsets, octree levels — the work torch.unique / ME's
 * coordinate manager do inside the reference's ME.SparseTensor and pruning
 * calls): exclusive prefix sum, d_out[i] = sum d_in[0..i), wrapping mod 2^32;
 * d_in and d_out may alias; d_total (device, nullable) receives the grand total.
 * Reduce-then-scan over 2048-element tiles. */
int pcc_exclusive_scan_u32(pcc_ctx* ctx, const uint32_t* d_in, uint32_t* d_out,
                           int64_t n, uint32_t* d_total);

/* The g_s stage form of the two above with the rule book formed on the fly.
 * The conv3 of a synthesis stage runs on the 8 generative children (row 8p+o) of
 * the n_parents rows of the level below; d_nbr_parent is THAT level's 27-offset
 * rule book ([27, parent_pitch]), and the child rule book (27 x 8 n_parents
 * int32, 352 MB for the bench frame) is never materialised: same values as
 * pcc_derive_map_up(parent book) followed by pcc_sparse_conv_head, bit for bit.
 * cin = cout = 32, K = 27 only (the shape of the model's g_s stages).
 * pcc_subset_map_up gives the rule book of the level that survives the top-k
 * pruning of those children (rows d_keep, ascending; d_remap from
 * pcc_inverse_rows over the 8 n_parents candidates), again from the parent
 * book: d_nbr is [27, n_keep]. */
int pcc_sparse_conv_head_up(pcc_ctx* ctx, const float* d_in, int64_t n_parents,
                            const int32_t* d_nbr_parent, int64_t parent_pitch,
                            const float* d_w, const float* d_bias, int relu,
                            float* d_out, const float* d_head_w,
                            const float* d_head_b, float* d_head_out);
int pcc_subset_map_up(pcc_ctx* ctx, const int32_t* d_nbr_parent,
                      int64_t parent_pitch, const uint32_t* d_keep,
                      const int32_t* d_remap, int64_t n_keep, int32_t* d_nbr);

/* rule book of a SUBSET of the output rows of a layer: d_nbr_out[k][j] =
 * d_nbr[k][d_rows[j]], or -1 where d_rows[j] < 0 ([k_vol, m], pitch m);
 * d_self (nullable) [m] = j where d_rows[j] >= 0, else -1.  With it a conv whose
 * output is only sampled afterwards (h_s followed by features_at_coordinates at
 * the latent's coordinates, codec_pipeline.py:401 / codec_parallel.py:387) is
 * evaluated at the sampled rows alone: same bits per row, a quarter of the rows;
 * pcc_gather_rows_or_zero(out, d_self) then zeroes the rows that were absent. */
int pcc_gather_map_columns(pcc_ctx* ctx, const int32_t* d_nbr, int k_vol,
                           int64_t pitch, const int32_t* d_rows, int64_t m,
                           int32_t* d_nbr_out, int32_t* d_self);

/* replaces: MinkowskiGenerativeConvolutionTranspose forward (kernel 2,
 * stride 2): out[8p+o] = W[o]^T in[p] + bias. */
int pcc_convT_gen(pcc_ctx* ctx, const float* d_in, int64_t n_in,
                  const float* d_w, const float* d_bias, int cin, int cout,
                  int relu, float* d_out);
/* 1x1 convolution (MinkowskiLinear / kernel-1 conv): occupancy and colour
 * heads of g_s. */
int pcc_linear(pcc_ctx* ctx, const float* d_in, int64_t n, const float* d_w,
               const float* d_bias, int cin, int cout, int relu, float* d_out);
/* pcc_convT_gen (cin = cout = 32) whose parent p is row d_rows[p] of d_in: the up
 * stage that follows a pruning, on the kept rows in place (same bits as
 * pcc_gather_rows followed by pcc_convT_gen). */
int pcc_convT_gen_gather(pcc_ctx* ctx, const float* d_in, const uint32_t* d_rows,
                         int64_t n_in, const float* d_w, const float* d_bias,
                         int relu, float* d_out);
/* pcc_linear (cin = 32, cout <= 8) applied to the rows d_rows[0..n) of d_in:
 * d_out[j] = linear(d_in[d_rows[j]]) — the colour head on the voxels kept by the
 * last pruning, without materialising their gathered feature rows (same bits as
 * pcc_gather_rows followed by pcc_linear). */
int pcc_linear_gather(pcc_ctx* ctx, const float* d_in, const uint32_t* d_rows,
                      int64_t n, const float* d_w, const float* d_bias, int cout,
                      int relu, float* d_out);

/* replaces: the per-frame top-k occupancy pruning inside model.g_s(y_hat,k=ks)
 * (codec_parallel.py:469): within each batch segment keep the k[b] rows with
 * the largest logit (ties: lower row first).  "Largest" is the order of the
 * logit's bit image (sign bit set: all bits complemented, else the sign bit
 * set; compared as uint32), which is the order of the values wherever they
 * have one and fixes the rest: -0.0 below +0.0, a positive NaN above +inf, a
 * negative NaN below -inf, NaNs among themselves by payload.  d_keep_rows receives the kept
 * row indices in ascending order; *h_n_keep their number.  h_offsets as from
 * pcc_batch_offsets (n_batch+1 entries), h_k n_batch entries.  The number of
 * kept rows is sum_f min(k[f], rows of frame f) by construction (no read-back);
 * h_n_keep may be NULL.  The call does not synchronise the stream for GOPs of
 * up to 8 frames. */
int pcc_topk_prune(pcc_ctx* ctx, const float* d_logits, int64_t n, int n_batch,
                   const int64_t* h_offsets, const int64_t* h_k,
                   uint32_t* d_keep_rows, int64_t* h_n_keep);
/* the same, and d_remap[r] (n entries, nullable) = position of row r in
 * d_keep_rows, or -1 for a row that is not kept: what pcc_inverse_rows makes of
 * d_keep_rows, written by the placement itself (the rule book of the pruned
 * level wants it, pcc_subset_map_up). */
int pcc_topk_prune_map(pcc_ctx* ctx, const float* d_logits, int64_t n, int n_batch,
                       const int64_t* h_offsets, const int64_t* h_k,
                       uint32_t* d_keep_rows, int64_t* h_n_keep, int32_t* d_remap);

/* ---- entropy-model device kernels ------------------------------------- */

/* replaces: EntropyBottleneck.compress symbol formation + dequantised z_hat
 * (codec_pipeline.py:303-306): sym[c*n+i] = rint(z[i][c] - med[c]) (int32,
 * channel-major), zhat[i][c] = sym + med[c]. */
int pcc_factorized_quant(pcc_ctx* ctx, const float* d_z, int64_t n, int c,
                         const float* d_med, int32_t* d_sym, float* d_zhat);
/* decoder side: zhat[i][c] = sym[c*n+i] + med[c] (codec_parallel.py:307-314) */
int pcc_factorized_dequant(pcc_ctx* ctx, const int32_t* d_sym, int64_t n,
                           int c, const float* d_med, float* d_zhat);
/* replaces: build_indexes + quantize of GaussianConditional.compress for Q
 * quality settings at once (codec_pipeline.py:407-430).
 *   params [n, 2c] = (scales_hat | means_hat) rows aligned with y rows
 *   scale  [q, c]  = scale_nn(q)+eps per quality
 *   table  [n_tab] ascending scale table (n_tab <= 64)
 *   sym,idx int32 [q, c, n] channel-major
 * sym = rint(y*s - mean*s), idx = (n_tab-1) - #{t in table[:-1] : max(sc*s,
 * table[0]) <= t}. */
int pcc_gaussian_quant(pcc_ctx* ctx, const float* d_y, const float* d_params,
                       int64_t n, int c, const float* d_scale, int q,
                       const float* d_table, int n_tab, int32_t* d_sym,
                       int32_t* d_idx);
/* element-wise forms behind the CompressAI-shaped tensor methods
 * gaussian_conditional.build_indexes(t) and EntropyModel.quantize(t, "symbols",
 * means) (any shape, n elements): idx = build_indexes(scales); sym = rint(x -
 * means) (means nullable). */
int pcc_build_indexes(pcc_ctx* ctx, const float* d_scales, int64_t n,
                      const float* d_table, int n_tab, int32_t* d_idx);
int pcc_quantize_symbols(pcc_ctx* ctx, const float* d_x, const float* d_means,
                         int64_t n, int32_t* d_sym);
/* compact form of the same: int16 symbols, uint8 indexes (3 instead of 8 bytes
 * per symbol across PCIe).  d_flag (int32[1]) is OR-ed with 1 if a symbol does
 * not fit int16; the caller then falls back to pcc_gaussian_quant. */
int pcc_gaussian_quant16(pcc_ctx* ctx, const float* d_y, const float* d_params,
                         int64_t n, int c, const float* d_scale, int q,
                         const float* d_table, int n_tab, int16_t* d_sym,
                         uint8_t* d_idx, int32_t* d_flag);
/* the same with int32 symbols and uint8 indexes, the element types the GPU
 * coder reads (pcc_rans_encode_dev): nothing overflows, nothing crosses PCIe */
int pcc_gaussian_quant_dev(pcc_ctx* ctx, const float* d_y, const float* d_params,
                           int64_t n, int c, const float* d_scale, int q,
                           const float* d_table, int n_tab, int32_t* d_sym,
                           uint8_t* d_idx);
int pcc_gaussian_indexes8(pcc_ctx* ctx, const float* d_params, int64_t n, int c,
                          const float* d_scale, const float* d_table, int n_tab,
                          uint8_t* d_idx);
/* decoder side (codec_parallel.py:394-409): indexes for one quality */
int pcc_gaussian_indexes(pcc_ctx* ctx, const float* d_params, int64_t n, int c,
                         const float* d_scale, const float* d_table, int n_tab,
                         int32_t* d_idx);
/* decoder side de-quantisation with offsets (codec_parallel.py:401-409):
 *   sigma = max(sc*s, bound); off = -(a / (b + sigma)), 0 where sym == 0
 *   yhat = sign(sym) * (|sym| + off) * (1/s) + mean */
int pcc_gaussian_dequant(pcc_ctx* ctx, const int32_t* d_sym,
                         const float* d_params, int64_t n, int c,
                         const float* d_scale, float bound, float off_a,
                         float off_b, float* d_yhat);

/* ---- host coders (no GPU needed) --------------------------------------- */

/* replaces: compressai.ans.RansEncoder.encode_with_indexes / RansDecoder.
 * decode_with_indexes (CompressAI 1.2.4, called from entropy_bottleneck /
 * gaussian_conditional .compress/.decompress: codec_pipeline.py:305-306,
 * 426-430; codec_parallel.py:307,400).
 *   cdfs   int32 [n_cdf, cdf_pitch] quantised CDFs (16-bit precision)
 *   sizes  int32 [n_cdf] cdf lengths, offsets int32 [n_cdf]
 * encode: returns bytes written into h_out (cap bytes) via *h_len. */
int pcc_rans_encode(const int32_t* h_sym, const int32_t* h_idx, int64_t n,
                    const int32_t* h_cdfs, int cdf_pitch, const int32_t* h_sizes,
                    const int32_t* h_offsets, int n_cdf, uint8_t* h_out,
                    int64_t cap, int64_t* h_len);
int pcc_rans_decode(const uint8_t* h_in, int64_t len, const int32_t* h_idx,
                    int64_t n, const int32_t* h_cdfs, int cdf_pitch,
                    const int32_t* h_sizes, const int32_t* h_offsets, int n_cdf,
                    int32_t* h_sym);
/* the same for n_streams independent streams coded on n_streams host threads
 * (the Q quality settings of gaussian_model_step_batched). */
int pcc_rans_encode_multi(const int32_t* h_sym, const int32_t* h_idx, int64_t n,
                          int n_streams, const int32_t* h_cdfs, int cdf_pitch,
                          const int32_t* h_sizes, const int32_t* h_offsets,
                          int n_cdf, uint8_t* h_out, int64_t cap_each,
                          int64_t* h_lens);

/* the same coders for the compact element widths (int16 symbols / uint8
 * indexes on encode, uint8 indexes on decode) */
int pcc_rans_encode_multi16(const int16_t* h_sym, const uint8_t* h_idx,
                            int64_t n, int n_streams, const int32_t* h_cdfs,
                            int cdf_pitch, const int32_t* h_sizes,
                            const int32_t* h_offsets, int n_cdf, uint8_t* h_out,
                            int64_t cap_each, int64_t* h_lens);
int pcc_rans_decode8(const uint8_t* h_in, int64_t len, const uint8_t* h_idx,
                     int64_t n, const int32_t* h_cdfs, int cdf_pitch,
                     const int32_t* h_sizes, const int32_t* h_offsets, int n_cdf,
                     int32_t* h_sym);

/* Seek points of a host-coded stream (round 4; pcc_codec_set_seek_points puts them into a container trailer).
 * _encode_seek: pcc_rans_encode, and for every h_seek_index[k] (ascending) inside (0, n) the coder's state and the
 * number of 32-bit words of the stream a decoder has consumed when symbol h_seek_index[k] is the next it decodes
 * (0 / 0 for an index outside (0, n)).  _decode_range: the symbols [i_lo, i_hi) from such a point (state_in, word_in;
 * i_lo == 0 with word_in == 0: the head of the stream), written to h_sym[i_lo .. i_hi); *h_state_out / *h_word_out =
 * where the decoder stands behind symbol i_hi - 1 — equal to the next point's values when stream and points agree.
 * The pieces between seek points are independent: any number of threads may decode them at once. */
int pcc_rans_encode_seek(const int32_t* h_sym, const int32_t* h_idx, int64_t n,
                         const int32_t* h_cdfs, int cdf_pitch, const int32_t* h_sizes,
                         const int32_t* h_offsets, int n_cdf, uint8_t* h_out, int64_t cap,
                         int64_t* h_len, const int64_t* h_seek_index, int n_seek,
                         uint64_t* h_seek_state, int64_t* h_seek_word);
int pcc_rans_decode_range(const uint8_t* h_in, int64_t len, const int32_t* h_idx, int64_t n,
                          const int32_t* h_cdfs, int cdf_pitch, const int32_t* h_sizes,
                          const int32_t* h_offsets, int n_cdf, int32_t* h_sym, int64_t i_lo,
                          int64_t i_hi, uint64_t state_in, int64_t word_in,
                          uint64_t* h_state_out, int64_t* h_word_out);

/* ---- range-ANS on the GPU: container version 1 (flagged extension) ------ */

/* Same call sites as the host coders above (codec_pipeline.py:305-306,426-430;
 * codec_parallel.py:307,398-400), different stream: the symbols of an array are
 * dealt to 64 rANS states per wave (csrc/rans_gpu.hip gives the layout), so the
 * coder runs on the device next to the kernels that make / consume the symbols
 * and the step has no serial host coder on its critical path.  The arithmetic of
 * a coding step (64-bit state, 16-bit CDFs, escape + 4-bit bypass) is that of
 * the reference's coder; a container whose y / z strings have this form carries
 * PCC_CONTAINER_V1 in the top byte of its first word (codec.hip) — the reference
 * decoder cannot read it, this library's decoders read both versions.
 *   tables : the CDF set in HBM (the arguments of pcc_rans_encode), made once
 *   d_sym  : int32 [n_streams, n]; d_idx uint8 [n_streams, n] table index per
 *            symbol, or NULL: index = position / idx_run (channel-major arrays).
 *            The coder's domain: symbol - offset of its table fits int32.
 *   d_out  : n_streams streams at d_out + s * cap_each (device, 4-byte aligned);
 *            pcc_rans_dev_bound(n) bytes always suffice; h_lens[s] = bytes
 * encode synchronises the stream once (the lengths); decode does not: it takes
 * the header fields pcc_rans_stream_info checked on the host copy of the stream
 * and ORs d_status (int32, device) with 1 / 2 / 4 if a chunk runs out of words /
 * an escape is malformed / a table index is not below n_cdf (the last row is
 * used instead) — test it after the next synchronisation.  encode clamps table
 * indexes the same way; with d_idx == NULL it refuses n > idx_run * n_cdf.
 * The coding loops read d_idx and the stream as aligned 32-bit words: the
 * device allocations behind d_in (decode) and d_idx (both) must be readable up
 * to the next multiple of 4 bytes beyond their last byte (any hipMalloc'd or
 * framework-allocated buffer is). */
typedef struct pcc_rans_dev pcc_rans_dev;
pcc_rans_dev* pcc_rans_dev_create(const int32_t* h_cdfs, int cdf_pitch,
                                  const int32_t* h_sizes, const int32_t* h_offsets,
                                  int n_cdf);
void pcc_rans_dev_destroy(pcc_rans_dev* tables);
int64_t pcc_rans_dev_bound(int64_t n);
int pcc_rans_encode_dev(pcc_ctx* ctx, const pcc_rans_dev* tables,
                        const int32_t* d_sym, const uint8_t* d_idx, int64_t idx_run,
                        int64_t n, int n_streams, uint8_t* d_out, int64_t cap_each,
                        int64_t* h_lens);
int pcc_rans_stream_info(const uint8_t* h_in, int64_t len, int64_t* h_n,
                         int64_t* h_steps, int64_t* h_chunks);
int pcc_rans_decode_dev(pcc_ctx* ctx, const pcc_rans_dev* tables, const uint8_t* d_in,
                        int64_t len, int64_t n, int64_t steps, int64_t n_chunks,
                        const uint8_t* d_idx, int64_t idx_run, int32_t* d_sym,
                        int32_t* d_status);

/* replaces: utils.gpcc_encode / gpcc_decode (shared/utils.py:169-240), i.e.
 * the tmc3 subprocess: lossless octree occupancy coding of one frame's latent
 * coordinates.  The blob is opaque to the container (length-prefixed slot) and
 * is NOT tmc3-compatible.
 * Device part: occupancy bytes of every octree level of one frame.
 *   d_keys    the frame's rows of a Morton-sorted key array (stride-ts tensor)
 *   key_shift 3*log2(ts): leaf = (key >> key_shift) & (2^(3*depth) - 1)
 *   depth     log2 of the side of the aligned root cube (host computes it from
 *             the first and last key: floor(msb(first^last)/3)+1, min 1)
 *   d_occ     uint8  [sum of level node counts], root level first
 *   h_level_n int64  [depth] nodes per level (root first)
 * cap = capacity of d_occ in bytes (n*depth is always enough). */
int pcc_octree_levels(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                      int key_shift, int depth, uint8_t* d_occ, int64_t cap,
                      int64_t* h_level_n);
/* host part: adaptive binary range-ANS of the occupancy bytes */
int pcc_octree_pack(const uint8_t* h_occ, const int64_t* h_level_n, int depth,
                    int64_t n_points, const int32_t* h_origin, uint8_t* h_out,
                    int64_t cap, int64_t* h_len);
/* parse blob header: n_points, depth, origin[3] */
int pcc_octree_peek(const uint8_t* h_in, int64_t len, int64_t* h_n_points,
                    int* h_depth, int32_t* h_origin);
/* decode blob to Morton-ordered points int32 [n_points,3] (origin added) */
int pcc_octree_unpack(const uint8_t* h_in, int64_t len, int32_t* h_points,
                      int64_t cap_points);
/* the same, and the node count of every octree level (h_level_n[0 .. depth-1],
 * 16 entries): level depth-1 = the leaves' parents, depth-2 their grandparents,
 * i.e. the sizes of the stride-2 coordinate sets above the decoded points. */
int pcc_octree_unpack_levels(const uint8_t* h_in, int64_t len, int32_t* h_points,
                             int64_t cap_points, int64_t* h_level_n);

/* one-call forms of the geometry slot: pcc_octree_encode = root cube from the
 * first / last key + pcc_octree_levels + pcc_octree_pack (utils.gpcc_encode,
 * shared/utils.py:169-207); pcc_octree_decode = pcc_octree_peek (+ unpack when
 * h_points is given) (utils.gpcc_decode, shared/utils.py:210-240, without the
 * `* 8`). */
int pcc_octree_encode(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                      int key_shift, uint8_t* h_out, int64_t cap, int64_t* h_len);
int pcc_octree_decode(const uint8_t* h_in, int64_t len, int32_t* h_points,
                      int64_t cap_points, int64_t* h_n_points);

/* Blob version 2 (round 4; csrc/octree2.hip gives the layout): the occupancy
 * ENTROPY coder on the GPU too — the adaptive binary model of version 1, coded
 * by 64 rANS states per wave over runs of consecutive nodes, every state's
 * model starting from the frame's average probabilities (header).  BASELINE.json
 * configs[2] (geometry-only coding of a ~100k-point LiDAR sweep) is this path.
 * pcc_octree_encode writes version 2 for sets above PCC_OCTREE_V2_MIN_LEAVES
 * leaves and version 1 (serial host coder: fewer bytes on small sets, and what
 * the latent-sized slots of the codec use) below; _version forces one
 * (0 = that rule).  Version-2 blobs are DEcoded by the GPU as well and have no
 * host decoder: pcc_octree_decode / pcc_octree_unpack* refuse them with
 * PCC_E_STREAM, the forms below take a context and read both versions.
 *   _decode_ctx : points to the host (h_points NULL: only the count)
 *   _decode_dev : points left in HBM (int32 [n,3], Morton order, origin added);
 *                 h_level_n (16 entries, nullable) = nodes per octree level */
/* Blob version 3 (round 4; csrc/octree_host.cpp gives the layout): the frame's
 * leaves in K = min(8, n / 4096) parts (at least 2), each a complete version-1
 * blob under the frame's root cube, cut between grandparent cells — coded by K
 * workgroups + K host coders and decoded by K host decoders side by side (the
 * serial decoder of a latent-sized slot stood at the head of every decode with
 * the GPU waiting for it).  pcc_octree_encode writes it for sets of
 * PCC_OCTREE_V3_MIN_LEAVES leaves and more, up to PCC_OCTREE_V2_MIN_LEAVES;
 * every host decoder above reads it (pcc_octree_unpack_levels: levels depth-1
 * and depth-2 are the frame's, the levels above count a node once per part). */
#define PCC_OCTREE_V2_MIN_LEAVES 65536
#define PCC_OCTREE_V3_MIN_LEAVES 8192
int pcc_octree_encode_version(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                              int key_shift, int version, uint8_t* h_out,
                              int64_t cap, int64_t* h_len);
int pcc_octree_blob_version(const uint8_t* h_in, int64_t len);
int pcc_octree_decode_ctx(pcc_ctx* ctx, const uint8_t* h_in, int64_t len,
                          int32_t* h_points, int64_t cap_points,
                          int64_t* h_n_points);
int pcc_octree_decode_dev(pcc_ctx* ctx, const uint8_t* h_in, int64_t len,
                          int32_t* d_points, int64_t cap_points,
                          int64_t* h_n_points, int64_t* h_level_n);

/* Geometry-only coding of a SEQUENCE of point sets (LiDAR sweeps): B frames
 * into B independent version-2 blobs in one call, and back.  Every blob is
 * byte-identical to what the one-frame call writes for that frame alone, so
 * _decode_ctx / _decode_dev read each of them.  The frames' chunks are coded
 * side by side: the number of launches does not grow with B, nor the number of
 * synchronisations (encode: 3 — end keys, level counts, blob lengths;
 * decode: 1).
 *   _encode_frames : d_keys = Morton keys of pcc_morton_keys with the frame
 *     index as batch index (0 .. n_frames-1), sorted (pcc_sort_pairs) and
 *     distinct after the key shift (PCC_E_DUP otherwise; unsorted keys or a
 *     frame index >= n_frames: PCC_E_ARG).  Blob f is
 *     h_out[h_offsets[f] .. h_offsets[f+1]) (h_offsets: n_frames+1 entries);
 *     a frame without keys gives the 24-byte empty blob.  More bytes than
 *     cap: PCC_E_NOMEM, nothing written.  Fewer than 2^27 leaves in all,
 *     1 <= n_frames <= 65535.
 *   _decode_frames : n_frames blobs of version 2 (another version: PCC_E_ARG
 *     naming the frame) -> their points int32 [n,3], origin added, Morton
 *     order inside a frame (as _decode_dev), concatenated in frame order;
 *     frame f's points are rows h_point_offsets[f] .. h_point_offsets[f+1]
 *     (n_frames+1 entries).  d_points (HBM) and / or h_points (host), both
 *     NULL = sizes only; more points than cap_points: PCC_E_NOMEM.  Every
 *     header is checked, and the sizes all of them announce summed, before
 *     anything is reserved; a corrupt blob is PCC_E_STREAM naming its frame.
 *     An h_points in pinned host memory (hipHostMalloc) receives the points
 *     straight from the device; any other array through the ctx's staging.
 * After an error the ctx stays usable.  Scratch per encoded frame is at least
 * one chunk (64 lanes x S >= 4 nodes): about 8 KB of device scratch even for a
 * one-point frame, so 65 535 tiny frames in one call take about 0.5 GB; a
 * frame's blob is staged at a bound in proportion to its nodes
 * (8 words per node + 384 B per chunk + header). */
int pcc_octree_encode_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                             int n_frames, int key_shift, uint8_t* h_out,
                             int64_t cap, int64_t* h_offsets);
int pcc_octree_decode_frames(pcc_ctx* ctx, const uint8_t* const* h_blobs,
                             const int64_t* h_lens, int n_frames,
                             int32_t* d_points, int32_t* h_points,
                             int64_t cap_points, int64_t* h_point_offsets);

/* Levels of detail of a version-2 blob: coarser cells from a PREFIX of its
 * bytes (csrc/octree2_blob.h parses and plans it on the host).  Nodes are
 * numbered breadth-first and dealt to lanes and chunks in that order, the
 * chunk table lies in front of the payload and every lane owns a contiguous
 * run of words, so the levels above a cut are a prefix of the blob; the root
 * cube is aligned to 2^depth in biased coordinates, so the nodes of a level
 * are global cells.  For n > 0 points, depth d, level sizes level_n[0..d-1],
 * S, chunk table words[nc], first payload byte off_payload and a level of
 * detail lod = k in 0 .. 15 (16 is excluded: 32768 is not a multiple of 2^16):
 *   cut level Lc = max(d - k, 0);
 *   cells m = n (k = 0), level_n[Lc] (0 < k < d), 1 (k >= d);
 *   nodes needed N' = level_n[0] + .. + level_n[Lc-1];
 *   result: int32 [m,3] CELL INDICES p >> k (arithmetic shift) of the frame's
 *     points, distinct, in Morton order; corner of a cell c << k, centre
 *     (c << k) + ((1 << k) >> 1).  k = 0 is pcc_octree_decode_frames' result;
 *   shortest prefix: k = 0 the whole blob; N' = 0: off_payload bytes (header,
 *     level table, S, nc, p0 and the WHOLE chunk table are always needed);
 *     otherwise with lanes = ceil(N' / S), c* = (lanes-1) / 64,
 *     l* = (lanes-1) % 64:
 *       off_payload + 2 (words[0] + .. + words[c*-1])
 *                   + 2 (192 + len[0] + .. + len[l*]),
 *     len being chunk c*'s own length table.  Any longer prefix, the whole
 *     blob included, decodes to the same result;
 *   an empty blob (24 bytes, n = 0) has 0 cells and needs its 24 bytes at
 *     every k.
 *   _lod_info : host only, no ctx: h_bytes / h_cells (nullable) receive what
 *     level `lod` needs and gives.  h_in may be the blob or any prefix long
 *     enough to answer (it must reach the last needed chunk's length table);
 *     a shorter one, or a damaged header: PCC_E_STREAM; another blob version
 *     or lod outside 0 .. 15: PCC_E_ARG.  A version-4 blob (below) answers
 *     with the same formulas over its own offsets; its lod 0 is the whole
 *     blob and wants the whole blob.
 *   _decode_frames_lod : pcc_octree_decode_frames at a level of detail: blobs
 *     or prefixes of them, every frame at the same lod (outside 0 .. 15:
 *     PCC_E_ARG); pcc_octree_decode_frames is its lod = 0 call.  A prefix even
 *     two bytes short of its level is PCC_E_STREAM ("truncated") naming the
 *     frame, refused on the host before anything is reserved or launched.
 *     Only the needed part of every blob is uploaded and only the needed
 *     chunks are decoded; nodes, links and output are sized from N' and m,
 *     which the stream verifies (level boundaries above the cut, the children
 *     of the first N' nodes).  What a prefix cannot verify (the level sizes
 *     below the cut, n) stays bounded by the header checks alone.  Same
 *     launches per call as _decode_frames, one synchronisation.
 * The sender's side of the same cells is pcc_octree_encode_frames with
 * key_shift = 3 lod over keys that are distinct per cell. */
int pcc_octree_lod_info(const uint8_t* h_in, int64_t len, int lod,
                        int64_t* h_bytes, int64_t* h_cells);
int pcc_octree_decode_frames_lod(pcc_ctx* ctx, const uint8_t* const* h_blobs,
                                 const int64_t* h_lens, int n_frames, int lod,
                                 int32_t* d_points, int32_t* h_points,
                                 int64_t cap_points, int64_t* h_point_offsets);

/* Inter-frame geometry coding: octree blob version 4, a PREDICTED frame
 * (csrc/octree4.hip, csrc/octree4_blob.h).  Version 4 is version 2 with three
 * changes; the tree, the root cube, the breadth-first numbering, the dealing
 * of nodes in runs of S to the 64 lanes of a chunk, the per-lane rANS states,
 * word runs, length table, chunk table, the p0 formula, the adaptation and the
 * implied eighth bit are version 2's.
 *   'O' 4 depth (W-1) | u32 n | i32 origin[3] | u32 payload_len |
 *   u32 level_n[depth] | u32 S | u32 n_chunks | u32 ref_n | u64 ref_sum |
 *   u16 p0[324] | u32 words[n_chunks] | chunks
 * Reference byte: R, the reference, is a set of distinct lattice points in the
 *   units of the frame.  Bit j of a node's reference byte is 1 exactly when R
 *   holds a point inside the cube of the node's child octant j (octants as in
 *   version 2: x is the top bit).  Purely geometric: R's own root cube and
 *   depth do not matter, and a node out of R's reach has reference byte 0.
 *   With key_shift = 3 k (the sender's side of a level of detail) frame and
 *   reference are both the cells at lod k.
 * Context of decision j of a node: r * 108 + (version 2's context), r = 0
 *   where the node's reference byte is 0, 1 where it is not and its bit j is
 *   0, 2 where its bit j is 1.  p0[324] from the frame's counts per context
 *   with version 2's formula; a context never seen gets that of (0, 0).
 * ref_n = |R|; ref_sum = the sum over R's points of
 *   ((x & 0xFFFF) << 32) | ((y & 0xFFFF) << 16) | (z & 0xFFFF) mod 2^64, the
 *   coordinates as a decoder returns them.  A decoder that holds another
 *   reference refuses the blob.
 * S: the encoder deals runs of at most 256 nodes (version 2: 512), because a
 *   level's launch of the decoder lasts up to 8 S dependent steps of a wave;
 *   a decoder takes S from the header, any multiple of 4 in 4 .. 512.
 * A frame without points stays the 24-byte version-2 blob; a frame whose
 *   reference has no points is written as version 2.
 * Levels of detail: the levels above a cut are a prefix of the bytes, as in
 *   version 2: cut level, cells m, nodes needed N' and the shortest prefix are
 *   the formulas above with off_payload = 24 + 4 depth + 20 + 648 + 4 nc
 *   (pcc_octree_lod_info answers for both versions).  A node above the cut at
 *   lod k has child cubes of side >= 2^k; the root corner is a multiple of
 *   2^depth in biased coordinates and 32768 a multiple of 2^k, so every such
 *   cube is a union of whole lod-k cells and "R has a point in the cube" is
 *   "R has a cell in the cube": the prefix decodes against the reference's
 *   CELLS at lod k alone (a cell c is searched as the point c << k), to the
 *   cells p >> k of the frame in Morton order.  k >= depth: nothing is
 *   decoded, the one cell is origin >> k.  What a cut cannot verify: ref_n
 *   and ref_sum describe full-resolution points, which a decoder that holds
 *   cells cannot form; at lod > 0 they are not compared.  A wrong reference at
 *   a cut is PCC_E_STREAM where the counts do not add up (a lane's words, an
 *   empty node, the children of a level) and otherwise m rows of wrong cells;
 *   it is never a store outside an array: every bound comes from the header's
 *   checks, the prefix's length and the rows at hand.
 *   _encode_frames_inter : pcc_octree_encode_frames whose frames are coded
 *     against the frame in front of them in the call.  intra_period = G >= 1:
 *     the coded frames g with g % G == 0 are version 2; 0: only the first
 *     frame of the keys is.  ref_first = 1: frame 0 of the keys is only the
 *     reference of frame 1: it gets no blob (h_offsets[1] == h_offsets[0]) and
 *     does not count in g.  Lossless coding makes the original the decoded
 *     frame, so all frames encode side by side: the intra frames in one batch,
 *     the predicted ones in another with one search kernel in front.
 *   _decode_frames_ref : any mix of versions 2 and 4.  The reference of a
 *     version-4 blob is the frame decoded before it in the call, for blob 0
 *     d_ref_points: int32 [n_ref,3], distinct, in Morton order, as a decode
 *     returns them.  A version-4 blob 0 without a reference, or a reference
 *     other than the one a blob was coded against (ref_n on the host, ref_sum
 *     and the order of d_ref_points on the device, read with the call's last
 *     synchronisation): PCC_E_ARG naming the frame.  A predicted frame decodes
 *     level by level, every wait a kernel boundary, launch sizes from the
 *     header alone; a damaged blob is PCC_E_STREAM naming the frame, and no
 *     access leaves what the header checks sized.  Outputs as
 *     pcc_octree_decode_frames'.
 *   _inter_info : host only, versions 2 and 4: version, points, predicted
 *     (0 / 1) and ref_points (0 for version 2), each nullable; the blob must
 *     be whole, or for version 4 exactly the prefix that pcc_octree_lod_info
 *     names for some lod.
 * The window (history = K, 1 <= K <= 8): R may be the union of several frames.
 *   Every frame of a call has a position: the leading reference frames first,
 *   then the coded frames; reference frames get no blob.  A predicted frame t
 *   has a window of W_t frames, 1 <= W_t <= K: the W_t frames directly in
 *   front of it.  The window never reaches back past the latest intra frame
 *   (that frame itself may be in it) and never past a frame without points
 *   (the frame behind an empty frame is intra, as before); so among the
 *   reference frames only the trailing run of non-empty ones exists, and at
 *   most K of them count.  Which frames are intra is decided as before
 *   (intra_period, frame 0 without a reference, the empty-frame rule).  R is
 *   the set of distinct lattice points of the window's frames (with key_shift
 *   = 3 k: cells), ref_n = |R|, ref_sum the sum over R.  Byte 3 of the head
 *   holds W_t - 1, so K = 1 writes the bytes of before and a decoder reads
 *   from the blob how many decoded frames to merge.  The header's parser
 *   accepts any byte 3; the decode entries refuse a window above 8
 *   (PCC_E_STREAM naming the frame).
 *   _encode_frames_inter_hist : _encode_frames_inter with the first
 *     n_ref_frames (0 .. history) frames of the keys as references and
 *     windows of up to `history` frames.  _encode_frames_inter is its
 *     (ref_first, 1) form; a call in which no window exceeds one frame queues
 *     what that entry queues.  The unions of all larger windows are formed on
 *     the device in one merge (pcc_merge_keys' kernels) with ONE host
 *     synchronisation more per call, for their sizes.  The keys of a window's
 *     frames must total fewer than 2^27: PCC_E_ARG naming the frame.
 *   _decode_frames_refs : _decode_frames_ref with n_refs (0 .. 8) references,
 *     oldest first, d_ref_points[r] as d_ref_points there, n_ref[r] >= 0.  The
 *     call keeps the keys of the last decoded frames, merges the W a blob asks
 *     for and takes ref_sum over the union.  For W > 1 the host can only bound
 *     ref_n (the largest of the window's frames <= ref_n <= their sum, checked
 *     before anything is sized); equality is checked on the device with
 *     ref_sum.  A window that reaches in front of the first frame at hand:
 *     PCC_E_ARG "needs W frames in front of it, n are here".
 *     _decode_frames_ref is its form with at most one reference.
 *   _decode_frames_refs_lod : _decode_frames_refs at a level of detail (lod
 *     outside 0 .. 15: PCC_E_ARG; 0 is _decode_frames_refs itself, launch for
 *     launch).  lod > 0: blobs of versions 2 and 4 or prefixes of them, and
 *     d_ref_cells[r] are CELLS at that lod: int32 [n_ref,3], each in
 *     [-(32768 >> lod), (32768 >> lod) - 1], distinct, in Morton order, as
 *     this call or _decode_frames_lod returns them (anything else: PCC_E_ARG
 *     naming the frame).  The result is every frame's cells; a version-2 blob
 *     of the call goes through _decode_frames_lod.  Levels 0 .. Lc-1 alone are
 *     decoded, arrays are sized from N' and m, only the prefix is uploaded and
 *     the decoder reads no word behind it; the children of level Lc-1 must
 *     number level_n[Lc] (PCC_E_STREAM).  A prefix even two bytes short is
 *     PCC_E_STREAM ("truncated") naming the frame, before anything is
 *     reserved or launched.  ref_n and ref_sum are not compared (above); a
 *     window's union is formed from the cells' keys and its size stays on the
 *     device.
 * Intra or a window, chosen per frame (_encode_frames_inter_best): positions,
 *   reference frames, the scheduled intra frames (intra_period, frame 0
 *   without a reference) and the empty-frame rule are those of history = K.
 *   For a coded frame t with points that is not a scheduled intra frame (nor
 *   behind a frame without points), Wmax_t is the window history = K gives it:
 *   up to K frames directly in front, not past a scheduled intra frame (which
 *   may be in it), not past a frame without points.  Its candidates are the
 *   version-2 blob of the frame and, for every W in 1 .. Wmax_t, the version-4
 *   blob against the union of the W frames in front of it, byte 3 = W - 1.
 *   The frame gets the SHORTEST candidate; of equal lengths version 2 wins,
 *   then the smaller W.  A version-2 blob written by choice does not cut the
 *   windows of the frames behind it: only scheduled intra frames and frames
 *   without points do.  Every blob written is byte for byte the blob that
 *   _encode_frames / _encode_frames_inter_hist write for that frame with that
 *   version and window, and the decode entries take such sequences as they
 *   are: a blob says its version and its window itself, and a decoder merges
 *   the W positions in front of a blob whatever their versions.
 *   Random access: the random-access points of such a sequence are its
 *   SCHEDULED intra frames.  A version-2 blob chosen for its length decodes
 *   alone, but a frame behind it may reach past it, so a decoder that starts
 *   there may lack frames a later blob needs.
 *   _encode_frames_inter_best : the arguments of _encode_frames_inter_hist;
 *     history is the largest window tried.  Lossless coding makes the original
 *     the decoded frame, so the choice for one frame changes nothing for any
 *     other, and all candidates of all frames are coded side by side: ONE
 *     version-2 batch over the coded frames with points, ONE version-4 batch
 *     over every (frame, W) candidate in which the occupancy levels of a frame
 *     are built once and shared by its candidates (each has its own reference
 *     bytes, counts, probabilities and lane coder run).  The unions W = 2 ..
 *     Wmax of a frame are nested, U_W = U_(W-1) + frame t - W, and are formed
 *     in one pass for all frames and all W (pcc_merge_keys_nested's kernels).
 *     Host synchronisations are those of _encode_frames_inter_hist: the frame
 *     bounds, the union sizes, level counts and lengths of each batch.  All
 *     candidates' lengths are then on the host; only the winners are copied
 *     out of the pinned staging.  Limits: fewer than 2^27 keys in a window,
 *     fewer than 2^31 in the unions of a call (PCC_E_ARG naming the frame).
 *     The unions take one block of device memory, 8 bytes per key of the sum
 *     over frames and W >= 2 of the keys of the W frames (the bound of the sum
 *     of |U_W|); a call whose block does not fit returns PCC_E_NOMEM saying
 *     so before any candidate is launched.
 *   pcc_merge_keys_nested : n_lists (1 .. 8) lists as pcc_merge_keys takes
 *     them, NEWEST FIRST: union W, W = 1 .. n_lists, is the union of lists 0 ..
 *     W - 1.  All of them in one pass: the keep flags (a key is kept where no
 *     list in front of its own holds an equal one) and their scan are the
 *     merge's, and the scatter places a kept key of list i into every union
 *     W > i at the kept keys below it in lists 0 .. W - 1 — one search per
 *     list and key where a merge per union takes W.  Union W is written at
 *     d_out + sum over V < W of (h_n[0] + .. + h_n[V - 1]), with room for the
 *     keys of its lists; cap >= the sum of those rooms (PCC_E_NOMEM).
 *     h_counts[W - 1] = |union W| (one synchronisation).  As a set of compared
 *     keys union W is pcc_merge_keys of lists 0 .. W - 1; of equal keys the
 *     newest list's is kept.
 *   pcc_merge_keys : the union of 1 .. 8 lists of keys on the device, each
 *     strictly increasing under (key & (2^48 - 1)) >> key_shift (bits from 48
 *     up, the frame index of a call's keys, are carried along and not
 *     compared) -> d_out [cap >= the lists' keys in all], strictly increasing
 *     under the same comparison; of equal keys the one of the first list that
 *     holds it is kept.  d_lists is a host array of device pointers.  A merge,
 *     not a sort: one thread per element, binary searches in the other lists,
 *     one scan of the keep flags, a scatter to computed places — no atomics,
 *     the same output on every run.  *h_count = the union's size (one
 *     synchronisation).
 * pcc_octree_decode_frames, _decode_frames_lod, _blob_version and the one-blob
 * entries go on refusing version 4. */
int pcc_octree_encode_frames_inter(pcc_ctx* ctx, const uint64_t* d_keys,
                                   int64_t n, int n_frames, int key_shift,
                                   int intra_period, int ref_first,
                                   uint8_t* h_out, int64_t cap,
                                   int64_t* h_offsets);
int pcc_octree_decode_frames_ref(pcc_ctx* ctx, const uint8_t* const* h_blobs,
                                 const int64_t* h_lens, int n_frames,
                                 const int32_t* d_ref_points, int64_t n_ref,
                                 int32_t* d_points, int32_t* h_points,
                                 int64_t cap_points, int64_t* h_point_offsets);
int pcc_octree_inter_info(const uint8_t* h_in, int64_t len, int* version,
                          int64_t* points, int* predicted, int64_t* ref_points);
int pcc_octree_encode_frames_inter_hist(pcc_ctx* ctx, const uint64_t* d_keys,
                                        int64_t n, int n_frames, int key_shift,
                                        int intra_period, int n_ref_frames,
                                        int history, uint8_t* h_out,
                                        int64_t cap, int64_t* h_offsets);
int pcc_octree_decode_frames_refs(pcc_ctx* ctx, const uint8_t* const* h_blobs,
                                  const int64_t* h_lens, int n_frames,
                                  const int32_t* const* d_ref_points,
                                  const int64_t* n_ref, int n_refs,
                                  int32_t* d_points, int32_t* h_points,
                                  int64_t cap_points,
                                  int64_t* h_point_offsets);
int pcc_octree_decode_frames_refs_lod(pcc_ctx* ctx,
                                      const uint8_t* const* h_blobs,
                                      const int64_t* h_lens, int n_frames,
                                      const int32_t* const* d_ref_cells,
                                      const int64_t* n_ref, int n_refs,
                                      int lod, int32_t* d_points,
                                      int32_t* h_points, int64_t cap_points,
                                      int64_t* h_point_offsets);
int pcc_merge_keys(pcc_ctx* ctx, const uint64_t* const* d_lists,
                   const int64_t* h_n, int n_lists, int key_shift,
                   uint64_t* d_out, int64_t cap, int64_t* h_count);
int pcc_octree_encode_frames_inter_best(pcc_ctx* ctx, const uint64_t* d_keys,
                                        int64_t n, int n_frames, int key_shift,
                                        int intra_period, int n_ref_frames,
                                        int history, uint8_t* h_out,
                                        int64_t cap, int64_t* h_offsets);
int pcc_merge_keys_nested(pcc_ctx* ctx, const uint64_t* const* d_lists,
                          const int64_t* h_n, int n_lists, int key_shift,
                          uint64_t* d_out, int64_t cap, int64_t* h_counts);

/* Lossless per-point attributes of such a sequence (near-lossless ones with a
 * bounded error: pcc_attr_encode_frames_nl below) (csrc/attr.hip: attribute
 * blob version 1, one per frame, its layout in that file's header): uint8 or
 * uint16 values, 1 <= c <= 4 channels, in the Morton order of the frame's
 * decoded points.  The blob depends on the geometry only through the point
 * count n.  Encode: one launch each of merge, counting pass, coder and packing
 * for all frames, one synchronisation (blob lengths); decode: one launch, one
 * synchronisation.
 *   _encode_frames : the rows of the call's pcc_octree_encode_frames before
 *     duplicates were dropped.  h_rows (n_frames+1 entries, h_rows[0] = 0):
 *     frame f is rows h_rows[f] .. h_rows[f+1] of the call's keys;
 *     d_values + h_value_offsets[f] holds its values as rows [rows_f, c_f] of
 *     h_format[f] = bytes per value (1 | 2) | c_f << 8, little-endian.
 *     d_perm = the permutation pcc_sort_pairs returned for those keys (frame
 *     index as batch index), d_run_starts = pcc_unique_rows' first sorted row
 *     of every run of equal keys (n_unique entries), h_points[f] = frame f's
 *     points after the merge (its geometry blob's n; summed: n_unique).
 *     Duplicates keep per channel the rounded mean (sum + cnt / 2) / cnt.
 *     Blob f is h_out[h_offsets[f] .. h_offsets[f+1]); a frame without points
 *     gives the 12-byte empty blob, which still names its dtype and c.  More
 *     bytes than cap: PCC_E_NOMEM, nothing written.  Fewer than 2^27 rows in
 *     all, 1 <= n_frames <= 65535; a bad format or counts that do not add up:
 *     PCC_E_ARG naming the frame.
 *   _decode_frames : n_frames attribute blobs -> their values: frame f's
 *     [n_f, c_f] values of h_format[f] (nullable) start at byte
 *     h_out_offsets[f] (n_frames+1 entries, 16-aligned; the last = bytes
 *     needed) of d_out (HBM) and / or h_out (host); both NULL = sizes only
 *     (host parse, nothing launched); more than cap_bytes: PCC_E_NOMEM.
 *     h_points (nullable): every frame's geometry point count (from
 *     h_point_offsets of pcc_octree_decode_frames); a blob that announces
 *     another count is PCC_E_STREAM naming the frame.  Every header is parsed
 *     and checked on the host (csrc/attr_blob.h) before anything is reserved
 *     or launched, and what is reserved follows the blobs' lengths; a corrupt
 *     payload is PCC_E_STREAM naming its frame.  An h_out in pinned host
 *     memory receives the values straight from the device.
 * After an error the ctx stays usable.  Device scratch per encoded frame is at
 * least one chunk: 64 lanes x S c 16 bpv records and as many words (at most
 * 2 MB per chunk). */
int pcc_attr_encode_frames(pcc_ctx* ctx, const void* d_values,
                           const int64_t* h_value_offsets,
                           const int32_t* h_format, const int64_t* h_rows,
                           const int64_t* h_points, int n_frames,
                           const uint32_t* d_perm,
                           const uint32_t* d_run_starts, int64_t n_unique,
                           uint8_t* h_out, int64_t cap, int64_t* h_offsets);
int pcc_attr_decode_frames(pcc_ctx* ctx, const uint8_t* const* h_blobs,
                           const int64_t* h_lens, int n_frames,
                           const int64_t* h_points, uint8_t* d_out,
                           uint8_t* h_out, int64_t cap_bytes,
                           int64_t* h_out_offsets, int32_t* h_format);

/* Attributes at every level of detail: attribute blob version 2 (its layout
 * and rule in csrc/attr_blob.h's header).  Lossless like version 1, chosen by
 * the sender; the values a decoder needs at level of detail k are a prefix of
 * the blob's bytes, and the value of a cell is the value of its Morton-first
 * point (a sample of the cell; the sender's side lod codes the cell's mean).
 *   for n > 0 values and lod k in 0 .. 15:
 *   values m = cells[k] of the header (cells[0] = n), which a decoder checks
 *     against the cell count of the frame's geometry at the same lod;
 *   shortest prefix: k = 0 the whole blob; otherwise lanes = ceil(m / S),
 *     c* = (lanes-1) / 64, l* = (lanes-1) % 64:
 *       off_payload + 2 (words[0] + .. + words[c*-1])
 *                   + 2 (192 + len[0] + .. + len[l*]),
 *     len being chunk c*'s own length table; header, p0 and the WHOLE chunk
 *     table are always needed.  Any longer prefix decodes to the same result;
 *   an empty blob (12 bytes, n = 0) has 0 values and needs its 12 bytes.
 *   _lod_info : host only, no ctx: h_bytes / h_values (nullable) receive what
 *     level `lod` needs and gives.  h_in may be the blob or any prefix that
 *     reaches the last needed chunk's length table; a shorter one, or a damaged
 *     header: PCC_E_STREAM; another blob version or lod outside 0 .. 15:
 *     PCC_E_ARG.
 *   _encode_frames_v2 : pcc_attr_encode_frames writing version 2.  Beside its
 *     arguments: d_keys, the call's n_unique distinct sorted keys in HBM (what
 *     pcc_octree_encode_frames took, frame after frame) and their key_shift
 *     (3 lod on the sender's side of a lod, else 0; the blob records that lod
 *     and decodes at a further level j with lod + j <= 15).  Launches: merge, size,
 *     scan and residuals of the introduction order, counting pass, coder,
 *     packing (7); one synchronisation.
 *   _decode_frames_lod : version-2 blobs or prefixes of them, every frame at
 *     the same lod (outside 0 .. 15: PCC_E_ARG), as pcc_attr_decode_frames
 *     returns its values: row j of frame f is the value of the j-th cell.
 *     d_cells: the int32 [*, 3] cells of all frames in HBM as
 *     pcc_octree_decode_frames_lod left them at the same lod (they are not
 *     uploaded again), frame f's rows h_cell_offsets[f] .. h_cell_offsets[f+1]
 *     (n_frames+1 entries, its h_point_offsets).  A frame whose cell count
 *     differs from the blob's cells[lod] is PCC_E_STREAM naming the frame; so
 *     is a prefix even two bytes short of its level ("truncated"), both on the
 *     host before anything is reserved or launched.  d_out and h_out both
 *     NULL = sizes only (d_cells and h_cell_offsets may then be NULL).  Only
 *     the level's bytes are uploaded and only its chunks decoded; the lane the
 *     level cuts short stops there.  Every index of the reconstruction is
 *     checked against the frame's value count: a corrupt stream is
 *     PCC_E_STREAM naming its frame.  Launches: size, scan, place, coder,
 *     walk (5); one synchronisation.  After an error the ctx stays usable. */
int pcc_attr_lod_info(const uint8_t* h_in, int64_t len, int lod,
                      int64_t* h_bytes, int64_t* h_values);
int pcc_attr_encode_frames_v2(pcc_ctx* ctx, const void* d_values,
                              const int64_t* h_value_offsets,
                              const int32_t* h_format, const int64_t* h_rows,
                              const int64_t* h_points, int n_frames,
                              const uint32_t* d_perm,
                              const uint32_t* d_run_starts, int64_t n_unique,
                              const uint64_t* d_keys, int key_shift,
                              uint8_t* h_out, int64_t cap, int64_t* h_offsets);
/* pcc_attr_encode_frames (version 1) / _v2 (version 2) for a call that dropped
 * rows (pcc_morton_keys_frames_f32 with drop): h_rows still counts every input
 * row, dropped ones included, since d_perm and the values do; n_kept is the
 * number of sorted keys that belong to kept rows.  The merge closes its last
 * run there, so no dropped row reaches a value, and a frame may have input
 * rows and no point.  d_keys / key_shift are read by version 2 only. */
int pcc_attr_encode_frames_kept(pcc_ctx* ctx, int version, const void* d_values,
                                const int64_t* h_value_offsets,
                                const int32_t* h_format, const int64_t* h_rows,
                                const int64_t* h_points, int n_frames,
                                const uint32_t* d_perm,
                                const uint32_t* d_run_starts, int64_t n_unique,
                                int64_t n_kept, const uint64_t* d_keys,
                                int key_shift, uint8_t* h_out, int64_t cap,
                                int64_t* h_offsets);
int pcc_attr_decode_frames_lod(pcc_ctx* ctx, const uint8_t* const* h_blobs,
                               const int64_t* h_lens, int n_frames, int lod,
                               const int32_t* d_cells,
                               const int64_t* h_cell_offsets, uint8_t* d_out,
                               uint8_t* h_out, int64_t cap_bytes,
                               int64_t* h_out_offsets, int32_t* h_format);

/* Near-lossless attributes with a bounded error: attribute blob versions 4
 * (unscalable, version 1's order and layout) and 7 (scalable, version 2's
 * introduction order, cells[16], sender's lod and prefix rule).  No decoded
 * value is off by more than e = max_error from what the lossless coder would
 * return for the same call (the merged value v: the rounded mean of duplicate
 * points, or of a cell on the sender's side of a lod).
 *
 * The rule, one quantiser for both kinds.  bpv = bytes per value (1 | 2),
 * mask = 2^(8 bpv) - 1, e an integer with 1 <= e < 2^(8 bpv - 1), step
 * q = 2 e + 1.  Inside the prediction loop reconstructions v^ are UNCLAMPED
 * signed integers; they are clamped to [0, mask] only when written out.
 *   residual        d = v - p                      (no wrap)
 *   index           j = sgn(d) floor((|d| + e) / q)
 *   reconstruction  v^ = p + j q                    so |v - v^| <= e
 *   output          clamp(v^, 0, mask)              (moves towards v: the bound
 *                                                   holds)
 * |j| <= (mask + 2 e) / q < 2^(8 bpv - 1): j takes the place of the lossless
 * kinds' residual in their binarisation (zero flag, sign, Exp-Golomb prefix and
 * suffix, kmax = 8 bpv - 1), contexts (channel, bucket of |j| of the channel's
 * previous point in the lane's run, edges 2 / 5 / 12 / 30, position) and model.
 *   version 4: a lane codes its run of S points in Morton order; p = 0 for the
 *     run's first point, v^[s-1] for the second, floor((v^[s-1] + v^[s-2] + 1)
 *     / 2) after that (an arithmetic shift: v^ may be negative or above mask).
 *   version 7: p = v^[first(i)], point 0 predicted from 0, so v^_i = q times
 *     the sum of j along the chain i -> first(i) -> .. -> 0 (order-free).  Level
 *     of detail k holds the first cells[k] indices, a prefix of the bytes by
 *     version 2's lane-granular rule; the value of a cell is the reconstruction
 *     of its Morton-first point.
 * Layout: version 1's / version 2's with a u32 max_error directly behind
 * payload_len (counted in it, everything behind it 4 bytes later); n = 0 gives
 * the 12-byte head alone, which records no e.  The version bytes 1, 2, 4, 7
 * differ pairwise in two bits.
 *   _encode_frames_nl : pcc_attr_encode_frames_kept with max_error.  version
 *     1 | 2 chooses the unscalable / scalable kind; n_kept = -1: the call
 *     dropped no rows (pcc_attr_encode_frames / _v2); max_error = 0: the
 *     lossless blob of that version, byte for byte; max_error = e > 0: version
 *     4 / 7.  An e of 2^(8 bpv - 1) or more for a frame's bpv: PCC_E_ARG naming
 *     the frame.  One launch more than the lossless encoder of the version (4:
 *     the loop of every lane run; 7: the walk of every point's chain).
 *   _info : host only, no ctx: what the head of an attribute blob of any of
 *     the four kinds says (all outputs nullable): version, bytes per value,
 *     channels, points n, max_error (0: lossless; 0 too for n = 0), scalable
 *     (versions 2 and 7), the sender's lod.  h_in may be a prefix of 12 bytes
 *     or more (16 for n > 0 of versions 4 and 7).  Anything else: PCC_E_STREAM.
 *   pcc_attr_decode_frames reads versions 1 and 4, pcc_attr_decode_frames_lod
 *     versions 2 and 7 (pcc_attr_lod_info likewise), one version per call: the
 *     first blob's; a blob of the call's other version is PCC_E_ARG naming the
 *     frame.  The near-lossless decoders keep every check of the lossless ones
 *     and add one (status 16): a reconstruction outside [-e, mask + e], which
 *     no encoder produces, is PCC_E_STREAM naming its frame. */
int pcc_attr_encode_frames_nl(pcc_ctx* ctx, int version, const void* d_values,
                              const int64_t* h_value_offsets,
                              const int32_t* h_format, const int64_t* h_rows,
                              const int64_t* h_points, int n_frames,
                              const uint32_t* d_perm,
                              const uint32_t* d_run_starts, int64_t n_unique,
                              int64_t n_kept, const uint64_t* d_keys,
                              int key_shift, int max_error, uint8_t* h_out,
                              int64_t cap, int64_t* h_offsets);
int pcc_attr_info(const uint8_t* h_in, int64_t len, int32_t* h_version,
                  int32_t* h_bpv, int32_t* h_channels, int64_t* h_points,
                  int32_t* h_max_error, int32_t* h_scalable, int32_t* h_lod);

/* Cross-channel prediction for attributes of two and more channels: attribute
 * blob versions 8, 11, 13 and 14, the cross forms of 1, 2, 4 and 7, chosen by
 * the sender frame by frame.  The channels of a camera's colour are strongly
 * correlated, and so are what the plain kinds code for them; a cross kind
 * codes the difference.
 *
 * The rule.  A frame of c >= 2 channels and a mask M, a subset of
 * {1 .. c - 1}.  Let w[i][ch] be what the plain kind codes for point i,
 * channel ch, in the plain kind's coding order: the wrapped residual r of
 * versions 1 and 2, the index j of versions 4 and 7, both integers in
 * [-h, h), h = 2^(8 bpv - 1), mask = 2^(8 bpv) - 1.  The cross kind codes
 *   x[i][ch] = w[i][ch]                                    ch = 0 or not in M
 *   x[i][ch] = ((w[i][ch] - w[i][ch-1] + h) & mask) - h    ch in M
 * a chain: channel ch against the ORIGINAL w of channel ch - 1, not against
 * x.  The decoder undoes it per point, channel by channel in ascending order,
 * w[ch] = ((x[ch] + w[ch-1] + h) & mask) - h, then continues exactly as the
 * plain kind does.  x goes through the coder as version 2's residuals do: no
 * prediction inside the run, context (channel, bucket of |x| of the channel's
 * previous point in the lane's run, 0 for the run's first point, position).
 * Binarisation, model, p0, S, chunks, word runs and the prefix rule of the
 * levels of detail are the plain kind's.
 * Consequence: a cross kind decodes to exactly the values the plain kind of
 * the same call decodes to, at every level of detail, and the near-lossless
 * bound holds unchanged.  Uncorrelated channels grow under it: the sender
 * chooses.
 * Layout: the plain kind's, with the cross version byte and byte 3 =
 * c | m << 4, bit ch - 1 of m set for ch in M (m != 0, m < 2^(c - 1); a plain
 * kind has byte 3 = c).  n = 0: the 12-byte head with those two bytes.  The
 * eight valid version bytes 1, 2, 4, 7, 8, 11, 13, 14 have odd parity, so any
 * two differ in two bits.
 *   _encode_frames_cross : pcc_attr_encode_frames_nl with h_cross, one mask m
 *     per frame (n_frames entries, not NULL): 0 gives the frame's plain kind,
 *     byte for byte; m < 0 or m >= 2^(c - 1) for the frame's c: PCC_E_ARG
 *     naming the frame.  A call whose frames with points all have m = 0 runs
 *     what _encode_frames_nl runs; any other call one elementwise launch more.
 *   _cross_mask : host only, no ctx: m of a head (0 for the plain kinds); the
 *     checks of pcc_attr_info, PCC_E_STREAM where they fail (among them a
 *     cross version byte with m = 0 or a bit at c - 1 or above, and a plain one
 *     with anything above c in byte 3).
 *   pcc_attr_decode_frames reads 8 and 13 beside 1 and 4,
 *     pcc_attr_decode_frames_lod and pcc_attr_lod_info 11 and 14 beside 2 and
 *     7, still one version per call; pcc_attr_info reports the cross version
 *     byte and c (the low nibble of byte 3). */
int pcc_attr_encode_frames_cross(pcc_ctx* ctx, int version, const void* d_values,
                                 const int64_t* h_value_offsets,
                                 const int32_t* h_format, const int64_t* h_rows,
                                 const int64_t* h_points, int n_frames,
                                 const uint32_t* d_perm,
                                 const uint32_t* d_run_starts, int64_t n_unique,
                                 int64_t n_kept, const uint64_t* d_keys,
                                 int key_shift, int max_error,
                                 const int32_t* h_cross, uint8_t* h_out,
                                 int64_t cap, int64_t* h_offsets);
int pcc_attr_cross_mask(const uint8_t* h_in, int64_t len, int32_t* h_mask);

/* Lossless attributes predicted from 3-D neighbours: attribute blob version
 * 25 and its cross-channel form 26.  Versions 1 and 2 predict along one
 * dimension (the Morton run; the one Morton-first point of the next larger
 * cell); this kind looks sideways in space and is about a tenth smaller on
 * colour.  Layout, chunks, coder, contexts, model, introduction order,
 * cells[], slod and the level-of-detail prefixes are version 2's, byte for
 * byte; only the predictor differs.  25 = 11001b and 26 = 11010b keep the odd
 * parity of the eleven bytes 1, 2, 4, 7, 8, 11, 13, 14, 19, 21, 22 and differ
 * from each of them in at least two bits.
 *
 * The rule (tests/attr_nbr_ref.py restates it in numpy).  Notation is version
 * 2's: n distinct points in Morton order, 48-bit keys, size of introduction
 * s(i), cells[], introduction order, slod.  Coordinates are biased by
 * 32768 >> slod; the lattice is [0, 65536 >> slod) per axis.
 *   Head: 'A' 25 (bpv | slod << 4) c | n | payload_len | cells[16] | S |
 *     n_chunks | p0 | words[] | chunks — version 2's with another version
 *     byte.  Version 26 puts the mask above the channels in byte 3 (c | m <<
 *     4) exactly as 11 does over 2.  An empty frame is the 12-byte head.
 *   Candidates of point i > 0: s = s(i), P its biased coordinates, u = P >> s,
 *     C = P >> (s + 1).  For each o in {-1, 0, 1}^3 whose cell C + o of side
 *     2^(s + 1) lies inside the lattice (per axis 0 <= C + o and
 *     (C + o) << (s + 1) below the lattice's side), j(o) is the frame's
 *     Morton-first point inside that cell, if the cell holds one: one lower
 *     bound over the sorted keys.  o = 0 is version 2's first(i) and always
 *     exists.  Every candidate was introduced at a size >= s + 1; its Morton
 *     index may be above i.
 *   Choice: d(o) = |(P_j >> s) - u|^2, an integer in 1 .. 27, never 0 (i and j
 *     are the first points of different cells of side 2^s).  The up to three
 *     candidates with the smallest (d, Morton index of j) are kept, each with
 *     the weight w = floor(65536 / d).
 *   Predictor per channel: p = floor((2 sum(w v_j) + sum(w)) / (2 sum(w))) in
 *     64-bit integers (three weights of 65536 times a uint16 value do not fit
 *     32 bits).  Residual r = ((v_i - p + h) & mask) - h, h = 2^(8 bpv - 1);
 *     point 0 is coded against 0.
 *   Order and coding: the residuals go in introduction order through version
 *     2's coder — no prediction inside the run; contexts = channel, bucket of
 *     the channel's previous residual in the lane's run, position.
 *   Version 26: the cross rule above applied to these residuals.
 *   Level of detail k: a point present at level k has s >= k, and u, C, the
 *     candidate cells and d are functions of P >> s and P >> (s + 1), which
 *     the cells P >> k give; the candidates' values are exact, because the
 *     kind is lossless.  So the decoder runs the same rule on its geometry's
 *     cells, biased by 32768 >> (slod + k) (slod + k <= 15), reconstructing
 *     the sizes 16 down to 0 one after the other.  Row j is the value of the
 *     Morton-first point of cell j, as version 2 defines it; the shortest
 *     prefix is version 2's formula.
 *   _encode_frames_nbr : pcc_attr_encode_frames_cross's arguments without
 *     version and max_error; h_cross may be NULL (every frame version 25);
 *     else a frame with m != 0 is version 26.  n_kept = -1: no row dropped.
 *     The other encode entry points refuse what they refused before.
 *   pcc_attr_decode_frames_lod and pcc_attr_lod_info read 25 and 26 beside
 *     2, 7, 11 and 14, still one version per call; pcc_attr_info reports the
 *     version byte with scalable = 1 and max_error = 0, pcc_attr_cross_mask
 *     the mask of a version-26 head.  A damaged blob gives PCC_E_STREAM or
 *     wrong values: every candidate index comes from a search over the
 *     decoder's own cells, none from the stream. */
int pcc_attr_encode_frames_nbr(pcc_ctx* ctx, const void* d_values,
                               const int64_t* h_value_offsets,
                               const int32_t* h_format, const int64_t* h_rows,
                               const int64_t* h_points, int n_frames,
                               const uint32_t* d_perm,
                               const uint32_t* d_run_starts, int64_t n_unique,
                               int64_t n_kept, const uint64_t* d_keys,
                               int key_shift, const int32_t* h_cross /* may be NULL */,
                               uint8_t* h_out, int64_t cap, int64_t* h_offsets);

/* Near-lossless attributes predicted from 3-D neighbours: attribute blob
 * version 28 and its cross-channel form 31, the bounded-error forms of 25 and
 * 26 as 7 and 14 are of 2 and 11.  Version 7 predicts every value from one
 * point, first(i); this kind predicts it from up to three, and is 11 to 25 %
 * smaller on colour at e = 1 .. 8.  28 = 11100b and 31 = 11111b keep the odd
 * parity of the thirteen bytes in use.
 *
 * Layout: version 7's (14's), byte for byte, under the version byte:
 *     'A' 28 (bpv | slod << 4) c | n | payload_len | max_error | cells[16] |
 *     S | n_chunks | p0 | words[] | chunks
 *   slod in byte 2; version 31: byte 3 = c | m << 4 as version 14 has it.  An
 *   empty frame is the 12-byte head.  The prefix rule is version 7's.
 * The rule (tests/attr_nbr_nl_ref.py restates it in numpy):
 *   Candidates, distances d, the tie-break on (d, Morton index) and the
 *     weights w = floor(65536 / d) are version 25's: functions of the geometry
 *     alone.  e = max_error >= 1, q = 2 e + 1, mask = 2^(8 bpv) - 1.
 *   Point 0 has p = 0.  Every other point i has, per channel,
 *     p = floor((2 sum(w v^_j) + sum(w)) / (2 sum(w))) over its candidates'
 *     DECODED values v^_j, the clamped values a decoder returns, in 64-bit
 *     integers.
 *   Index: j_i = sgn(d) floor((|d| + e) / q) with d = v_i - p.  There is no
 *     wrap: |d| <= mask, so |j_i| < 2^(8 bpv - 1).
 *   Decoded value: v^_i = clip(p + j_i q, 0, mask).  p + j_i q is within e of
 *     v_i and v_i is in range, so |v_i - v^_i| <= e.
 *   A closed loop: every candidate was introduced at a larger size than its
 *     point, so both sides form v^ size by size, 16 down to 0.
 *   The j go in introduction order through version 7's coder (contexts =
 *     channel, bucket of the channel's previous index in the lane's run,
 *     position).  Version 31 applies version 14's cross rule to them.
 *   Level of detail k: a point present at level k has size s >= k, and its
 *     candidates were introduced at sizes >= s + 1, so a decoder at a cut
 *     forms the same p from its cells alone.  Row j is v^ of the Morton-first
 *     point of cell j: within e of the row versions 25 / 26 return at that
 *     lod.
 *   A decoder forms p + j q in 64 bits (a damaged uint16 stream at e = 32767
 *     reaches 2^31), clamps to [0, mask], and reports PCC_E_STREAM where the
 *     sum lies outside [-e, mask + e], which no encoder's reconstruction
 *     does.  No index comes from the stream.
 *   _encode_frames_nbr_nl : pcc_attr_encode_frames_nbr's arguments with
 *     max_error (1 .. 2^(8 bpv - 1) - 1 of every frame) in front of h_cross,
 *     which may be NULL (every frame version 28); else a frame with m != 0 is
 *     version 31.
 *   pcc_attr_decode_frames_lod and pcc_attr_lod_info read 28 and 31 beside
 *     2, 7, 11, 14, 25 and 26, still one version per call; pcc_attr_info
 *     reports the version byte with scalable = 1 and the head's max_error,
 *     pcc_attr_cross_mask the mask of a version-31 head.  Every other entry
 *     point refuses the two bytes as it refuses any byte it does not know. */
int pcc_attr_encode_frames_nbr_nl(pcc_ctx* ctx, const void* d_values,
                                  const int64_t* h_value_offsets,
                                  const int32_t* h_format, const int64_t* h_rows,
                                  const int64_t* h_points, int n_frames,
                                  const uint32_t* d_perm,
                                  const uint32_t* d_run_starts, int64_t n_unique,
                                  int64_t n_kept, const uint64_t* d_keys,
                                  int key_shift, int max_error,
                                  const int32_t* h_cross /* may be NULL */,
                                  uint8_t* h_out, int64_t cap, int64_t* h_offsets);

/* Transform-coded attributes: attribute blob version 19, a ninth kind, lossy,
 * for rates below about a byte per point, where a near-lossless predictive
 * coder (a staircase on the prediction error) is the wrong tool.  An integer
 * lifting form of the region-adaptive hierarchical transform (G-PCC's RAHT)
 * over the binary splits of the Morton tree.
 *
 * The rule (tests/attr_transform_ref.py restates it in numpy).  Per frame, as
 * for version 2: n distinct points in Morton order, their 48-bit keys key_i
 * biased by 32768 >> slod (slod the sender's level of detail), merged values
 * v_i per channel of bpv bytes; H = 2^(8 bpv - 1), mask = 2 H - 1, and an
 * integer q = qstep in 1 .. H - 1.
 *   Sublevel of introduction: b(0) = 48; b(i) = hb(key_i xor key_{i-1}) in
 *     0 .. 47 for i > 0 (hb: highest set bit).  Point i is the first leaf of
 *     the RIGHT child of exactly one binary split of the Morton tree, the
 *     split at bit b(i): version 2's size of introduction at bit granularity
 *     (s = floor(b / 3)).
 *   The pair of point i, t = b(i) < 48:
 *     lo = lower_bound(keys, key_i with its low t + 1 bits cleared)
 *     hi = lower_bound(keys, (key_i | (2^t - 1)) + 1), within the frame
 *     wa = i - lo, wb = hi - i, w = wa + wb: the leaves of the left child,
 *     of the right child and of the node.
 *     step s = max(2, isqrt(floor(q^2 w / (wa wb)))); the product stays
 *     below 2^63.
 *   Forward: val = v, signed integers that are never clamped inside;
 *     sublevels t = 0, 1, .., 47 in that order, the pairs of a sublevel
 *     independent of each other (no two touch the same slot):
 *       h = val[i] - val[lo]
 *       val[lo] += floor(wb h / w)        floor towards -inf: the node's value,
 *                                         kept at its first leaf
 *       x[i] = sgn(h) min(floor((|h| + floor(s / 2)) / s), H - 1)
 *     (s >= 2 and |h| <= mask: the min changes an index by at most 1.)  After
 *     sublevel 47, x[0] = val[0] - H: the frame's integer weighted mean, in
 *     [-H, H), not quantised.
 *   Inverse: val[0] = x[0] + H; sublevels t = 47 .. 0, every i with b(i) = t,
 *     with the same lo, hi, wa, wb, s:
 *       h^ = x[i] s;  va = val[lo] - floor(wb h^ / w);
 *       val[lo] = va;  val[i] = va + h^
 *     and the output is clamp(val, 0, mask).
 *   The floor of 2 under the step: with a step of 1 the min clamps indices
 *     (|h| can reach mask, an index only H - 1), which cost the first form of
 *     this kind 10 dB.  The kind therefore has NO lossless setting; q = 1
 *     codes with s = 2 where q^2 w / (wa wb) < 4.
 *   Coding order: (b descending, Morton index ascending), point 0 first.  x in
 *     that order is dealt to lanes and chunks (S points per lane, as every
 *     kind) and coded exactly as version 2 codes its residuals: the same
 *     binarisation, contexts (channel, bucket of |x| of the channel's previous
 *     point in the lane's run, position; buckets not retuned), p0 and model,
 *     no prediction inside the run.
 *   Layout: 'A' 19 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 qstep |
 *     u32 S | u32 n_chunks | u16 p0[nctx] | u32 words[n_chunks] | chunk
 *     payloads: version 4's layout with version 2's slod nibble.  n = 0: the
 *     12-byte head alone, which records no q.  Byte 19 keeps the odd parity
 *     of the eight other version bytes.
 * The decoder needs the frame's keys, so a version-19 blob decodes as the
 * version-2 family does, against the cells its geometry decode left on the
 * device, and at lod 0 only: a decoder at a cut does not know how many points
 * lie under a cell and cannot form the weights, so the kind has no
 * level-of-detail prefixes.
 *   _encode_frames_transform : the arguments of pcc_attr_encode_frames_nl with
 *     version 2 (d_keys, key_shift as pcc_attr_encode_frames_v2 takes them;
 *     n_kept = -1: no row was dropped) and qstep in place of max_error:
 *     qstep < 1, or >= H for a frame's format: PCC_E_ARG.  Launches: the merge,
 *     three for the coding order, ONE synchronisation that reads which
 *     sublevels hold a point, one launch per such sublevel (at most 48, over
 *     all frames of the call at once), the mean, and the counting pass, coder
 *     and blob assembly of every kind.
 *   pcc_attr_decode_frames_lod with lod = 0 reads version 19 (one version per
 *     call; lod > 0: PCC_E_ARG): three launches for the order and the same
 *     synchronisation, the lane decoder, the root, one launch per occupied
 *     sublevel top-down, the clamp.  A blob whose point count is not that of
 *     its cells: PCC_E_STREAM.
 *   pcc_attr_info reports version 19 with max_error 0, scalable 0 and the
 *     sender's lod, from the blob or a prefix of 16 bytes or more; every part
 *     of the header that is present is checked (q in 1 .. H - 1, S and
 *     n_chunks against n, p0, the chunk table against the blob's announced
 *     length), PCC_E_STREAM where a check fails.  pcc_attr_qstep: host only,
 *     q of such a head, 0 for every other kind and for a blob without points.
 *   pcc_attr_lod_info refuses version 19 as it refuses the kinds 1, 4, 8 and
 *     13: PCC_E_ARG. */
int pcc_attr_encode_frames_transform(pcc_ctx* ctx, const void* d_values,
                                     const int64_t* h_value_offsets,
                                     const int32_t* h_format, const int64_t* h_rows,
                                     const int64_t* h_points, int n_frames,
                                     const uint32_t* d_perm,
                                     const uint32_t* d_run_starts, int64_t n_unique,
                                     int64_t n_kept, const uint64_t* d_keys,
                                     int key_shift, int qstep, uint8_t* h_out,
                                     int64_t cap, int64_t* h_offsets);
int pcc_attr_qstep(const uint8_t* h_in, int64_t len, int32_t* h_qstep);

/* Transform-coded attributes with a colour transform and one step per channel:
 * attribute blob version 21, a tenth kind.  It is version 19 with a colour
 * word and c steps where version 19 keeps its one q; every lossy image, video
 * and point-cloud coder decorrelates colour first (luma and two chroma
 * differences) and gives each channel its own step, G-PCC's RAHT included.
 *
 * The rule (tests/attr_colour_ref.py restates it in numpy).  Everything is
 * version 19's -- keys, sublevels, pairs, weights, the forward and inverse
 * lift, the mean, the coding order, the entropy stage, the clamp of an index
 * at H - 1 -- except the following.
 *   Steps: q[ch] in 1 .. H - 1 for every channel ch < c.  The step of a pair
 *     in channel ch is s[ch] = max(2, isqrt(floor(q[ch]^2 w / (wa wb)))).
 *     With all q[ch] equal and no colour transform the indices are exactly
 *     version 19's; only the head differs.
 *   Colour transform (colour = 1; frames with c >= 3; channels 0, 1, 2 are R,
 *     G, B, a fourth channel is untouched).  Applied to the merged values of
 *     every distinct point after the merge and before the first lift.  All
 *     arithmetic on signed integers, >> the arithmetic shift (floor),
 *     H = 2^(8 bpv - 1), mask = 2 H - 1:
 *       co = R - B;  t = B + (co >> 1);  cg = G - t;  y = t + (cg >> 1)
 *       Y = y,  Co = (co >> 1) + H,  Cg = (cg >> 1) + H
 *     all three in 0 .. mask: YCoCg-R with the low bit of each chroma
 *     difference dropped, so the values fit the value width, a node's value
 *     stays a uint16 in the lift and the index clamp stays as it is.
 *   Inverse, applied to the inverse lift's output after its clamp to
 *     0 .. mask, then clamped again per channel:
 *       co' = 2 (Co - H);  cg' = 2 (Cg - H);  t = Y - (cg' >> 1)
 *       G = cg' + t;  B = t - (co' >> 1);  R = B + co'
 *     Without quantisation the round trip moves no channel by more than 1.
 *     For bpv = 1: (255, 255, 255) -> (255, 128, 128) -> (255, 255, 255);
 *     (255, 0, 0) -> (63, 255, 64) -> (254, 0, 0), G = -1 before the clamp;
 *     (0, 255, 0) -> (127, 128, 255); (0, 0, 255) -> (63, 0, 64).
 *   Layout: 'A' 21 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 colour |
 *     u32 q[c] | u32 S | u32 n_chunks | u16 p0[nctx] | u32 words[n_chunks] |
 *     chunk payloads.  colour: 0 none, 1 the transform above; anything else,
 *     and 1 with c < 3, is PCC_E_STREAM.  n = 0: the 12-byte head alone, which
 *     records neither colour nor steps.  Byte 21 keeps the odd parity of the
 *     nine other version bytes.
 *   _encode_frames_transform2 : the arguments of
 *     pcc_attr_encode_frames_transform with h_qstep[4], colour in place of
 *     qstep; a frame reads its first c entries.  A step < 1, or >= H for a
 *     frame's format: PCC_E_ARG naming the frame; so is colour outside {0, 1},
 *     and colour = 1 with a frame of fewer than 3 channels.  Launches: version
 *     19's, and with colour = 1 one elementwise pass between the merge and the
 *     coding order.
 *   pcc_attr_decode_frames_lod with lod = 0 reads version 21 (one version per
 *     call; lod > 0: PCC_E_ARG): version 19's launches, the last of them the
 *     inverse colour store where a frame of the call has colour = 1.
 *   pcc_attr_info reports version 21 as it reports 19, from the blob or a
 *     prefix that reaches q[c - 1] (16 + 4 c bytes).  pcc_attr_transform_info:
 *     host only, the colour word and the steps of such a head (h_qstep[ch] = 0
 *     for ch >= c); 0s for every other kind and for a blob without points.
 *     pcc_attr_qstep stays as it is: 0 for version 21.
 *   pcc_attr_lod_info refuses version 21 as it refuses 19: PCC_E_ARG. */
int pcc_attr_encode_frames_transform2(pcc_ctx* ctx, const void* d_values,
                                      const int64_t* h_value_offsets,
                                      const int32_t* h_format, const int64_t* h_rows,
                                      const int64_t* h_points, int n_frames,
                                      const uint32_t* d_perm,
                                      const uint32_t* d_run_starts, int64_t n_unique,
                                      int64_t n_kept, const uint64_t* d_keys,
                                      int key_shift, const int32_t h_qstep[4],
                                      int colour, uint8_t* h_out, int64_t cap,
                                      int64_t* h_offsets);
int pcc_attr_transform_info(const uint8_t* h_in, int64_t len, int32_t* h_colour,
                            int32_t h_qstep[4]);

/* Transform-coded attributes with level-of-detail prefixes: attribute blob
 * version 22, an eleventh kind.  Versions 19 and 21 weigh a split by the
 * leaves under its two children, which a decoder that holds a geometry prefix
 * cannot count.  Version 22 is version 21 under weights such a decoder can
 * form: the sender names its deepest cut K; above K a split is weighed by the
 * K-cells under its children, inside a K-cell by its level alone.
 *
 * The rule (tests/attr_scalable_ref.py restates it in numpy).  Everything is
 * version 21's -- keys, sublevels b(i), the pairs lo / hi, x[0], the coding
 * order, the entropy stage, the clamp of an index at H - 1, the colour word,
 * one step q[ch] per channel -- except the weights, the steps and the head.
 * Per frame: n distinct points in Morton order, keys key_i biased by
 * 32768 >> slod; K = scalable_to, 1 <= K, slod + K <= 15.
 *   K-cells: first(i) = 1 if i == 0 or key_i >> 3 K != key_{i-1} >> 3 K.
 *     g(i) = the number of firsts among points 0 .. i - 1; C = g(n).  A node
 *     split at bit t >= 3 K begins and ends on K-cell boundaries, so
 *     g(b) - g(a) is the exact number of K-cells in [a, b).
 *   Scale: M = max(1, floor((2 n + C) / (2 C))), the rounded mean number of
 *     points in a K-cell.
 *   The pair of point i at t = b(i) >= 3 K: ca = g(i) - g(lo),
 *     cb = g(hi) - g(i), w = ca + cb stand where version 19 has wa, wb, w in
 *     both lifts.  s[ch] = max(2, isqrt(floor(q[ch]^2 w / (ca cb M)))).
 *     q^2 w < 2^58; ca cb M < 2^55 because M (ca + cb) <= n + C / 2.
 *   A pair at t < 3 K (inside a K-cell; hi is not needed):
 *     forward val[lo] += floor(h / 2); inverse va = val[lo] - floor(h^ / 2);
 *     s[ch] = max(2, isqrt(floor(2 q[ch]^2 / 2^floor(2 t / 3)))).
 *   Decoding at a cut j, 0 <= j <= K: the same procedure on the m_j = count[j]
 *     cell keys kappa = key >> 3 j that the geometry decode at lod j leaves,
 *     biased by 32768 >> (slod + j).  b'(r) = hb(kappa_r xor kappa_{r-1}), the
 *     absolute sublevel t = b' + 3 j; K-cells are kappa >> 3 (K - j); the
 *     coefficients are the first m_j of the coding order; the inverse runs
 *     over sublevels 47 .. 3 j; M from the head's n and count[K].  Row r is
 *     the node value of cell r -- the cell's mean under the rule's weights,
 *     not version 2's sample of the Morton-first point -- clamped, then
 *     colour-inverted as version 21's values are.  Cells that give another
 *     count at a level from j up than the head (count[K] among them):
 *     PCC_E_STREAM.
 *   Layout: 'A' 22 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 colour |
 *     u32 q[c] | u32 K | u32 count[16] | u32 S | u32 n_chunks | u16 p0[nctx] |
 *     u32 words[n_chunks] | chunk payloads.  count[j] = #{i : b(i) >= 3 j},
 *     version 2's.  n = 0: the 12-byte head alone.  Byte 22 = 10110b keeps the
 *     odd parity of the ten other version bytes.  The prefix of lod j is
 *     version 2's, from count[j], S and the last needed chunk's length table.
 *   _encode_frames_transform3 : the arguments of _transform2 and scalable_to
 *     = K in 1 .. 15 - key_shift / 3 (else PCC_E_ARG).  Launches: version
 *     21's, one pass that flags the K-cell firsts and the device-wide scan
 *     behind the coding order, the 16 counts for the head, and the lift under
 *     the new weights in place of version 21's.  No further synchronisation.
 *   pcc_attr_decode_frames_lod reads version 22 at lod 0 .. K of every blob of
 *     the call (one version per call; blobs or the prefixes pcc_attr_lod_info
 *     names; lod > K: PCC_E_ARG), against the cells of the geometry at lod.
 *   pcc_attr_lod_info accepts version 22 for lod <= K, PCC_E_ARG above.
 *   pcc_attr_info reports version 22 with scalable = 1, from the blob or a
 *     prefix that reaches K (20 + 4 c bytes); pcc_attr_transform_info its
 *     colour word and steps; pcc_attr_scalable_to: host only, K of such a
 *     head, 0 for every other kind and for a blob without points. */
int pcc_attr_encode_frames_transform3(pcc_ctx* ctx, const void* d_values,
                                      const int64_t* h_value_offsets,
                                      const int32_t* h_format, const int64_t* h_rows,
                                      const int64_t* h_points, int n_frames,
                                      const uint32_t* d_perm,
                                      const uint32_t* d_run_starts, int64_t n_unique,
                                      int64_t n_kept, const uint64_t* d_keys,
                                      int key_shift, const int32_t h_qstep[4],
                                      int colour, int scalable_to, uint8_t* h_out,
                                      int64_t cap, int64_t* h_offsets);
int pcc_attr_scalable_to(const uint8_t* h_in, int64_t len, int32_t* h_scalable_to);

/* Versions 19 and 21 under a byte target per frame.  No blob format changes:
 * a frame coded under a target is, byte for byte, the version 19 or 21 blob
 * that _encode_frames_transform / _transform2 write at the steps the search
 * below chooses.  tests/attr_rate_ref.py restates the rule in numpy.
 *
 * Ladder.  For a frame of c channels and bpv bytes per value, H = 2^(8 bpv - 1),
 * base steps q[ch] in 1 .. H - 1 (the caller's qstep, the finest it accepts)
 * and the quarter-octave multipliers m = (16, 19, 23, 27), rung j = 0, 1, ..
 * has the steps
 *     q_j[ch] = min(H - 1, ((q[ch] * m[j % 4]) << (j / 4)) >> 4).
 * The ladder ends with the first rung whose steps are all H - 1, that rung
 * included; J is the number of rungs (at most 61: uint16, q = 1).  Rung 0 is
 * q itself; rungs may repeat (they give the same blob).  uint8, q = (32):
 * 32 38 46 54 64 76 92 108 127, J = 9.
 *
 * Length.  len_f(j) = the length of the blob that the existing call writes for
 * frame f at the steps of rung j, everything else (colour, key_shift, dropped
 * rows) as in this call.
 *
 * Search.  Lengths are not monotone in the step, so the procedure is the rule.
 * Per frame f with target B_f >= 1:
 *   1. A = { j : j % 4 == 0 } and J - 1, ascending.
 *   2. a = the first rung of A with len_f(a) <= B_f.
 *   3. No rung of A fits: the frame gets rung J - 1 and is over its target;
 *      the call does not fail.
 *   4. a = 0: the frame gets rung 0.
 *   5. Otherwise, with a' the rung of A in front of a: the first j in
 *      a' < j < a with len_f(j) <= B_f, or a where there is none.
 * A frame without points gets the 12-byte empty blob, whatever its target.
 *
 *   pcc_attr_rate_ladder : host only.  h_steps [64][4] receives the ladder
 *     (0 behind channel c), *h_rungs = J.  c outside 1 .. 4, bpv outside
 *     {1, 2}, a step < 1 or >= H: PCC_E_ARG.
 *   pcc_attr_encode_frames_rate : the arguments of _transform2 up to
 *     key_shift, then h_qstep[4], per_channel (0: version 19 from h_qstep[0],
 *     colour must be 0; 1: version 21 from h_qstep[0 .. c - 1] and colour),
 *     h_target[n_frames] and scratch_limit.  h_rung (nullable) receives the
 *     rung of every frame, -1 for a frame without points.  Checks and
 *     messages are _transform2's; a target < 1: PCC_E_ARG naming the frame;
 *     more bytes than cap: PCC_E_NOMEM, nothing written; the ctx stays usable
 *     after an error.  Version 22 has other weights and is not offered.
 *     The forward lift does not depend on the step, so merge, colour
 *     transform, coding order and lift run once; a quantiser pass then forms
 *     the indices of candidate rows (a frame at a rung), which the coder's
 *     counting pass and lane coder take as frames of their own, all rows of a
 *     stage in one launch each.  Stage 1 codes the rungs of A of every frame,
 *     stage 2 the at most three rungs of step 5; a row's length is its head
 *     plus twice the sum of its chunks' words, so only the winners' blobs are
 *     assembled.  Synchronisations: the coding order's, one per stage (stage
 *     2 only where a frame reaches step 5), the blobs' lengths.
 *     scratch_limit (bytes; 0: 1 GiB): a candidate row takes its indices and
 *     two record arrays of n_chunks * 64 * T words (about 190 MB for a
 *     1M-point RGB frame).  The rows of a stage are coded in groups that fit
 *     the limit, one row always allowed; a winner whose group had to give its
 *     scratch to a later one is coded once more before assembly.  Bytes and
 *     rungs do not depend on the limit. */
int pcc_attr_rate_ladder(const int32_t h_qstep[4], int c, int bpv, int32_t* h_steps,
                         int32_t* h_rungs);
int pcc_attr_encode_frames_rate(pcc_ctx* ctx, const void* d_values,
                                const int64_t* h_value_offsets, const int32_t* h_format,
                                const int64_t* h_rows, const int64_t* h_points,
                                int n_frames, const uint32_t* d_perm,
                                const uint32_t* d_run_starts, int64_t n_unique,
                                int64_t n_kept, const uint64_t* d_keys, int key_shift,
                                const int32_t h_qstep[4], int per_channel, int colour,
                                const int64_t* h_target, int64_t scratch_limit,
                                uint8_t* h_out, int64_t cap, int64_t* h_offsets,
                                int32_t* h_rung);

/* ---- exact nearest neighbours on the lattice: the D1 metric (csrc/nn.hip, the walk in csrc/nn_cells.h) -- */

/* The rule (tests/nn_ref.py restates it in numpy).  For a frame f there are
 * two sets of lattice points, every coordinate in [-32768, 32767]:
 *   queries    Q_f, a multiset: duplicates count, as pc_error counts them;
 *   reference  R_f, distinct points in Morton order.
 * For q in Q_f
 *   d2(q)  = min over r in R_f of (qx-rx)^2 + (qy-ry)^2 + (qz-rz)^2, an
 *            unsigned 64-bit integer (at most 3 * 65535^2 = 12 884 508 675,
 *            above 2^32);
 *   row(q) = the row of the minimiser among the call's sorted reference keys
 *            (counted over the whole call, not from the frame's first row);
 *            among equidistant minimisers the SMALLEST row, the Morton-first.
 * Only points of the same frame are candidates.  Per frame: count = |Q_f|,
 * sum = the sum of d2(q) (uint64: 2^27 rows * 2^34 < 2^64), max = the largest
 * d2(q).  A frame with queries and an empty reference: each such query gets
 * d2 = 2^64 - 1 and row = -1, and the frame's three statistics are 0.
 *
 *   pcc_nn_frames : d_qkeys: Morton keys of the queries (pcc_morton_keys_frames),
 *     in any order, duplicates allowed; d_rkeys: the reference keys, sorted and
 *     distinct, as pcc_octree_encode_frames takes them.  Outputs, each
 *     nullable: d_sqdist [n_q], d_row [n_q], d_stats [n_frames][3] (count,
 *     sum, max; zeroed by the call).  One thread per query walks the implicit
 *     octree of the sorted keys of its frame without a stack; the result does
 *     not depend on the order of the queries, sorted queries are faster.
 *     Checked before the search is launched (one synchronisation): n_frames in
 *     1 .. 65535 and n_q, n_r <= 2^27 (PCC_E_ARG); a reference or query key
 *     whose frame index is not below n_frames (PCC_E_RANGE); reference keys
 *     not sorted (PCC_E_ARG) or not distinct (PCC_E_DUP), as
 *     pcc_octree_encode_frames reports them; pcc_last_error says which.
 *     n_q = 0 and n_r = 0 launch no search (n_r = 0 fills the sentinels).
 *   pcc_nn_attr_sse_frames : the attribute side of the same pairing.  d_row:
 *     pcc_nn_frames' rows for d_qkeys; d_a [n_q][channels] and d_b
 *     [n_r][channels]: values of bpv = 1 (uint8) or 2 (uint16) bytes, 1 .. 4
 *     channels, row i of d_a belonging to query i and row j of d_b to
 *     reference row j.  d_sse [n_frames][channels] (zeroed by the call):
 *     the sum over the frame's queries of (a[i][ch] - b[row[i]][ch])^2, uint64.
 *     A query whose row is -1 adds nothing.
 *   pcc_nn_replay_host : host only, no ctx.  The traversal of pcc_nn_frames,
 *     the same function compiled for the host, run query by query on the
 *     calling thread: d2, row and the nodes each query tried (cells tested and
 *     points measured), each output nullable.  For counting nodes and for
 *     checks where there is no device; not a product path. */
int pcc_nn_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, int64_t n_q,
                  const uint64_t* d_rkeys, int64_t n_r, int n_frames,
                  uint64_t* d_sqdist, int32_t* d_row, uint64_t* d_stats);
int pcc_nn_attr_sse_frames(pcc_ctx* ctx, const uint64_t* d_qkeys,
                           const int32_t* d_row, int64_t n_q, const void* d_a,
                           const void* d_b, int64_t n_r, int bpv, int channels,
                           int n_frames, uint64_t* d_sse);
int pcc_nn_replay_host(const uint64_t* h_qkeys, int64_t n_q,
                       const uint64_t* h_rkeys, int64_t n_r, uint64_t* h_sqdist,
                       int32_t* h_row, uint32_t* h_nodes);

/* ---- k nearest neighbours, surface normals (csrc/knn.hip), the D2 metric (csrc/nn.hip) -- */

/* The rules (tests/normals_ref.py restates them in numpy).
 *
 * k nearest neighbours.  Per frame the reference R is the frame's distinct
 * points in Morton order (sorted distinct keys, the frame index above bit 48);
 * the queries are those same points.  For a point p and an integer k in
 * 3 .. 32, knn(p) is the first k_eff = min(k, n_f) rows of the frame ordered by
 * (|r - p|^2, row) ascending: p itself is its own nearest neighbour, at
 * distance 0 (Open3D's KDTreeSearchParamKNN convention), and among equidistant
 * rows the smaller row (Morton-first) comes first.  Rows are counted over the
 * whole call's keys, as pcc_nn_frames counts them.  Slots k_eff .. k - 1 hold
 * row -1 and d2 = 2^64 - 1.  Distances are unsigned 64-bit integers, at most
 * 3 * 65535^2.  Only points of the same frame are candidates.
 *
 * Scatter matrix.  With d_j = r_j - p over the m = k_eff neighbours (the zero
 * vector of p itself included),
 *   C = m * sum d_j d_j^T - (sum d_j)(sum d_j)^T,
 * m^2 times the covariance, exact in int64: |C| <= 2 * 32 * 32 * 65535^2 < 2^46.
 * Stored as six int64: xx, xy, xz, yy, yz, zz.
 *
 * Normal.  A unit eigenvector of C for its smallest eigenvalue, computed in
 * float64 on the device and returned as float32 [3].  Where the eigenspace has
 * more than one dimension (collinear neighbours, a symmetric lattice
 * neighbourhood) any unit vector of it is right.  The result is always finite
 * and of unit length.  A frame with fewer than 3 distinct points has no normal:
 * (0, 0, 0) and C = 0 are written for its points.  Sign: with a viewpoint
 * (three int32 lattice coordinates, e.g. the sensor) n is flipped where
 * n . (viewpoint - p) < 0; without one the sign is unspecified.
 *
 * D2 (point-to-plane).  Only side A (the original) carries normals, as with
 * pc_error -n: the normal of a pair is always the normal of the pair's A point.
 *   A -> B: for row a of A with r = nn_B(a), proj(a) = ((a - b_r) . n_a)^2;
 *   B -> A: for row b of B with r = nn_A(b), proj(b) = ((b - a_r) . n_{a_r})^2.
 * The dot product is formed in float64 as (ex*nx + ey*ny) + ez*nz: each product
 * is an integer of at most 17 bits times a float32, exact in float64, so the
 * value does not depend on fma contraction.  d2_mse = sum proj / count;
 * d2_psnr = 10 log10(3 peak^2 / max(d2_mse_ab, d2_mse_ba)).
 *
 *   pcc_knn_frames : d_keys: n sorted distinct keys of n_frames frames.
 *     Outputs, each written only when its pointer is non-null: d_rows [n][k],
 *     d_sqdist [n][k], d_cov [n][6], d_normals [n][3]; h_viewpoint: three
 *     int32 on the host, or null.  One thread per point walks the implicit
 *     octree of its frame's keys without a stack, the k best in registers.
 *     Checked before the search is launched (one synchronisation): k in
 *     3 .. 32, n <= 2^27 and n_frames in 1 .. 65535 (PCC_E_ARG); keys not
 *     sorted (PCC_E_ARG) or not distinct (PCC_E_DUP); a frame index not below
 *     n_frames (PCC_E_RANGE).  n = 0 launches nothing.
 *   pcc_nn_d2_frames : d_row: pcc_nn_frames' rows of d_qkeys among d_rkeys;
 *     d_normals: float32 [.][3]; d_normal_row [n_q]: the row of d_normals to
 *     use for query i, null: row i (the caller keeps them inside d_normals).
 *     d_proj [n_q] (nullable): proj per query; d_sum [n_frames] (nullable,
 *     zeroed by the call): the frame's sum of proj, float64, added in an
 *     unspecified order.  A row of -1 or out of range, a negative normal row
 *     or a frame index not below n_frames adds nothing (proj 0).
 *   pcc_knn_replay_host : host only, no ctx.  The traversal and the epilogue
 *     of pcc_knn_frames, the same functions compiled for the host, without a
 *     viewpoint; additionally h_nodes [n]: the nodes each query tried (cells
 *     tested and points measured).  k and n as above (PCC_E_ARG), keys not
 *     sorted (PCC_E_ARG) or not distinct (PCC_E_DUP).  Not a product path. */
int pcc_knn_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames,
                   int k, int32_t* d_rows, uint64_t* d_sqdist, int64_t* d_cov,
                   float* d_normals, const int32_t* h_viewpoint);
int pcc_nn_d2_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, const int32_t* d_row,
                     int64_t n_q, const uint64_t* d_rkeys, int64_t n_r,
                     const float* d_normals, const int32_t* d_normal_row,
                     int n_frames, double* d_proj, double* d_sum);
int pcc_knn_replay_host(const uint64_t* h_keys, int64_t n, int k, int32_t* h_rows,
                        uint64_t* h_sqdist, int64_t* h_cov, float* h_normals,
                        uint32_t* h_nodes);

/* ---- outlier removal by exact k-NN (csrc/outlier.h, behind csrc/knn.hip's search) -- */

/* The rules (tests/outlier_ref.py restates them in Python integers).  Both are
 * per frame, over the frame's n DISTINCT lattice points in Morton order (n
 * sorted distinct keys, as pcc_knn_frames takes them); only points of the same
 * frame are neighbours.
 *
 * Statistical (k in 3 .. 32, std_ratio >= 0).  The neighbours of a point are
 * those of pcc_knn_frames at that k: the point itself at distance 0 (Open3D's
 * nb_neighbors convention), k_eff = min(k, n), ties to the smaller row.
 *   score      q_i = sum over j < k_eff of floor(16 sqrt(d2_ij)), an unsigned
 *              integer.  Each term is the exact integer square root of d2 << 8
 *              (d2 <= 3 * 65535^2, so d2 << 8 < 2^42): sqrt in float64 followed
 *              by the fix-up  while (r*r > x) --r; while ((r+1)*(r+1) <= x) ++r;
 *              so the result does not rest on how any sqrt rounds.  All points
 *              of a frame share k_eff: comparing sums is comparing Open3D's
 *              mean distances.  q_i < 32 * 2^21 = 2^26.
 *   frame sums S1 = sum q_i and S2 = sum q_i^2, exact integers, independent of
 *              the order of summation.  S1 < 2^53.  q_i^2 < 2^52 times
 *              n <= 2^27 does not fit one word: the device accumulates
 *              sum (q_i^2 & 0xffffffff) and sum (q_i^2 >> 32) in two uint64 and
 *              the host joins them, S2 = lo + (hi << 32).
 *   threshold  on the host, in arbitrary-precision integers, between the two
 *              kernels.  R = rint(256 * std_ratio), std_ratio <= 255.  T is the
 *              largest integer t with
 *                n t <= S1   or   65536 (n - 1) (n t - S1)^2 <= R^2 n (n S2 - S1^2),
 *              that is t <= mean + (R / 256) std with the sample standard
 *              deviation (divisor n - 1) that Open3D uses.  In closed form
 *                T = (S1 + isqrt(R^2 n (n S2 - S1^2) div (65536 (n - 1)))) div n.
 *              A frame with n < 2 keeps everything: T = 2^64 - 1.  T is never
 *              formed in floating point or on the device (the products pass
 *              2^128).
 *   verdict    point i is kept iff q_i <= T.
 *
 * Radius (min_neighbours m in 1 .. 31, radius2 a non-negative integer in
 * squared lattice units).  Point i is kept iff at least m OTHER points of its
 * frame lie at d2 <= radius2; equivalently n > m and slot m of its k-NN list
 * at k = m + 1 (slot 0 is the point itself) has d2 <= radius2.  With
 * m = nb_points this is Open3D's remove_radius_outlier (which counts the point
 * itself and asks for more than nb_points).  radius2 above 3 * 65535^2 is legal
 * and keeps every frame of more than m points.
 *
 *   pcc_outlier_scores_frames : d_keys: n sorted distinct keys of n_frames
 *     frames.  One thread per point runs pcc_knn_frames' search and forms q_i
 *     in the same thread; d_scores [n] takes q_i and d_sums [n_frames][4]
 *     (zeroed by the call) takes S1, sum (q^2 & 0xffffffff), sum (q^2 >> 32) and
 *     the frame's n.  Nothing of shape [n][k] is written.  Checked before
 *     anything is launched (one synchronisation), as pcc_knn_frames checks:
 *     k in 3 .. 32, n <= 2^27, n_frames in 1 .. 65535 (PCC_E_ARG); keys not
 *     sorted (PCC_E_ARG) or not distinct (PCC_E_DUP); a frame index not below
 *     n_frames (PCC_E_RANGE).  n = 0 launches nothing (the sums are zeroed).
 *   pcc_outlier_mask_frames : d_keep [n] = q_i <= d_threshold[frame of i]
 *     (1 / 0), d_kept [n_frames] (zeroed by the call) the kept points of every
 *     frame.  d_threshold: n_frames uint64 on the device.  The same checks.
 *   pcc_outlier_radius_frames : the radius rule; d_keep [n], d_counts
 *     [n_frames][2] (zeroed by the call): the frame's n and its kept points.
 *     The search holds m + 1 entries and its pruning bound never exceeds
 *     radius2 + 1, so a point stops after the cells within its radius; the
 *     verdict is the unbounded search's.  min_neighbours in 1 .. 31
 *     (PCC_E_ARG), otherwise the same checks.
 *   pcc_outlier_compact_rows : from verdicts on distinct points to the input
 *     rows of a call.  d_index [n]: pcc_rows_index' result with no frame's rows
 *     taken off (the distinct row of every input row over the whole call, -1
 *     for a dropped row); d_keep [n_keys]; d_offsets [n_frames + 1]: the input
 *     rows' frame offsets.  d_mask [n] (nullable): the verdict of every input
 *     row; d_kept_rows [n]: for the kept rows in input order, the row's place
 *     inside its own frame; d_kept_offsets [n_frames + 1]: the kept rows in
 *     front of every frame, and their total.  No synchronisation.
 *   pcc_gather_rows_pitched : d_dst row t (tight) = row d_rows[t] of d_src,
 *     whose n_src rows of row_bytes lie pitch_bytes apart; any row_bytes up to
 *     4096 (pcc_gather_rows takes multiples of 4 of tight rows only).  A row
 *     not below n_src is written as zeros.
 *   pcc_outlier_isqrt_host : floor(sqrt(x)) as the score forms it, x < 2^42
 *     (2^64 - 1 above).  Host only.
 *   pcc_outlier_replay_host : host only, no ctx.  The kernels' functions
 *     compiled for the host, row by row on the calling thread; every output is
 *     nullable.  h_scores [n], h_sums [n_frames][4], h_nodes [n] (the nodes the
 *     score's search tried); h_keep [n] = h_scores <= h_threshold[frame] (needs
 *     both); h_keep_radius / h_nodes_radius [n]: the radius rule under the
 *     bounded search; h_keep_unbounded / h_nodes_unbounded [n]: under
 *     pcc_knn_frames' own search.  k, min_neighbours, n, n_frames as above
 *     (PCC_E_ARG, PCC_E_DUP, PCC_E_RANGE).  Not a product path. */
int pcc_outlier_scores_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                              int n_frames, int k, uint64_t* d_scores,
                              uint64_t* d_sums);
int pcc_outlier_mask_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                            int n_frames, const uint64_t* d_scores,
                            const uint64_t* d_threshold, uint8_t* d_keep,
                            uint64_t* d_kept);
int pcc_outlier_radius_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n,
                              int n_frames, int min_neighbours, uint64_t radius2,
                              uint8_t* d_keep, uint64_t* d_counts);
int pcc_outlier_compact_rows(pcc_ctx* ctx, const int32_t* d_index, int64_t n,
                             const uint8_t* d_keep, int64_t n_keys,
                             const int64_t* d_offsets, int n_frames,
                             uint8_t* d_mask, uint32_t* d_kept_rows,
                             int64_t* d_kept_offsets);
int pcc_gather_rows_pitched(pcc_ctx* ctx, const void* d_src, int64_t n_src,
                            int64_t pitch_bytes, const uint32_t* d_rows,
                            int64_t n, int row_bytes, void* d_dst);
uint64_t pcc_outlier_isqrt_host(uint64_t x);
int pcc_outlier_replay_host(const uint64_t* h_keys, int64_t n, int n_frames, int k,
                            int min_neighbours, uint64_t radius2,
                            const uint64_t* h_threshold, uint64_t* h_scores,
                            uint64_t* h_sums, uint8_t* h_keep, uint32_t* h_nodes,
                            uint8_t* h_keep_radius, uint32_t* h_nodes_radius,
                            uint8_t* h_keep_unbounded,
                            uint32_t* h_nodes_unbounded);

/* ---- DBSCAN clusters by union-find (csrc/cluster.h, behind csrc/knn.hip's search) -- */

/* The rule (tests/cluster_ref.py restates it in Python integers).  It is per
 * frame, over the frame's n DISTINCT lattice points in Morton order (n sorted
 * distinct keys, as pcc_knn_frames takes them); only points of the same frame
 * are neighbours.  Parameters: radius2, an integer in 0 .. 4096 (squared
 * lattice units); min_neighbours m in 0 .. 31; min_points in 1 .. 2^27.
 *   1 core points   point i is a core point iff at least m OTHER points lie at
 *                   d2 <= radius2: the radius rule of pcc_outlier_radius_frames,
 *                   word for word.  With m = 0 every point is a core point and
 *                   the rule is plain Euclidean clustering (connected
 *                   components; PCL's EuclideanClusterExtraction).
 *   2 edges         two core points i and j are joined iff d2(i, j) <= radius2
 *                   (inclusive).
 *   3 components    the connected components of the core points.  The root of
 *                   a component is its smallest row: its Morton-first core
 *                   point.
 *   4 border points a point that is not a core point belongs to the component
 *                   of its nearest core point with d2 <= radius2; among
 *                   equidistant core points the SMALLEST row wins.  A point
 *                   with no such core point is noise.  A border point never
 *                   joins two components.  (DBSCAN, Open3D's cluster_dbscan,
 *                   with the one order-dependent choice of the textbook
 *                   algorithm made deterministic.)
 *   5 size, pruning the size of a component is its core points plus its border
 *                   points; a component with size < min_points is noise as a
 *                   whole.
 *   6 numbering     the components that remain are numbered 0 .. K-1 by (size
 *                   descending, root row ascending): label 0 is the largest
 *                   cluster.  Every noise point has label -1.
 * The result is a function of the point set alone: not of scheduling, of the
 * order of input rows, or of which frames share a call.
 * radius2 above 4096 is PCC_E_ARG, as a condition and not a measurement: a
 * point's walk visits every point within its radius, and radius 64 bounds
 * that work per thread.  Coarser needs cluster coarser points, p >> k.
 *
 *   pcc_cluster_frames : d_keys: n sorted distinct keys of n_frames frames.
 *     d_labels int32 [n]; d_sizes uint32 [n], nullable: frame f's K_f sizes in
 *     label order from the frame's first row on, the rest zero; d_counts
 *     [n_frames][4] (zeroed by the call): points, core points, clusters K,
 *     noise points.  Core flags by pcc_outlier_radius_frames' kernel (m = 0: a
 *     fill); one walk per point under the constant bound radius2, in which a
 *     core point unites with the core points in front of it (lock-free
 *     union-find, the larger root under the smaller; relaxed agent-scope
 *     atomics only, no fence, no waiting) and any other point keeps its
 *     nearest core point; no list of neighbours is written.  A second launch
 *     flattens; sizes, the min_points cut, the numbering (one stable sort) and
 *     the counts follow on the device, with no host array of size n.  Checks
 *     and refusals are those of pcc_outlier_radius_frames (one synchronisation
 *     in front), and min_neighbours, radius2, min_points in their ranges
 *     (PCC_E_ARG; pcc_last_error names the argument).  n = 0 launches nothing
 *     (the counts are zeroed).  After an error the ctx stays usable.  The
 *     counts are the caller's to read behind a synchronisation of its own.
 *   pcc_cluster_replay_host : host only, no ctx.  The kernels' functions
 *     compiled for the host, row by row on the calling thread; every output is
 *     nullable.  h_labels, h_sizes, h_counts as above; h_core uint8 [n];
 *     h_root int32 [n]: the root row (a row of the call) of the point's
 *     component before pruning and numbering, -1 for a point without one;
 *     h_nodes [n]: the nodes each walk tried.  Not a product path.
 *   pcc_cluster_replay_host_reversed : the same with every frame's walks, and
 *     so the unions, issued from the last row to the first: the result must
 *     not differ. */
int pcc_cluster_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames,
                       int min_neighbours, uint64_t radius2, int64_t min_points,
                       int32_t* d_labels, uint32_t* d_sizes, uint64_t* d_counts);
int pcc_cluster_replay_host(const uint64_t* h_keys, int64_t n, int n_frames,
                            int min_neighbours, uint64_t radius2, int64_t min_points,
                            int32_t* h_labels, uint32_t* h_sizes, uint64_t* h_counts,
                            uint8_t* h_core, int32_t* h_root, uint32_t* h_nodes);
int pcc_cluster_replay_host_reversed(const uint64_t* h_keys, int64_t n, int n_frames,
                                     int min_neighbours, uint64_t radius2,
                                     int64_t min_points, int32_t* h_labels,
                                     uint32_t* h_sizes, uint64_t* h_counts,
                                     uint8_t* h_core, int32_t* h_root,
                                     uint32_t* h_nodes);

/* ---- attribute transfer onto another geometry: recolouring (csrc/transfer.hip) -- */

/* The rule (tests/transfer_ref.py restates it in numpy, on tests/nn_ref.py).
 * Per frame there are two sides:
 *   source  S, a multiset of lattice points, every row with a value of 1 .. 4
 *           channels, uint8 or uint16; duplicates count row by row, as the
 *           queries of pcc_nn_frames do;
 *   target  T, distinct lattice points in Morton order.
 * Two searches under the rule of pcc_nn_frames above, ties to the SMALLEST row:
 *   backward  b(s) = the row of the nearest target of source row s;
 *   forward   f(t) = the row of the nearest DISTINCT source point of target t
 *             (rows among the frame's distinct source points in Morton order).
 * For a target t let B(t) = { s : b(s) = t } and cnt(t) = |B(t)|.  Per channel
 *   cnt > 0   out[t] = (sum over s in B(t) of v[s] + cnt / 2) / cnt, the
 *             project's merge rule for duplicate points (integer division, the
 *             sum in 64 bits: 2^27 rows * 65535 < 2^43);
 *   cnt == 0  out[t] = the merged value of the distinct source point f(t): the
 *             same rounded mean over its run of duplicate rows;
 *   a frame without a source (f(t) = -1): out[t] = 0, cnt = 0.
 * The sums are integers, so the result does not depend on the order in which
 * they are formed: it is the same from run to run.
 *
 *   pcc_attr_transfer_frames : runs no search; both row arrays are outputs of
 *     pcc_nn_frames, so a caller that holds the pairing already (for
 *     pcc_nn_attr_sse_frames) pays for it once.  d_skeys [n_s]: the source
 *     keys, sorted, duplicates allowed; d_sruns [n_su]: the first sorted row
 *     of every distinct source point (pcc_unique_rows), a run ending where the
 *     next begins, the last at n_s; d_svalues [n_s][channels]: the values in
 *     the order of d_skeys, bpv = 1 (uint8) or 2 (uint16) bytes each;
 *     d_row_st [n_s]: pcc_nn_frames' rows of d_skeys among the n_t distinct
 *     target keys; d_row_ts [n_t]: its rows of the target keys among the n_su
 *     distinct source keys.  Rows are counted over the whole call, as
 *     pcc_nn_frames counts them, and a pairing never leaves its frame, so the
 *     frames of a call do not mix.  d_out [n_t][channels]; d_count [n_t]
 *     (nullable): cnt.
 *     Two launches on the context's stream and no synchronisation: one thread
 *     per source row adds its values to a zeroed uint64 [n_t][channels + 1]
 *     accumulator in the context's scratch (runs of equal adjacent target rows
 *     are summed inside the wave first, then one 64-bit integer atomic per
 *     channel and one for the count per run), then one thread per target
 *     forms the mean or takes the fallback.
 *     Checked (PCC_E_ARG, pcc_last_error says which): n_s, n_t <= 2^27,
 *     n_su <= n_s and 0 only with it, n_frames in 1 .. 65535, bpv 1 or 2,
 *     channels 1 .. 4, null arrays.  n_t = 0 launches nothing; n_s = 0 zeroes
 *     d_out and d_count.  Nothing read from an array indexes outside one: a
 *     d_row_st entry outside [0, n_t) or a source key whose frame index is
 *     not below n_frames adds nothing, a d_row_ts entry outside [0, n_su)
 *     gives 0, a run is cut at n_s. */
int pcc_attr_transfer_frames(pcc_ctx* ctx, const uint64_t* d_skeys, int64_t n_s,
                             const uint32_t* d_sruns, int64_t n_su,
                             const void* d_svalues, const int32_t* d_row_st,
                             const int32_t* d_row_ts, int64_t n_t, int bpv,
                             int channels, int n_frames, void* d_out,
                             uint32_t* d_count);

/* ---- attributes from where they lie on the device (csrc/attr_stage.hip) ---- */

/* The rule (tests/attr_stage_ref.py restates it in numpy).  A per-point value
 * reaches the attribute coders, pcc_nn_attr_sse_frames and
 * pcc_attr_transfer_frames as a uint8 or uint16.
 *   Integer sources (uint8, uint16) are taken as they are; a uint8 value in a
 *   uint16 destination is zero-extended.
 *   Float sources (float32, float64) are quantised with a scale s, per value:
 *     v = clamp(rint(x * s), 0, peak),  peak = 255 (uint8) or 65535 (uint16)
 *   in the source's own precision: one IEEE multiplication (__fmul_rn /
 *   __dmul_rn, nothing contracted), round-half-to-even, and the clamp on the
 *   float before it becomes an integer.  s is narrowed to float32 once for
 *   float32 sources and used as a double for float64 sources.  -0.0 and
 *   denormals give 0; a finite x whose product overflows gives 0 or peak by
 *   its sign.  A non-finite x (NaN, +-Inf) sets status bit 0 and its output is
 *   unspecified: an error for the caller (PCC_E_RANGE in GeometryCodec), as a
 *   non-finite coordinate is.  s is not written into any blob: the caller
 *   carries it, as it carries voxel.
 *
 *   pcc_attr_stage_frames : one launch on the context's stream, one thread per
 *     row, no synchronisation, no scratch.  Per frame one record: d_src, the
 *     first value of the frame's first row on the device; kind, what a value
 *     is; channels c_f in 1 .. 4; pitch >= c_f, the distance of two rows in
 *     ELEMENTS (a [:, 4:7] view of an interleaved array needs no copy);
 *     out_offset (packed mode).  The records and the n_frames + 1 row offsets
 *     (frame f = rows [offs[f], offs[f + 1]) of the call, offs[0] = 0) are
 *     given twice, as the host arrays that are checked and as the copies on
 *     the device that the kernel reads: a caller uploads both in one piece.
 *     Two modes:
 *       packed (channels == 0, d_perm NULL): frame f's rows tight as
 *         [rows_f][c_f] at byte out_offset[f] of d_out — 16-aligned and
 *         ascending, the d_values / h_value_offsets layout of
 *         pcc_attr_encode_frames and its siblings.  An integer source keeps
 *         its width, a float source gets bpv bytes per value.  Bytes between
 *         two frames are not written.
 *       sorted (channels 2 or 4 with bpv * channels == 4 or 8): d_out
 *         [n][channels] of bpv bytes per value; row i is source row d_perm[i]
 *         of the call, widened, channels c_f and above 0 — what
 *         pcc_nn_attr_sse_frames and pcc_attr_transfer_frames take, in place of
 *         a widening on the host, an upload and pcc_gather_rows.  A d_perm
 *         entry >= n reads nothing, writes a zero row and sets status bit 1.
 *     d_status: one int32 on the device, zeroed by the caller, OR-ed into.
 *     Checked (PCC_E_ARG, pcc_last_error says which, nothing launched): null
 *     arrays, n_frames outside 1 .. 65535, 2^27 rows or more, descending row
 *     offsets, a bad kind, a channel count outside 1 .. 4 (sorted: above
 *     channels), a pitch below c_f, a source not aligned to its elements, a
 *     uint16 source into uint8 rows (sorted), value offsets that are not
 *     16-aligned or overlap, more output than out_bytes, a d_out that is not
 *     16-aligned, and a non-finite or non-positive scale when a float source
 *     is present.  n == 0 launches nothing. */
#define PCC_ATTR_SRC_U8 0
#define PCC_ATTR_SRC_U16 1
#define PCC_ATTR_SRC_F32 2
#define PCC_ATTR_SRC_F64 3
typedef struct pcc_attr_stage_frame {
  const void* d_src;
  int64_t pitch;      /* elements between two rows, >= channels */
  int64_t out_offset; /* packed mode: the frame's first byte in d_out */
  int32_t kind;       /* PCC_ATTR_SRC_* */
  int32_t channels;   /* 1 .. 4 */
} pcc_attr_stage_frame; /* 32 bytes */
int pcc_attr_stage_frames(pcc_ctx* ctx, const pcc_attr_stage_frame* h_frames,
                          const pcc_attr_stage_frame* d_frames,
                          const int64_t* h_row_offsets,
                          const int64_t* d_row_offsets, int n_frames,
                          double scale, int bpv, int channels,
                          const uint32_t* d_perm, void* d_out,
                          int64_t out_bytes, int32_t* d_status);

/* ---- whole-GOP entry points ------------------------------ */

/* replaces: CompressionPipeline.compress() (sender/encoder/codec_pipeline.py:
 * 196-236, called from sender/encoder/encoder.py:139) and
 * DecompressionPipeline.decompress() (receiver/decoder/codec_parallel.py:141-171,
 * called from receiver/decoder/decoder.py:62) for one GOP, in native code: the
 * op-level entry points above driven in the reference's stage order.  The
 * containers are byte-identical to those of the Python mirror of the pipelines
 * (codec_pipeline.py / codec_parallel.py of this package), which drives the same
 * entry points one by one.
 *
 * A codec = model weights in HBM + one ctx (stream, scratch) + a device pool
 * for the tensors of one call + pinned staging: one codec per in-flight call
 * (the reference runs up to 3, sender/encoder/encoder.py:50).  Results (output
 * containers, reconstructed cloud) are owned by the codec and stay valid until
 * the next call on it.
 *
 * h_ckpt: "PCCW" blob = u32 count, then per tensor { u16 name_len, name, u8 dtype
 * (0 float32, 1 int32), u8 ndim, u32 dims[], u64 nbytes, pad to 8, data, pad to
 * 8 }, little-endian — the tensors of assets/demo_small.npz (DESIGN.md MODEL);
 * native.pack_checkpoint() writes it. */
typedef struct pcc_codec pcc_codec;
typedef struct pcc_buf {
  const uint8_t* data;
  int64_t len;
} pcc_buf;
typedef struct pcc_cloud_info {
  int64_t n_points;
  int32_t n_frames;         /* frames the container announces                      */
  int32_t n_offsets;        /* entries of h_offsets = frames with points, plus one */
  const int64_t* h_offsets; /* row range of every frame in d_coords / d_colors     */
  const int32_t* d_coords;  /* [n_points,4] rows (b,x,y,z), Morton order per frame */
  const float* d_colors;    /* [n_points,3] as the colour head leaves them         */
  double q_g, q_a;          /* quality setting read from the container             */
} pcc_cloud_info;

pcc_codec* pcc_codec_create(const void* h_ckpt, size_t n, int device, void* stream);
void pcc_codec_destroy(pcc_codec* codec);
pcc_ctx* pcc_codec_ctx(pcc_codec* codec); /* the codec's ctx (stream, profiler) */

/* Container version the encoder entry points of this codec write (default 0).
 *   PCC_CONTAINER_V0  the reference's layout, byte for byte (make_bitstream_batched,
 *                     codec_pipeline.py:464-517): y and z strings are single rANS
 *                     streams, coded on the host (CompressAI's format)
 *   PCC_CONTAINER_V1  the same fields, the top byte of the first word (num_frames,
 *                     at most 65535) set to 1, and the y / z strings in the GPU
 *                     coder's wave-interleaved form (pcc_rans_encode_dev): no serial
 *                     host coder on the path.  The reference's decoder cannot read
 *                     it; pcc_decode_gop reads both versions. */
#define PCC_CONTAINER_V0 0
#define PCC_CONTAINER_V1 1
int pcc_codec_set_container_version(pcc_codec* codec, int version);
/* Seek points of the host-coded y strings (round 4).  pieces > 1: a version-0 container written by this codec carries,
 * BEHIND its last frame record, the trailer "PCSK" | int32 count | count x (int32 symbol index | uint64 coder state |
 * int32 32-bit words consumed) — where a decoder of the y string stands at `pieces` - 1 cuts of the symbol array
 * (multiples of 64 near k n / pieces; none for strings under 65536 symbols).  Everything in front of the trailer is
 * the reference's container byte for byte, and the reference's reader never reaches the trailer: it reads exactly
 * num_frames frame records (receiver/decoder/codec_parallel.py:200-213).  pcc_decode_gop* decodes the pieces between
 * the points on as many host threads, checks every piece's end against the next point and falls back to the serial
 * decode when a trailer does not parse or check out (a container without one is decoded serially as before).
 * 0 (default): no trailer. */
int pcc_codec_set_seek_points(pcc_codec* codec, int pieces);

/* d_coords int32 [n,4] rows (b,x,y,z), b in [0,n_frames); d_feats float32 [n,4]
 * = (1,r,g,b) (codec_pipeline.py:258); h_q [n_q,2] = (q_g,q_a) per quality
 * (shared/config.yaml:12-15).  h_out receives n_q containers; h_k (nullable)
 * int64 [3,n_frames] = k[scale][frame]; h_stage_s (nullable) double[7] seconds =
 * analysis, hyper_analysis, factorized_model, hyper_synthesis,
 * geometry_compression, gaussian_model, bitstream_writing.
 * Errors: PCC_E_RANGE / PCC_E_DUP for bad coordinates, like the SparseTensor
 * constructor of the Python mirror. */
int pcc_encode_gop(pcc_codec* codec, const int32_t* d_coords,
                   const float* d_feats, int64_t n, int n_frames,
                   const double* h_q, int n_q, pcc_buf* h_out, int64_t* h_k,
                   double* h_stage_s);
/* The same call on the frames as the capture stage produces them
 * (sender/capturer/capturer.py:111-126; consumed by unpack_batch,
 * codec_pipeline.py:243-262, and utils.stack_tensors, shared/utils.py:10-42):
 * per frame f, h_d_points[f] = device array [h_n[f],3] of int16 (points_i16 != 0)
 * or int32 voxel coordinates, h_d_colors[f] = device array [h_n[f],3] of float64
 * (colors_f64 != 0) or float32 colours in [0,1].  The batch column, the casts and
 * the (1,r,g,b) rows are formed inside the key and gather kernels; at most 32
 * frames per call (more: concatenate and use pcc_encode_gop).  The h_* tables are
 * host arrays of n_frames entries.  Same outputs and errors as pcc_encode_gop. */
int pcc_encode_gop_frames(pcc_codec* codec, const void* const* h_d_points,
                          int points_i16, const void* const* h_d_colors,
                          int colors_f64, const int64_t* h_n, int n_frames,
                          const double* h_q, int n_q, pcc_buf* h_out,
                          int64_t* h_k, double* h_stage_s);
/* The same with the frame arrays still in HOST memory, as compress(gop) receives
 * them from the capturer over ZeroMQ (codec_pipeline.py:243-262): h_points[f] /
 * h_colors[f] are host arrays.  The library uploads them itself and overlaps the
 * two PCIe legs with the start of the path: the points go up first, the Morton
 * keys and their sort run while the (4x larger, float64) colours follow. */
int pcc_encode_gop_host_frames(pcc_codec* codec, const void* const* h_points,
                               int points_i16, const void* const* h_colors,
                               int colors_f64, const int64_t* h_n, int n_frames,
                               const double* h_q, int n_q, pcc_buf* h_out,
                               int64_t* h_k, double* h_stage_s);
/* h_stage_s (nullable) double[6] seconds = bitstream_reading,
 * geometry_decompression, factorized_model, hyper_synthesis, guassian_model,
 * synthesis_transform.  Truncated / inconsistent containers: PCC_E_STREAM. */
int pcc_decode_gop(pcc_codec* codec, const uint8_t* h_in, int64_t len,
                   pcc_cloud_info* h_info, double* h_stage_s);
/* copy the cloud of the last pcc_decode_gop into caller-owned device buffers
 * (int32 [n_points,4], float32 [n_points,3]; either may be NULL); returns when
 * the copies are complete */
int pcc_decode_fetch(pcc_codec* codec, int32_t* d_coords, float* d_colors);
/* the same cloud as pack_batches returns it (codec_parallel.py:474-502):
 * points int32 [n_points,3] (no batch column; frame i = rows h_offsets[i] ..
 * h_offsets[i+1]), colours float32 [n_points,3] with NaN -> 0 and
 * clip(c * 255, 0, 255) / 255 applied on the device.  The destinations may be
 * device or host buffers (hipMemcpyDefault); returns when they are filled. */
int pcc_decode_fetch_packed(pcc_codec* codec, int32_t* points, float* colors);
/* decompress() into the caller's arrays in one call (codec_parallel.py:141-171 +
 * pack_batches 474-502): pcc_decode_gop with pcc_decode_fetch_packed's kernel
 * and transfers queued behind the last layer — no synchronisation and no trip
 * through the caller between the two.  points / colors hold cap_points rows
 * (host or device memory); pcc_container_points gives the number of points a
 * container announces (sum over frames of its finest k, an upper bound of what
 * is decoded; host-only parse, nothing beyond the slot bounds is validated).
 * More points decoded than cap_points: PCC_E_ARG, nothing is written.  Any
 * other error (PCC_E_STREAM from a malformed version-1 stream is only known when
 * the GPU coder's status word comes back, after the transfers were queued):
 * the contents of points / colors are undefined. */
int pcc_container_points(const uint8_t* h_in, int64_t len, int64_t* h_n_points,
                         int32_t* h_n_frames);
int pcc_decode_gop_packed(pcc_codec* codec, const uint8_t* h_in, int64_t len,
                          int32_t* points, float* colors, int64_t cap_points,
                          pcc_cloud_info* h_info, double* h_stage_s);

/* ---- capture pre-step ------------------------------- */

/* replaces: the voxelisation the capturer does per camera frame with numpy +
 * Open3D (sender/capturer/capturer.py:88-126).  Input: ZED XYZRGBA float32
 * [m,4] (colour packed in the 4th float, r = bits 0-7, g = 8-15, b = 16-23).
 *  pcc_vox_valid : valid[i] = finite && norm <= depth_clip; returns the
 *                  per-axis minimum of the valid points and their number
 *  pcc_vox_keys  : Open3D voxel index of every valid point packed as
 *                  ix<<42|iy<<21|iz (all ones for invalid points); d_flag is
 *                  OR-ed with 1 if an index does not fit 21 bits
 *  pcc_vox_mean  : on keys sorted with pcc_sort_pairs (d_perm = its permutation,
 *                  first n_valid entries): per voxel, mean position / colour in
 *                  double (input order) -> integer voxel rint(mean/voxel_size)
 *                  as rows (0,x,y,z) and float64 colours in [0,1]
 *  pcc_unique_rows: indices of the first row of every run of equal rows in an
 *                  array sorted so that duplicates are adjacent */
int pcc_vox_valid(pcc_ctx* ctx, const float* d_xyzrgba, int64_t m,
                  float depth_clip, uint8_t* d_valid, float* h_min_bound,
                  int64_t* h_n_valid);
int pcc_vox_keys(pcc_ctx* ctx, const float* d_xyzrgba, const uint8_t* d_valid,
                 int64_t m, const double* h_voxel_min_bound, double voxel_size,
                 uint64_t* d_keys, int32_t* d_flag);
int pcc_vox_mean(pcc_ctx* ctx, const float* d_xyzrgba,
                 const uint64_t* d_sorted_keys, const uint32_t* d_perm,
                 int64_t n_valid, double voxel_size, int32_t* d_out_coords,
                 double* d_out_colors, int64_t cap, int64_t* h_n_voxels);
int pcc_unique_rows(pcc_ctx* ctx, const int32_t* d_sorted_coords, int64_t n,
                    uint32_t* d_rows, int64_t* h_n_unique);

#ifdef __cplusplus
}
#endif
#endif /* PCC_H */
