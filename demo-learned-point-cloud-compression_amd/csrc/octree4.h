// octree4.h — what the batched coder of octree2.hip asks of octree4.hip when it writes predicted frames (octree blob
// version 4; include/pcc.h has the rule, octree4_blob.h the header's parser).
#pragma once
#include <stddef.h>
#include <stdint.h>

struct pcc_ctx;

// nodes per lane of a version-4 blob (the decoder reads S from the header and accepts what version 2's accepts): a
// level's launch of the decoder lasts up to 8 S dependent steps of a wave
constexpr int kO4SMax = 256;

// the reference of a predicted frame of an encode call: ref_n >= 1 keys on the device, strictly increasing under the
// key shift — the frame in front of it among the call's keys, or the union of its window (o4_merge_async)
struct O4Pred {
  const uint64_t* ref_keys;
  int64_t ref_n;
};

// one predicted frame whose nodes want their reference bytes: its occupancy bytes (root first) at occ + occ_off, level
// L = nodes [off[L], off[L + 1]) (off[depth] = all nodes), its root cube, its reference's keys
struct O4RefJob {
  int64_t occ_off, n_points;
  int64_t rb_off;          // where the job's reference bytes go: occ_off, unless several jobs share the tree
  int64_t off[17];
  const uint64_t* ref_keys;
  int64_t ref_n;
  int32_t depth;
  int32_t origin[3];
};

// scratch of a frame of n_nodes nodes and n_points leaves
size_t o4_ref_scratch_bytes(int64_t n_nodes, int64_t n_points);
// rb + rb_off receives the reference byte of every node of every job, ref_n[f] / ref_sum[f] what identifies job f's
// reference.  Queued on the context's stream; the jobs take `scratch` (the largest job's bytes) in turn, and a job
// behind one of the same tree (the same occ_off) finds the tree's links there.
int o4_ref_bytes_async(pcc_ctx* ctx, int key_shift, const O4RefJob* jobs, int nf, const uint8_t* occ,
                       uint8_t* rb, uint32_t* ref_n, unsigned long long* ref_sum, char* scratch, size_t scratch_b);

// ---- the merged reference of a window of more than one frame (history > 1; include/pcc.h has the rule) ---------------
constexpr int kO4MaxWindow = 8;

// one union: up to 8 lists of keys on the device, each strictly increasing under (key & mask48) >> key_shift -> out,
// the strictly increasing union (of equal keys the one of the first list that holds it), room for all lists' keys
struct O4MergeJob {
  const uint64_t* list[kO4MaxWindow];
  int64_t n[kO4MaxWindow];
  int32_t nl;
  uint64_t* out;
};
// the job as the kernels read it: list i = elements [off[i], off[i + 1]) of the job, the job's elements from `base`
// on among the call's
struct O4MergeDev {
  const uint64_t* list[kO4MaxWindow];
  int64_t off[kO4MaxWindow + 1];
  int64_t base;
  uint64_t* out;
  int32_t nl;
};
// device scratch of a call whose jobs hold `total` keys in all (total >= 1, total + 1 < 2^31)
size_t o4_merge_scratch_bytes(int64_t total, int nj);
// All jobs in three steps queued on the context's stream, whatever their number: keep flags, one scan, scatter.
// *d_counts (in the scratch) receives the size of every union.  h_tab[nj] is the table on its way to the device: the
// caller keeps it until its next synchronisation.  RESERVES THE ARENA (the scan's block sums): the caller holds
// nothing in it.
int o4_merge_async(pcc_ctx* ctx, const O4MergeJob* jobs, int nj, int key_shift, char* scratch, size_t scratch_b,
                   O4MergeDev* h_tab, uint32_t** d_counts);

// ---- the nested unions of a frame's windows (pcc_octree_encode_frames_inter_best) ------------------------------------
// The lists of a job NEWEST FIRST: list i is the frame i + 1 in front of the coded one, and union W (1 .. nl) is the
// union of lists 0 .. W - 1.  One pass forms them all: a key is kept where no newer list holds an equal one (the keep
// flags and their scan are the merge's), and a kept key of list i goes into every union W > i, at the kept keys below
// it in lists 0 .. W - 1.  out[W - 1] (nullptr: union W is not wanted — union 1 is list 0 itself) has room for the
// keys of lists 0 .. W - 1.
struct O4NestJob {
  const uint64_t* list[kO4MaxWindow];
  int64_t n[kO4MaxWindow];
  int32_t nl;
  uint64_t* out[kO4MaxWindow];
};
struct O4NestOut {
  uint64_t* out[kO4MaxWindow];
};
// device scratch of a call whose jobs hold `total` keys in all (total >= 1, total + 1 < 2^31)
size_t o4_nest_scratch_bytes(int64_t total, int nj);
// All jobs in three steps queued on the context's stream.  (*d_counts)[kO4MaxWindow * j + W - 1] (in the scratch)
// receives the size of union W of job j, wanted or not.  h_tab[nj] and h_out[nj] are on their way to the device: the
// caller keeps them until its next synchronisation.  RESERVES THE ARENA, as o4_merge_async does.
int o4_nest_async(pcc_ctx* ctx, const O4NestJob* jobs, int nj, int key_shift, char* scratch, size_t scratch_b, O4MergeDev* h_tab,
                  O4NestOut* h_out, uint32_t** d_counts);
