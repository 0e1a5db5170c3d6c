// octree4.h — what the batched coder of octree2.hip asks of octree4.hip when it writes predicted frames (octree blob
// version 4; include/pcc.h has the rule, octree4_blob.h the header's parser).
#pragma once
#include <stddef.h>
#include <stdint.h>

struct pcc_ctx;

// nodes per lane of a version-4 blob (the decoder reads S from the header and accepts what version 2's accepts): a
// level's launch of the decoder lasts up to 8 S dependent steps of a wave
constexpr int kO4SMax = 256;

// the reference of a predicted frame of an encode call: the keys d_keys[ref_lo, ref_lo + ref_n) (ref_n >= 1)
struct O4Pred {
  int64_t ref_lo, ref_n;
};

// one predicted frame whose nodes want their reference bytes: its occupancy bytes (root first) at occ + occ_off, level
// L = nodes [off[L], off[L + 1]) (off[depth] = all nodes), its root cube, its reference's keys
struct O4RefJob {
  int64_t occ_off, n_points;
  int64_t off[17];
  int64_t ref_lo, ref_n;
  int32_t depth;
  int32_t origin[3];
};

// scratch of a frame of n_nodes nodes and n_points leaves
size_t o4_ref_scratch_bytes(int64_t n_nodes, int64_t n_points);
// rb + occ_off receives the reference byte of every node of every job, ref_n[f] / ref_sum[f] what identifies job f's
// reference.  Queued on the context's stream; the jobs take `scratch` (the largest job's bytes) in turn.
int o4_ref_bytes_async(pcc_ctx* ctx, const uint64_t* d_keys, int key_shift, const O4RefJob* jobs, int nf, const uint8_t* occ,
                       uint8_t* rb, uint32_t* ref_n, unsigned long long* ref_sum, char* scratch, size_t scratch_b);
