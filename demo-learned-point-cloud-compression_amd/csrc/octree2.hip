// octree2.hip — blob version 2 of the geometry slot: the octree occupancy ENTROPY coder on the GPU.
//
// Replaces, for point sets above PCC_OCTREE_V2_MIN_LEAVES leaves, the serial host coder of blob version 1
// (octree_host.cpp) behind utils.gpcc_encode / gpcc_decode (shared/utils.py:169-240; tmc3 in the reference): rounds
// 1-3 formed the occupancy bytes on the GPU and coded them in one adaptive binary rANS stream on a host core — two
// 64-bit divisions per decision, 9.4 ms to code and 4.6 ms to decode BASELINE.json configs[2] (a 104k-point LiDAR
// sweep: 197k nodes, 1.5M decisions).  Version 2 keeps that model — context = (level class, bit position, ones so
// far), 12-bit probabilities, adaptation shift 4 — and deals the nodes (breadth-first, root first) in runs of S
// consecutive nodes to the 64 lanes of chunks, one wave per chunk, each lane with its own 32-bit rANS state (L = 2^16,
// 16-bit words) and its own copy of the model in LDS:
//
//   'O' 2 depth 0 | u32 n | i32 origin[3] | u32 payload_len |
//   u32 level_n[depth] | u32 S | u32 n_chunks | u16 p0[108] | u32 words[n_chunks] | chunk payloads (16-bit words)
//   chunk c, lane l : nodes [(64 c + l) S, (64 c + l + 1) S) below n_nodes = sum(level_n)
//   step t = 8 s + j: every lane codes bit j of its node s (nothing when the node does not exist or the bit is
//                     implied: j == 7 behind seven zeros)
//   payload         = 64 x (state lo, state hi) | u16 len[64] | words of lane 0 | words of lane 1 | ..: every lane has
//                     its own run of 16-bit renormalisation words, in the order its decoder consumes them
//
// (The first form of this round shared one word sequence per chunk — blocks per step, a lane's place by ballot + mbcnt,
// as the y / z coder of container version 1 does: 0.92 / 1.04 ms per coder launch for the sweep, i.e. ~0.25 us per
// step: a lone wave issues one instruction every ~5 cycles whether or not it depends on the one before, and a step was
// ~100 instructions — the refill's ballot, two ds_bpermute and window bookkeeping, a 64-bit-float division per
// decision in the encoder.  Per-lane runs need none of that: a refill is a shift and an LDS read of the lane's own next
// word, the division a lookup of 2^32 / freq in a 16-KB LDS table; 128 B of length table per chunk: +0.9 % bytes.
// With steps free of divergent branches and the encoder's records as 16-byte pieces per node: 0.53 / 0.52 ms to code /
// decode the sweep, blob on the host <-> keys / points in HBM; DESIGN.md 6c has the steps.)
//
// A lane's model starts from the frame's average probability per context (p0: a counting pass, 216 B of header)
// instead of 1/2, so that a run of 512 nodes does not pay for learning it again: +3.6 % bytes against version 1 on
// the sweep (1.5 % the 4-byte final states, 0.9 % the run lengths), +4.3 % on a 1M-point room.  The node count of every level
// is in the header because a decoder lane needs the level class of a node before the levels above it are decoded;
// with them ALL nodes decode in one launch, and the leaves follow from ONE exclusive scan of the nodes' child counts
// (breadth-first numbering: the first child of node i is node 1 + sum of the child counts in front of i), a pass that
// writes every child's (parent, octant) link and a pass in which every leaf walks up `depth` links.
// All integer: bit-exact against oracle/pcc_oracle.c (orc_octree2_encode / orc_octree_decode).
//
// Levels of detail (the header's parser and the rule in full: octree2_blob.h).  Breadth-first numbering, the chunk table
// in front of the payload and a contiguous run of words per lane make the levels above a cut a PREFIX of the bytes, and
// the nodes of level L are indexed exactly where the leaves of a tree of depth L would be.  For lod k in 0 .. 15:
// Lc = max(depth - k, 0); cells m = n (k = 0), level_n[Lc] (0 < k < depth), 1 (k >= depth); nodes needed
// N' = level_n[0] + .. + level_n[Lc - 1]; result = the m distinct cell indices p >> k in Morton order (corner c << k,
// centre (c << k) + ((1 << k) >> 1)); shortest prefix = the whole blob (k = 0), off_payload (N' = 0), else with
// lanes = ceil(N' / S), c* = (lanes - 1) / 64, l* = (lanes - 1) % 64:
// off_payload + 2 (words[0] + .. + words[c* - 1]) + 2 (192 + len[0] + .. + len[l*]) of chunk c*'s length table.
// The decoder below is one path for all k: the tree with depth := Lc, n_nodes := N', n_points := m, origin >> k.
#include "common.h"
#include "lanerans.h"
#include "octree2_blob.h"
#include "octree4.h"
#include "octree4_blob.h"
#include "octree_best_host.h"

#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

void octree_root(uint64_t first, uint64_t last, int key_shift, int* depth, int32_t origin[3]);

namespace {

constexpr int kCtx = kO2Ctx;      // 3 level classes x 36 (bit position, ones so far)
constexpr int kSMax = kO2SMax;     // nodes per lane: a launch lasts 8 S dependent steps of one wave
constexpr int kHeader = kO2Header;
constexpr uint32_t kL = 1u << 16;

__device__ __forceinline__ int lane_rank(unsigned long long bal) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

struct O2Layout {
  int64_t S, nc;
};
static O2Layout o2_layout(int64_t n_nodes, int64_t s_max = kSMax) {
  int64_t c = (n_nodes + (int64_t)kLanes * s_max - 1) / ((int64_t)kLanes * s_max);
  if (c < 1) c = 1;
  int64_t s = (n_nodes + kLanes * c - 1) / (kLanes * c);
  s = (s + 3) / 4 * 4;
  if (s < 4) s = 4;
  return O2Layout{s, c};
}

// ---- encoder -----------------------------------------------------------------------------------------------------
// one frame (>= 1 leaf) of an encode call
struct O2Frame {
  int64_t occ_off;                     // its occupancy bytes (4-aligned) in the call's node array
  int64_t n_nodes, start_last, start_prev;
  int64_t rec_off;                     // 16-bit words of records (and of word regions) of the frames in front of it
  int64_t out_off, out_cap;            // its blob in the output staging: offset, bound
  int32_t S, nc, cb, sb, sn;           // chunks: S, count, first (of the call); stats blocks: first, count
  int32_t depth;
  uint32_t n_points;
  int32_t origin[3];
  // A frame of the table is a CODING JOB over a tree, and several jobs may share one (the candidates of a frame under
  // pcc_octree_encode_frames_inter_best, each against another reference): `tree` is where the call's level counts hold
  // the tree's, rb_off where the job's own reference bytes lie (version 4).  One job per tree: tree = the job, rb_off =
  // occ_off.
  int32_t tree;
  int64_t rb_off;
};

// What version 4 (a predicted frame: octree4.hip, include/pcc.h) adds to the coder's three kernels, REF = true: the
// reference byte of every node beside its occupancy byte (same offsets), which splits every context in three, and what
// identifies the reference in the header.  REF = false is version 2 and reads none of it.
struct O2Ref {
  const uint8_t* rb;
  const uint32_t* ref_n;               // per frame of the call
  const unsigned long long* ref_sum;
};
// r of decision j: 0 = the reference byte is 0, 1 = it is not and its bit j is 0, 2 = its bit j is 1
__device__ __forceinline__ int o4_r(uint32_t rbyte, int j) { return rbyte == 0u ? 0 : 1 + (int)((rbyte >> j) & 1u); }

// zeros and ones seen per context over the whole frame: cnt[2 KC f + 2 ctx + bit] (KC = 108, or 324 with REF); frame f
// takes blocks [sb, sb + sn)
template <bool REF>
__global__ __launch_bounds__(256) void k_o2_stats(const uint8_t* __restrict__ occ_all, const O2Frame* __restrict__ tab, int nf,
                                                  uint32_t* __restrict__ cnt_all, O2Ref ref) {
  constexpr int kCtx = REF ? 3 * kO2Ctx : kO2Ctx;
  __shared__ uint32_t s_cnt[2 * kCtx];
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].sb; });
  const uint8_t* occ = occ_all + tab[f].occ_off;
  const int64_t n_nodes = tab[f].n_nodes, start_last = tab[f].start_last, start_prev = tab[f].start_prev;
  const int64_t b = (int64_t)blockIdx.x - tab[f].sb, nb = tab[f].sn;
  uint32_t* cnt = cnt_all + 2 * kCtx * (int64_t)f;
  for (int i = threadIdx.x; i < 2 * kCtx; i += blockDim.x) s_cnt[i] = 0u;
  __syncthreads();
  for (int64_t node = b * blockDim.x + threadIdx.x; node < n_nodes; node += nb * blockDim.x) {
    const uint32_t byte = occ[node];
    uint32_t rbyte = 0;
    if constexpr (REF) rbyte = ref.rb[tab[f].rb_off + node];
    const int cls = node >= start_last ? 0 : (node >= start_prev ? 1 : 2);
    int ones = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t bit = (byte >> j) & 1u;
      const int r108 = REF ? 108 * o4_r(rbyte, j) : 0;
      if (!(j == 7 && ones == 0)) atomicAdd(&s_cnt[2 * (r108 + cls * 36 + j * (j + 1) / 2 + ones) + bit], 1u);
      ones += (int)bit;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * kCtx; i += blockDim.x)
    if (s_cnt[i]) atomicAdd(&cnt[i], s_cnt[i]);
}

// One wave per chunk.  Forward pass: every lane walks its S nodes with its own model and leaves one record per step
// (probability of a one | bit << 15, 0 = nothing coded) in rec[chunk][step][lane]; backward pass: the lane's rANS steps
// in reverse, every renormalisation word stored downwards from the end of the lane's own T-word region of `work`
// ([chunk][lane][T]: a step emits at most one word).  states[chunk][128] and lens[chunk][64] receive the final states
// and the word counts; words_out[chunk] = 192 + sum of the counts.  Every global access of the coding loop is
// unconditional (rans_gpu.hip's rule).  Block = chunk of the call: frame f owns blocks [cb, cb + nc); its records and
// word regions start rec_off words in, states / lens / words_out are indexed by the call's chunk.
template <bool REF>
__global__ __launch_bounds__(64) void k_o2_enc(const uint8_t* __restrict__ occ_all, const O2Frame* __restrict__ tab, int nf,
                                               const uint32_t* __restrict__ cnt_all, uint16_t* __restrict__ rec_all,
                                               uint16_t* __restrict__ work_all, uint16_t* __restrict__ states,
                                               uint16_t* __restrict__ lens, uint32_t* __restrict__ words_out,
                                               uint16_t* __restrict__ p0_all, O2Ref ref) {
  constexpr int kCtx = REF ? 3 * kO2Ctx : kO2Ctx;
  __shared__ uint16_t s_model[(kCtx + 1) * kLanes];   // [ctx][lane]; row kCtx takes the writes of decisions that are not coded
  __shared__ uint16_t s_p0[kCtx];
  __shared__ __attribute__((aligned(16))) uint32_t s_rcp[4096];
  const int lane = threadIdx.x;
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].cb; });
  const int64_t cg = blockIdx.x, c = cg - tab[f].cb;
  const uint32_t* occ32 = reinterpret_cast<const uint32_t*>(occ_all + tab[f].occ_off);
  const int64_t n_nodes = tab[f].n_nodes, start_last = tab[f].start_last, start_prev = tab[f].start_prev;
  const int S = tab[f].S;
  const uint32_t* cnt = cnt_all + 2 * kCtx * (int64_t)f;
  uint16_t* p0_out = p0_all + kCtx * (int64_t)f;
  uint16_t* rec = rec_all + tab[f].rec_off;
  uint16_t* work = work_all + tab[f].rec_off;
  for (int ctx = lane; ctx < kCtx; ctx += kLanes) {
    const uint32_t p = o2_p0(cnt[2 * ctx], cnt[2 * ctx + 1]);
    s_p0[ctx] = (uint16_t)p;
    if (c == 0) p0_out[ctx] = (uint16_t)p;
  }
  lr_load_rcp(s_rcp, lane);
  __syncthreads();
  for (int ctx = 0; ctx < kCtx; ++ctx) s_model[ctx * kLanes + lane] = s_p0[ctx];
  const int64_t T = 8 * (int64_t)S;
  // records: one 16-byte piece per (node, lane) — the node's 8 decisions —, [chunk][node][lane]: the forward pass stores
  // one dwordx4 per node, the backward pass requests a node's piece four nodes (32 steps) ahead.  (As [step][lane]
  // 16-bit entries requested 8 steps ahead the backward pass waited for every one of them: a step is ~0.1 us, a load
  // that comes from L2 ~0.8 us.)
  uint4* rec4 = reinterpret_cast<uint4*>(rec) + c * (int64_t)S * kLanes;
  const int64_t node0 = (c * kLanes + lane) * S;   // a multiple of 4: four nodes per dword
  const int64_t last_dw = (n_nodes - 1) >> 2;
  uint32_t dw_next = occ32[(node0 >> 2) < last_dw ? (node0 >> 2) : last_dw];
  const uint32_t* rb32 = nullptr;
  uint32_t rdw_next = 0;
  if constexpr (REF) {
    rb32 = reinterpret_cast<const uint32_t*>(ref.rb + tab[f].rb_off);
    rdw_next = rb32[(node0 >> 2) < last_dw ? (node0 >> 2) : last_dw];
  }
  for (int s = 0; s < S; s += 4) {
    const uint32_t dw = dw_next;
    dw_next = occ32[((node0 + s + 4) >> 2) < last_dw ? ((node0 + s + 4) >> 2) : last_dw];
    const uint32_t rdw = rdw_next;
    if constexpr (REF) rdw_next = rb32[((node0 + s + 4) >> 2) < last_dw ? ((node0 + s + 4) >> 2) : last_dw];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t node = node0 + s + q;
      const bool valid = node < n_nodes;
      const uint32_t byte = (dw >> (8 * q)) & 0xFFu;
      const uint32_t rbyte = REF ? (rdw >> (8 * q)) & 0xFFu : 0u;
      const int cls = node >= start_last ? 0 : (node >= start_prev ? 1 : 2);
      uint32_t p[8];
      int at[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r108 = REF ? 108 * o4_r(rbyte, j) : 0;
        at[j] = (r108 + cls * 36 + j * (j + 1) / 2 + __popc(byte & ((1u << j) - 1u))) * kLanes + lane;
        p[j] = s_model[at[j]];
      }
      uint32_t r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t bit = (byte >> j) & 1u;
        const bool act = valid && !(j == 7 && (byte & 0x7Fu) == 0u);
        r[j] = act ? (p[j] | (bit << 15)) : 0u;
        s_model[act ? at[j] : kCtx * kLanes + lane] = (uint16_t)o2_adapt(p[j], bit);   // no branch: a dummy row for the rest
      }
      rec4[(int64_t)(s + q) * kLanes + lane] = make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
    }
  }

  // backward pass
  uint16_t* reg_w = reinterpret_cast<uint16_t*>(uniform_u64((uint64_t)(work + c * kLanes * T)));
  const __amdgpu_buffer_rsrc_t reg_rs = __builtin_amdgcn_make_buffer_rsrc(reg_w, 0, (int)(uint32_t)(kLanes * T * 2), 0x00027000);
  int wp = (int)T;            // words [wp, T) of the lane's region are written
  const uint32_t lane_off = (uint32_t)lane * (uint32_t)T * 2u;
  uint32_t x = kL;
  constexpr int kAhead = 4;   // nodes in flight (S is a multiple of 4)
  uint4 R[kAhead];
  auto fetch = [&](int sn) -> uint4 { return rec4[(int64_t)(sn >= 0 ? sn : 0) * kLanes + lane]; };
#pragma unroll
  for (int d = 0; d < kAhead; ++d) R[d] = fetch(S - 1 - d);
  struct Prep {
    uint32_t freq, start, rcp;
    bool act;
  };
  auto prep = [&](uint32_t r) -> Prep {   // one step ahead: the LDS lookup has a whole step to arrive in
    const uint32_t p1 = r & 0xFFFu, bit = r >> 15;
    Prep q;
    q.act = r != 0u;
    q.freq = bit ? p1 : 4096u - p1;
    q.start = bit ? 4096u - p1 : 0u;
    q.rcp = s_rcp[q.freq & 4095u];
    return q;
  };
  auto rec_of = [](const uint4& v, int j) -> uint32_t {
    const uint32_t w = j < 2 ? v.x : (j < 4 ? v.y : (j < 6 ? v.z : v.w));
    return (w >> (16 * (j & 1))) & 0xFFFFu;
  };
  Prep cur = prep(rec_of(R[0], 7));
  for (int s0 = S - 1; s0 >= 0; s0 -= kAhead) {
#pragma unroll
    for (int d = 0; d < kAhead; ++d) {
      const int sn = s0 - d;
      const uint4 Rc = R[d];
      const uint4 Rn = R[(d + 1) % kAhead];   // node sn - 1 (requested earlier; for d == kAhead - 1: at the top of this round)
#pragma unroll
      for (int j = 7; j >= 0; --j) {
        const Prep nxt = j > 0 ? prep(rec_of(Rc, j - 1)) : prep(sn > 0 ? rec_of(Rn, 7) : 0u);
        const bool need = cur.act && x >= (cur.freq << 20);   // ((L >> 12) << 16) * freq; freq <= 4081
        wp -= need ? 1 : 0;
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)x, reg_rs, need ? lane_off + (uint32_t)wp * 2u : 0xFFFFFFF0u, 0, 0);
        x = need ? x >> 16 : x;
        {
          // x / freq with x < 2^20 freq: mulhi by floor(2^32 / freq) is the quotient or one less.  Selects, no branch: a
          // divergent branch costs a lone wave more than the six instructions it would skip
          const uint32_t q0 = __umulhi(x, cur.rcp);
          const uint32_t r0 = x - q0 * cur.freq;
          const bool over = r0 >= cur.freq;
          const uint32_t qd = q0 + (over ? 1u : 0u), rem = r0 - (over ? cur.freq : 0u);
          x = cur.act ? (qd << 12) + rem + cur.start : x;
        }
        cur = nxt;
      }
      R[d] = fetch(sn - kAhead);   // the slot is free: node sn - kAhead into it
    }
  }
  states[cg * 2 * kLanes + 2 * lane] = (uint16_t)x;
  states[cg * 2 * kLanes + 2 * lane + 1] = (uint16_t)(x >> 16);
  const uint32_t len = (uint32_t)((int)T - wp);
  lens[cg * kLanes + lane] = (uint16_t)len;
  uint32_t tot = len;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) tot += (uint32_t)__shfl_xor((int)tot, d, 64);
  if (lane == 0) words_out[cg] = 3u * kLanes + tot;
}

// the blobs, assembled where `out_all` points (pinned host memory: the bytes cross PCIe as the kernel writes them),
// frame f's at out_off: frame f owns workgroups [cb + f, cb + f + nc + 1) — workgroup c < nc of them moves chunk c
// (states, length table, the 64 runs), workgroup nc writes the header; len_out[f] = bytes, or -1 (out_cap)
// (REF: the header of version 4 — ref_n and ref_sum behind the chunk count, 324 initial probabilities)
template <bool REF>
__global__ __launch_bounds__(256) void k_o2_pack(const uint16_t* __restrict__ work_all, const O2Frame* __restrict__ tab, int nf,
                                                 const uint16_t* __restrict__ states_all, const uint16_t* __restrict__ lens_all,
                                                 const uint32_t* __restrict__ words_all, const uint32_t* __restrict__ counts_all,
                                                 const uint16_t* __restrict__ p0_all, uint8_t* __restrict__ out_all,
                                                 long long* __restrict__ len_out, O2Ref ref) {
  constexpr int kCtx = REF ? 3 * kO2Ctx : kO2Ctx;
  constexpr int kRefWords = REF ? 3 : 0;   // ref_n, ref_sum
  __shared__ unsigned long long s_sum[256];
  __shared__ uint32_t s_off[kLanes + 1];
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].cb + i; });
  const O2Frame& h = tab[f];
  const int64_t c = (int64_t)blockIdx.x - h.cb - f, nc = h.nc, T = 8 * (int64_t)h.S, cap = h.out_cap;
  const uint16_t* work = work_all + h.rec_off;
  const uint16_t* states = states_all + h.cb * 2 * kLanes;
  const uint16_t* lens = lens_all + h.cb * kLanes;
  const uint32_t* words = words_all + h.cb;
  const uint32_t* counts = counts_all + (int64_t)PCC_OCT_CSTRIDE * h.tree;
  const uint16_t* p0 = p0_all + kCtx * (int64_t)f;
  uint8_t* out = out_all + h.out_off;
  unsigned long long part = 0;
  const int64_t upto = c < nc ? c : nc;
  for (int64_t j = threadIdx.x; j < upto; j += blockDim.x) part += words[j];
  s_sum[threadIdx.x] = part;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
    __syncthreads();
  }
  const unsigned long long before = s_sum[0];
  const unsigned long long head = (unsigned long long)kHeader + 4ull * h.depth + 8ull + 4ull * kRefWords + 2ull * kCtx + 4ull * nc;
  if (c == nc) {
    const unsigned long long total = head + before * 2;
    const bool fits = (long long)total <= cap;
    if (threadIdx.x == 0) {
      len_out[f] = fits ? (long long)total : -1;
      __threadfence_system();
    }
    if (!fits) return;
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
    if (threadIdx.x == 0) {
      o32[0] = (uint32_t)'O' | ((REF ? 4u : 2u) << 8) | ((uint32_t)h.depth << 16);
      o32[1] = h.n_points;
      o32[2] = (uint32_t)h.origin[0];
      o32[3] = (uint32_t)h.origin[1];
      o32[4] = (uint32_t)h.origin[2];
      o32[5] = (uint32_t)(total - kHeader);
      o32[6 + h.depth] = (uint32_t)h.S;
      o32[7 + h.depth] = (uint32_t)h.nc;
      if constexpr (REF) {
        o32[8 + h.depth] = ref.ref_n[f];
        o32[9 + h.depth] = (uint32_t)ref.ref_sum[f];
        o32[10 + h.depth] = (uint32_t)(ref.ref_sum[f] >> 32);
      }
    }
    if ((int)threadIdx.x < h.depth) o32[6 + threadIdx.x] = counts[threadIdx.x];
    uint16_t* o16 = reinterpret_cast<uint16_t*>(o32 + 8 + kRefWords + h.depth);
    if constexpr (REF) {
      for (int i = threadIdx.x; i < kCtx; i += 256) o16[i] = p0[i];
    } else {
      if ((int)threadIdx.x < kCtx) o16[threadIdx.x] = p0[threadIdx.x];
    }
    uint32_t* tab = o32 + 8 + kRefWords + h.depth + kCtx / 2;
    for (int64_t j = threadIdx.x; j < nc; j += blockDim.x) tab[j] = words[j];
    return;
  }
  const uint32_t cw = words[c];
  if ((long long)(head + (before + cw) * 2) > cap) return;   // the header block reports it
  uint16_t* dst = reinterpret_cast<uint16_t*>(out + head) + before;
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

// ---- decoder -----------------------------------------------------------------------------------------------------
// status (int32): OR of 1 = a chunk ran out of words or did not use all of its words, 2 = an empty node,
// 8 = the child counts do not add up to the announced level sizes / point count; one per frame of the call
//
// one frame (>= 1 node to decode) of a decode call.  At a level of detail (octree2_blob.h) the frame is the tree cut
// at level Lc: n_nodes = N', n_points = m cells, depth = Lc, origin >> lod, nc / lanes_last / last_words what the
// prefix holds of its chunks — while the coder's parameters (S, start_last, start_prev: the level classes) and n_full
// stay the FULL tree's
struct O2DFrame {
  int64_t body_off;                    // p0 | chunk table | payload of its blob in the call's uploaded bodies (4-aligned)
  int64_t table_off, payload_off;      // from body_off
  int64_t n_nodes, start_last, start_prev, n_points;
  int64_t n_full;                      // nodes of the whole tree (n_nodes < n_full: a cut tree)
  int64_t node_base;                   // its nodes in the call's node arrays (occupancy, child counts, scan): 4-aligned
  int64_t link_base;                   // its links in the call's link array: nodes, then leaves
  int64_t pt_base;                     // its first point in the output
  int64_t off[17];                     // nodes in front of level L (off[depth] = n_nodes)
  int32_t S, nc, cb, lb, qb, depth;    // first chunk, first block of k_o2_link, of k_o2_points
  int32_t lanes_last;
  uint32_t last_words;                 // of chunk nc - 1: lanes whose runs are present, words present (whole tree: 64, all)
  int32_t origin[3];
};

// the chunk's words in LDS when they fit (a chunk is 64 S nodes: <= 32 KB of payload for S = 512 unless the stream was
// made to cost more than 8 bits per node), else read from the stream where they lie (slow, correct)
constexpr int kDecLdsWords = 24576;   // 48 KB beside the 13.9 KB of models

template <bool IN_LDS>
__device__ __forceinline__ void o2_decode_chunk(uint16_t* s_model, const uint16_t* __restrict__ s_words,
                                                const uint16_t* __restrict__ p /* the chunk in the stream */, uint32_t cw,
                                                int lanes_here, int64_t c, int lane, int64_t n_nodes, bool cut,
                                                int64_t start_last, int64_t start_prev, int S,
                                                uint32_t* __restrict__ occ32, int& bad) {
  uint32_t x = (uint32_t)p[2 * lane] | ((uint32_t)p[2 * lane + 1] << 16);
  // the lane's run: [rbase, rend) in 16-bit words from the chunk's start
  const uint32_t my_len = p[2 * kLanes + lane];
  uint32_t incl = my_len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
    incl += lane >= d ? o : 0u;
  }
  // the runs that are present (all 64 unless this is the last chunk of a cut tree) fill the words that are present
  const uint32_t total = (uint32_t)__shfl((int)incl, lanes_here - 1, 64);
  if (3u * kLanes + total != cw) {   // wave-uniform
    bad |= 1;
    return;
  }
  const uint32_t rbase = 3u * kLanes + incl - my_len, rend = rbase + my_len;
  uint32_t pos = rbase;   // next word of the run
  auto word_at = [&](uint32_t i) -> uint32_t {
    const uint32_t ic = i < cw ? i : cw - 1;   // a lane at the end of the chunk's last run looks one word too far: never used
    if constexpr (IN_LDS) return s_words[ic];
    return p[ic];
  };
  uint32_t nextw = word_at(pos);
  const int64_t node0 = (c * kLanes + lane) * S;
  // the lane's bytes leave as dwords (node0 and S are multiples of 4) through a descriptor over the node array padded
  // to a whole dword: a lane past the end stores beyond it (dropped)
  const __amdgpu_buffer_rsrc_t occ_rs = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<void*>(uniform_u64((uint64_t)occ32)), 0,
      __builtin_amdgcn_readfirstlane((int)(uint32_t)(((n_nodes + 3) >> 2) << 2)), 0x00027000);
  auto cls_of = [&](int64_t node) -> int { return node >= start_last ? 0 : (node >= start_prev ? 1 : 2); };
  // the model entry of the NEXT decision is requested before the current one is decoded — both candidates (the ones
  // so far, and one more) — so that the LDS round trip is not on the chain from state to state
  uint32_t p_cur = s_model[(cls_of(node0) * 36) * kLanes + lane];
  const int a_dummy = kCtx * kLanes + lane;   // takes the model writes of decisions that are not coded (no branch)
  // the wave's trip count is lane 0's (the lanes' runs lie one behind the other): up to the dword that holds the
  // frame's last node (a cut tree's N' - 1).  Behind that node a lane's steps code nothing and consume nothing, so the
  // lane that straddles it stops there and a lane whose run starts behind it does nothing — without a branch in the
  // steps and with a scalar loop counter, as for the whole tree
  const int64_t left = n_nodes - node0, left0 = n_nodes - c * kLanes * S;
  const int s_end = __builtin_amdgcn_readfirstlane(left0 >= (int64_t)S ? S : (left0 > 0 ? (int)((left0 + 3) & ~(int64_t)3) : 0));
  for (int s = 0; s < s_end; s += 4) {
    uint32_t dw = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t node = node0 + s + q;
      const bool valid = node < n_nodes;
      const int cbase = cls_of(node) * 36;
      int ones = 0;
      uint32_t byte = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int at = (cbase + j * (j + 1) / 2 + ones) * kLanes + lane;
        uint32_t c0, c1 = 0;
        if (j < 7) {
          const int an = (cbase + (j + 1) * (j + 2) / 2 + ones) * kLanes + lane;
          c0 = s_model[an];
          c1 = s_model[an + kLanes];
        } else {
          c0 = s_model[(cls_of(node + 1) * 36) * kLanes + lane];   // decision 0 of the next node
        }
        const bool act = valid && !(j == 7 && ones == 0);
        const uint32_t p1 = p_cur;
        const uint32_t cum = x & 4095u;
        const uint32_t dbit = cum >= 4096u - p1 ? 1u : 0u;
        const uint32_t start = dbit ? 4096u - p1 : 0u, freq = dbit ? p1 : 4096u - p1;
        const uint32_t xn = freq * (x >> 12) + cum - start;
        x = act ? xn : x;
        s_model[act ? at : a_dummy] = (uint16_t)o2_adapt(p1, dbit);
        const uint32_t bit = act ? dbit : (valid ? 1u : 0u);   // else: the implied bit
        const bool need = act && x < kL;
        bad |= (need && pos >= rend) ? 1 : 0;
        x = need ? (x << 16) | nextw : x;
        pos += need ? 1u : 0u;
        nextw = word_at(pos);   // every step (the same word again when nothing was consumed): no branch
        ones += (int)bit;
        byte |= bit << j;
        p_cur = (j < 7 && bit) ? c1 : c0;
      }
      bad |= (valid && byte == 0u) ? 2 : 0;
      dw |= byte << (8 * q);
    }
    __builtin_amdgcn_raw_buffer_store_b32(dw, occ_rs, (uint32_t)(node0 + s), 0, 0);
  }
  // every word of the run consumed — but for the lanes of a cut tree whose runs go on (or lie) behind node N' - 1
  if (pos != rend && !(cut && left < (int64_t)S)) bad |= 1;
}

// block = chunk of the call: frame f owns blocks [cb, cb + nc)
__global__ __launch_bounds__(64) void k_o2_dec(const uint8_t* __restrict__ bodies, const O2DFrame* __restrict__ tab, int nf,
                                               uint8_t* __restrict__ occ_all, int32_t* __restrict__ status_all) {
  __shared__ uint16_t s_model[(kCtx + 1) * kLanes];   // row kCtx: dummy (o2_decode_chunk)
  __shared__ __attribute__((aligned(16))) uint16_t s_words[kDecLdsWords];
  const int lane = threadIdx.x;
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].cb; });
  const int64_t c = (int64_t)blockIdx.x - tab[f].cb;
  const uint8_t* body = bodies + tab[f].body_off;
  const uint16_t* p0 = reinterpret_cast<const uint16_t*>(body);
  const uint32_t* table = reinterpret_cast<const uint32_t*>(body + tab[f].table_off);
  const uint16_t* payload = reinterpret_cast<const uint16_t*>(body + tab[f].payload_off);
  const int64_t n_nodes = tab[f].n_nodes, start_last = tab[f].start_last, start_prev = tab[f].start_prev;
  const int S = tab[f].S;
  const bool cut = n_nodes < tab[f].n_full, last = c == tab[f].nc - 1;
  const int lanes_here = last ? tab[f].lanes_last : kLanes;
  uint32_t* occ32 = reinterpret_cast<uint32_t*>(occ_all + tab[f].node_base);
  int32_t* status = status_all + f;
  for (int ctx = 0; ctx < kCtx; ++ctx) s_model[ctx * kLanes + lane] = p0[ctx];
  unsigned long long before = 0;
  for (int64_t j = lane; j < c; j += kLanes) before += table[j];
  for (int d = 32; d >= 1; d >>= 1) before += __shfl_xor(before, d, 64);
  // the words of the chunk that are here: all of them, or what a prefix holds of a cut tree's last chunk (the host
  // read them off the same length table and checked them against the chunk table: o2_parse)
  const uint32_t cw = (uint32_t)__builtin_amdgcn_readfirstlane((int)(last ? tab[f].last_words : table[c]));
  const uint16_t* p = payload + before;
  int bad = 0;
  if (cw < 3 * kLanes) {
    if (lane == 0) atomicOr(status, 1);
    return;
  }
  if (cw <= (uint32_t)kDecLdsWords) {
    // the chunk into LDS: dwords from the aligned address at or below its first word
    const int mis = (int)(((uintptr_t)p >> 1) & 1);
    const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p - mis);
    const uint32_t n_dw = (cw + (uint32_t)mis + 1u) >> 1;
    for (uint32_t i = lane; i < n_dw; i += kLanes) {
      const uint32_t v = p32[i];
      const int w0 = 2 * (int)i - mis;
      if (w0 >= 0 && w0 < (int)cw) s_words[w0] = (uint16_t)v;
      if (w0 + 1 >= 0 && w0 + 1 < (int)cw) s_words[w0 + 1] = (uint16_t)(v >> 16);
    }
    __syncthreads();
    o2_decode_chunk<true>(s_model, s_words, p, cw, lanes_here, c, lane, n_nodes, cut, start_last, start_prev, S, occ32, bad);
  } else {
    o2_decode_chunk<false>(s_model, s_words, p, cw, lanes_here, c, lane, n_nodes, cut, start_last, start_prev, S, occ32, bad);
  }
  const unsigned long long b1 = __ballot((bad & 1) != 0), b2 = __ballot((bad & 2) != 0);
  if (lane == 0 && (b1 | b2) != 0ull) atomicOr(status, (b1 ? 1 : 0) | (b2 ? 2 : 0));
}

__global__ __launch_bounds__(256) void k_o2_popc(const uint8_t* __restrict__ occ, int64_t n_nodes, uint32_t* __restrict__ pc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_nodes) pc[i] = (uint32_t)__popc((uint32_t)occ[i]);
}

// link[child] = parent << 3 | octant for every child the occupancy bytes announce (breadth-first numbering: the first
// child of node i is node 1 + excl[i], excl the exclusive scan of the child counts over the frame's nodes — the
// call's one scan minus its value at the frame's first node); the first node of every level checks that its level
// starts where the header says, node 0 checks the frame's total.  Frame f owns blocks [lb, lb + ceil(n_nodes / 256)).
__global__ __launch_bounds__(256) void k_o2_link(const uint8_t* __restrict__ occ, const uint32_t* __restrict__ excl,
                                                 const uint32_t* __restrict__ total, int64_t n_tot,
                                                 const O2DFrame* __restrict__ tab, int nf, uint32_t* __restrict__ link_all,
                                                 int32_t* __restrict__ status_all) {
  const int f = o2_find(nf, blockIdx.x, [&](int j) { return (int64_t)tab[j].lb; });
  const O2DFrame& fr = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - fr.lb) * blockDim.x + threadIdx.x, n_nodes = fr.n_nodes;
  if (i >= n_nodes) return;
  const int64_t base = fr.node_base, n_all = n_nodes + fr.n_points;
  const uint32_t e0 = excl[base];
  const uint32_t byte = occ[base + i];
  const int64_t first = 1 + (int64_t)(excl[base + i] - e0);
  int bad = 0;
  if (i == 0) {   // behind the frame's last node: its padding (no children), then the next frame or the end
    const int64_t end = base + ((n_nodes + 3) & ~(int64_t)3);
    const uint32_t ev = end < n_tot ? excl[end] : *total;
    if ((int64_t)(ev - e0) != n_all - 1) bad = 8;
  }
  for (int L = 0; L < fr.depth; ++L)
    if (i == fr.off[L] && first != fr.off[L + 1]) bad = 8;
  if (bad) atomicOr(status_all + f, bad);
  uint32_t* link = link_all + fr.link_base;
  int k = 0;
  for (int j = 0; j < 8; ++j)
    if ((byte >> j) & 1u) {
      const int64_t child = first + k;
      if (child < n_all) link[child] = ((uint32_t)i << 3) | (uint32_t)j;
      ++k;
    }
}

// every leaf walks up its `depth` links: the octants on the way are its cell inside the root cube.  Frame f owns blocks
// [qb, qb + ceil(n_points / 256)); a link holds a node of its own frame (or 0), so the walk stays inside the frame
__global__ __launch_bounds__(256) void k_o2_points(const uint32_t* __restrict__ link_all, const O2DFrame* __restrict__ tab, int nf,
                                                   int32_t* __restrict__ points_all, int32_t* __restrict__ status_all) {
  const int f = o2_find(nf, blockIdx.x, [&](int j) { return (int64_t)tab[j].qb; });
  const O2DFrame& fr = tab[f];
  const int64_t e = ((int64_t)blockIdx.x - fr.qb) * blockDim.x + threadIdx.x;
  if (e >= fr.n_points) return;
  const uint32_t* link = link_all + fr.link_base;
  const int depth = fr.depth;
  uint64_t code = 0;
  uint32_t idx = (uint32_t)(fr.n_nodes + e);
  for (int d = 0; d < depth; ++d) {
    const uint32_t l = link[idx];
    code |= (uint64_t)(l & 7u) << (3 * d);
    idx = l >> 3;
  }
  if (idx != 0u) atomicOr(status_all + f, 8);
  int32_t* points = points_all + 3 * (fr.pt_base + e);
  points[0] = (int32_t)pcc_compact3(code >> 2) + fr.origin[0];
  points[1] = (int32_t)pcc_compact3(code >> 1) + fr.origin[1];
  points[2] = (int32_t)pcc_compact3(code) + fr.origin[2];
}

// checks of the keys of an encode call (sorted, distinct after the key shift, frame index < n_frames):
// flag |= 1 duplicate, 2 out of order, 4 frame index
__global__ __launch_bounds__(256) void k_of_check(const uint64_t* __restrict__ keys, int64_t n, int shift, int n_frames,
                                                  int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = keys[i];
  int bad = (int64_t)(b >> 48) >= n_frames ? 4 : 0;
  if (i > 0) {
    const uint64_t a = keys[i - 1];
    bad |= (a >> shift) == (b >> shift) ? 1 : 0;
    bad |= a > b ? 2 : 0;
  }
  if (bad) atomicOr(flag, bad);
}

// per frame (thread f <= n_frames): offs[f] = first key of frame f (or n); ends[2 f], ends[2 f + 1] = its first and
// last key (frames with keys)
__global__ __launch_bounds__(64) void k_of_frames(const uint64_t* __restrict__ keys, int64_t n, int n_frames,
                                                  int64_t* __restrict__ offs, uint64_t* __restrict__ ends) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_frames) return;
  auto lower = [&](uint64_t target) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  const int64_t lo = lower((uint64_t)f << 48);
  offs[f] = lo;
  if (f == n_frames) return;
  const int64_t hi = lower((uint64_t)(f + 1) << 48);
  if (hi > lo) {
    ends[2 * f] = keys[lo];
    ends[2 * f + 1] = keys[hi - 1];
  }
}

}  // namespace

// pinned staging of a context, grown on demand (blobs and decoded points cross PCIe through it)
int o2_stage_reserve(pcc_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->stage_cap) return PCC_OK;
  size_t want = ctx->stage_cap ? ctx->stage_cap : ((size_t)1 << 20);
  while (want < bytes) want *= 2;
  PCC_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->stage) PCC_HIP(hipHostFree(ctx->stage));
  ctx->stage = nullptr;
  ctx->stage_cap = 0;
  PCC_HIP(hipHostMalloc(&ctx->stage, want, hipHostMallocDefault));
  ctx->stage_cap = want;
  return PCC_OK;
}

// the same with the first `keep` bytes of the staging carried over where it grows (what an earlier batch of the call
// left there)
static int o2_stage_reserve_keep(pcc_ctx* ctx, size_t bytes, size_t keep) {
  if (bytes <= ctx->stage_cap || keep == 0) return o2_stage_reserve(ctx, bytes);
  size_t want = ctx->stage_cap;
  while (want < bytes) want *= 2;
  PCC_HIP(hipStreamSynchronize(ctx->stream));
  void* grown = nullptr;
  PCC_HIP(hipHostMalloc(&grown, want, hipHostMallocDefault));
  memcpy(grown, ctx->stage, std::min(keep, ctx->stage_cap));
  (void)hipHostFree(ctx->stage);
  ctx->stage = grown;
  ctx->stage_cap = want;
  return PCC_OK;
}

// ======================================================================== entry points (internal + C-ABI)

static inline int64_t o2_round(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// the last error, prefixed with the frame it belongs to
static int o2_frame_error(int rc, const char* who, int frame) {
  const std::string m = pcc_last_error();
  pcc_set_error("%s: frame %d: %s", who, frame, m.c_str());
  return rc;
}

struct O2In {   // one frame of an encode call: leaves d_keys[lo, lo + n) (n >= 1), its root cube
  int64_t lo, n;
  int depth;
  int32_t origin[3];
};

// blobs of version 2 of the frames fr[0 .. nf): the levels of all frames (launches independent of nf), ONE
// synchronisation for all level counts (they size the chunks), the coder's three launches over all frames' chunks,
// ONE synchronisation for all blob lengths.  Blob f is left in the pinned staging at (*offs)[f], (*lens)[f] bytes.
//
// pred (version 4, octree4.hip): every frame of the batch is a predicted frame, pred[f] the keys of its reference
// (ref_n keys on the device, Morton-sorted and distinct after the key shift).  One step is added in front of the
// coder's launches: the reference byte of every node.
//
// job_tree (with pred; pcc_octree_encode_frames_inter_best): the batch holds nj CODING JOBS over the nf trees, job j a
// blob of frame job_tree[j] against pred[j] — the levels of a frame are built once and shared by its candidates, every
// job has its own reference bytes, context counts, probabilities and chunks.  offs, lens and pred are then per job.
// stage_base: the batch leaves the first stage_base bytes of the staging as they are (an earlier batch's blobs) and
// works behind them.  Without the two the batch queues what it queued before them.
static int o2_encode_batch(pcc_ctx* ctx, const uint64_t* d_keys, int key_shift, const O2In* fr, int nf,
                           std::vector<int64_t>* offs, std::vector<int64_t>* lens, const O4Pred* pred = nullptr,
                           const int* job_tree = nullptr, int n_jobs = 0, size_t stage_base = 0) {
  hipStream_t st = ctx->stream;
  const int nj = job_tree ? n_jobs : nf;
  auto tree_of = [&](int j) { return job_tree ? job_tree[j] : j; };
  PCC_REQUIRE(nj >= 1 && (!job_tree || pred), PCC_E_ARG, "octree blob v2: a batch of %d jobs", nj);
  const int KC = pred ? 3 * kCtx : kCtx;
  const int64_t s_max = pred ? kO4SMax : kSMax;
  const int64_t ref_head = pred ? 12 : 0;
  const int64_t small_max = pcc_octree_small_max();
  // levels: the frames of the single-workgroup form first, then those of the wave form
  std::vector<PccOctFrame> lt((size_t)nf);
  std::vector<int64_t> cap_of((size_t)nf);
  int ns = 0, nl = 0;
  for (int f = 0; f < nf; ++f) ns += fr[f].n <= small_max ? 1 : 0;
  int64_t occ_bytes = 0, waves = 0, leaves = 0;
  size_t coder_b = 3 * 256 + 4096, ref_b = 0, scan_b = 0;
  std::vector<size_t> coder_of((size_t)nf), scan_of((size_t)nf);
  for (int f = 0, is = 0, il = 0; f < nf; ++f) {
    const O2In& g = fr[f];
    PCC_REQUIRE(g.n >= 1 && g.depth >= 1 && g.depth <= 16 && key_shift + 3 * g.depth <= 48, PCC_E_ARG,
                "octree blob v2: frame %d: %lld leaves at depth %d", f, (long long)g.n, g.depth);
    cap_of[(size_t)f] = o2_round(g.n * g.depth, 16);
    PccOctFrame& r = lt[(size_t)(g.n <= small_max ? is++ : ns + il++)];
    r.key_lo = g.lo;
    r.n = g.n;
    r.occ_off = occ_bytes;
    r.cap = cap_of[(size_t)f];
    r.wave0 = g.n <= small_max ? -1 : waves;
    r.mask = pcc_octree_leaf_mask(g.depth);
    r.depth = g.depth;
    r.slot = f;
    if (g.n > small_max) waves += (g.n + 63) / 64;
    occ_bytes += cap_of[(size_t)f];
    leaves += g.n;
    // the coder's scratch is sized by the node counts, known after the first synchronisation, and a second reservation
    // would drop what the first holds: the arena is reserved for the node counts of surfaces and sweeps (<= 2.5 nodes
    // per leaf); a sparser batch (up to `depth` nodes per leaf) takes a block of its own for this call
    const int64_t guess = std::min<int64_t>(cap_of[(size_t)f], 5 * g.n / 2 + 64 * g.depth + 4096);
    const O2Layout l = o2_layout(guess, s_max);
    coder_of[(size_t)f] = (size_t)l.nc * (8 * l.S * kLanes * 2 * 2 + 4 + 3 * kLanes * 2);   // records, word regions, tables
    if (pred) {   // (the scans of the child counts take their block sums from the arena, frame after frame)
      ref_b = std::max(ref_b, o4_ref_scratch_bytes(guess, g.n));
      scan_of[(size_t)f] = pcc_scan_scratch_bytes(cap_of[(size_t)f]) + 512;
    }
  }
  int64_t rb_bytes = 0;   // the jobs' reference bytes, each job's as many as its tree's occupancy bytes
  std::vector<int64_t> rb_off((size_t)nj);
  for (int j = 0; j < nj; ++j) {
    const int t = tree_of(j);
    PCC_REQUIRE(t >= 0 && t < nf, PCC_E_ARG, "octree blob v2: job %d codes frame %d of %d", j, t, nf);
    coder_b += coder_of[(size_t)t];
    scan_b += scan_of[(size_t)t];
    rb_off[(size_t)j] = rb_bytes;
    rb_bytes += cap_of[(size_t)t];
  }
  nl = nf - ns;
  PCC_REQUIRE(leaves < ((int64_t)1 << 27) && occ_bytes < ((int64_t)1 << 32), PCC_E_ARG, "octree blob v2: %lld leaves in %d frames",
              (long long)leaves, nf);
  const size_t lt_b = pcc_align((size_t)nf * sizeof(PccOctFrame)), ct_b = pcc_align((size_t)nj * sizeof(O2Frame));
  const size_t counts_b = pcc_align((size_t)nf * PCC_OCT_CSTRIDE * 4);
  const size_t pred_b = pred ? pcc_align((size_t)rb_bytes + 16) + 2 * pcc_align((size_t)nj * 8) + ref_b + scan_b + 4096 : 0;
  PCC_TRY(pcc_arena_reserve(ctx, (size_t)occ_bytes + 16 + counts_b + pcc_align((size_t)nj * 2 * KC * 4) + pcc_align((size_t)nj * KC * 2) +
                                     lt_b + ct_b + pcc_octree_frames_scratch(waves, nl) + coder_b + pred_b + 16384));
  uint8_t* occ = (uint8_t*)pcc_arena_alloc(ctx, (size_t)occ_bytes + 16);
  uint32_t* counts = (uint32_t*)pcc_arena_alloc(ctx, counts_b);
  uint32_t* cnt = (uint32_t*)pcc_arena_alloc(ctx, (size_t)nj * 2 * KC * 4);
  uint16_t* p0 = (uint16_t*)pcc_arena_alloc(ctx, (size_t)nj * KC * 2);
  O2Ref ref{nullptr, nullptr, nullptr};
  if (pred) {
    ref.rb = (const uint8_t*)pcc_arena_alloc(ctx, (size_t)rb_bytes + 16);
    ref.ref_n = (const uint32_t*)pcc_arena_alloc(ctx, (size_t)nj * 4);
    ref.ref_sum = (const unsigned long long*)pcc_arena_alloc(ctx, (size_t)nj * 8);
    if (!ref.rb || !ref.ref_n || !ref.ref_sum) return PCC_E_NOMEM;
  }
  PccOctFrame* d_lt = (PccOctFrame*)pcc_arena_alloc(ctx, lt_b);
  O2Frame* d_ct = (O2Frame*)pcc_arena_alloc(ctx, ct_b);
  if (!occ || !counts || !cnt || !p0 || !d_lt || !d_ct) return PCC_E_NOMEM;
  PccProfScope prof(ctx, "octree2_encode", leaves, fr[0].depth, nf > 1 ? nf : 0, 0);
  PCC_TRY(o2_stage_reserve_keep(ctx, stage_base + lt_b + counts_b, stage_base));
  memcpy((char*)ctx->stage + stage_base, lt.data(), (size_t)nf * sizeof(PccOctFrame));
  PCC_HIP(hipMemcpyAsync(d_lt, (char*)ctx->stage + stage_base, (size_t)nf * sizeof(PccOctFrame), hipMemcpyHostToDevice, st));
  PCC_TRY(pcc_octree_frames_async(ctx, d_keys, key_shift, lt.data(), d_lt, ns, nl, occ, counts));
  uint32_t* hc = (uint32_t*)((char*)ctx->stage + stage_base + lt_b);
  PCC_HIP(hipMemcpyAsync(hc, counts, (size_t)nf * PCC_OCT_CSTRIDE * 4, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipMemsetAsync(cnt, 0, (size_t)nj * 2 * KC * 4, st));
  PCC_HIP(hipStreamSynchronize(st));
  // the coder's table from the level counts
  std::vector<uint32_t> level_counts;   // (version 4 reads them again behind the staging's next reservation)
  if (pred) level_counts.assign(hc, hc + (size_t)nf * PCC_OCT_CSTRIDE);
  std::vector<O2Frame> ct((size_t)nj);
  std::vector<int64_t> occ_of((size_t)nf);
  for (const PccOctFrame& r : lt) occ_of[(size_t)r.slot] = r.occ_off;
  int64_t rec_words = 0, out_bytes = 0, chunks = 0, stats_blocks = 0;
  for (int j = 0; j < nj; ++j) {
    const int f = tree_of(j);
    const uint32_t* c = hc + (size_t)PCC_OCT_CSTRIDE * f;
    const int depth = fr[f].depth;
    int64_t n_nodes = 0;
    for (int L = 0; L < depth; ++L) n_nodes += (int64_t)c[L];
    PCC_REQUIRE(c[0] == 1, PCC_E_ARG, "pcc_octree2_encode: keys exceed 3*depth bits (root level has %u nodes)", c[0]);
    PCC_REQUIRE(n_nodes <= cap_of[(size_t)f], PCC_E_NOMEM, "pcc_octree2_encode: %lld nodes for %lld leaves", (long long)n_nodes,
                (long long)fr[f].n);
    const O2Layout lay = o2_layout(n_nodes, s_max);
    const int64_t T = 8 * lay.S, cap_words = 3 * kLanes + kLanes * T;   // bound of a chunk in the blob
    const int64_t head = kHeader + 4 * depth + 8 + ref_head + 2 * KC + 4 * lay.nc;
    O2Frame& r = ct[(size_t)j];
    r.occ_off = occ_of[(size_t)f];
    r.tree = f;
    r.rb_off = job_tree ? rb_off[(size_t)j] : r.occ_off;
    r.n_nodes = n_nodes;
    r.start_last = n_nodes - (int64_t)c[depth - 1];
    r.start_prev = depth >= 2 ? r.start_last - (int64_t)c[depth - 2] : 0;
    r.rec_off = rec_words;
    r.out_off = out_bytes;
    // a step emits at most one word, and only for a coded decision (<= 8 per node): a frame of few nodes gets a bound
    // in proportion to them, not to its chunk's 64 x T steps
    r.out_cap = head + 2 * std::min<int64_t>(lay.nc * cap_words, 3 * kLanes * lay.nc + 8 * n_nodes);
    r.S = (int32_t)lay.S;
    r.nc = (int32_t)lay.nc;
    r.cb = (int32_t)chunks;
    r.sb = (int32_t)stats_blocks;
    r.sn = (int32_t)std::min<unsigned>(nblk(n_nodes, 256), 256u);
    r.depth = depth;
    r.n_points = (uint32_t)fr[f].n;
    for (int a = 0; a < 3; ++a) r.origin[a] = fr[f].origin[a];
    rec_words += lay.nc * T * kLanes;
    out_bytes += o2_round(r.out_cap, 16);
    chunks += lay.nc;
    stats_blocks += r.sn;
  }
  PCC_REQUIRE(chunks + nj < ((int64_t)1 << 31) && stats_blocks < ((int64_t)1 << 31), PCC_E_ARG,
              "octree blob v2: %lld chunks in %d jobs", (long long)chunks, nj);
  struct Own {   // the rare block of its own, freed on every way out
    void* p = nullptr;
    ~Own() { if (p) (void)hipFree(p); }
  } own;
  const size_t rec_b = pcc_align((size_t)rec_words * 2), work_b = rec_b;   // [chunk][step][lane] / [chunk][lane][T]
  const size_t small_b = pcc_align((size_t)chunks * (4 + 2 * kLanes * 2 + kLanes * 2));   // words | states | lens
  // version 4: the scratch of the reference bytes, sized by the largest frame's nodes (the frames take it in turn)
  size_t ref_need = 0;
  if (pred)
    for (int j = 0; j < nj; ++j) ref_need = std::max(ref_need, o4_ref_scratch_bytes(ct[(size_t)j].n_nodes, fr[tree_of(j)].n));
  uint16_t *rec, *work;
  char *small, *ref_scratch;
  if (pcc_align(ctx->arena_off) + rec_b + work_b + small_b + ref_need + scan_b + 2048 <= ctx->arena_cap) {
    rec = (uint16_t*)pcc_arena_alloc(ctx, rec_b);
    work = (uint16_t*)pcc_arena_alloc(ctx, work_b);
    small = (char*)pcc_arena_alloc(ctx, small_b);
    ref_scratch = (char*)pcc_arena_alloc(ctx, ref_need + 256);
  } else {
    PCC_HIP(hipMalloc(&own.p, rec_b + work_b + small_b + ref_need + 256));
    rec = (uint16_t*)own.p;
    work = (uint16_t*)((char*)own.p + rec_b);
    small = (char*)own.p + rec_b + work_b;
    ref_scratch = small + small_b;
  }
  if (!rec || !work || !small || !ref_scratch) return PCC_E_NOMEM;
  uint32_t* words = (uint32_t*)small;
  uint16_t* states = (uint16_t*)(small + (size_t)chunks * 4);
  uint16_t* lens_d = states + (size_t)chunks * 2 * kLanes;
  // staging: the coder's table on its way to the device | the blobs | their lengths
  const size_t lens_at = ct_b + (size_t)out_bytes;
  PCC_TRY(o2_stage_reserve_keep(ctx, stage_base + lens_at + (size_t)nj * 8 + 64, stage_base));
  uint8_t* stage = (uint8_t*)ctx->stage + stage_base;
  memcpy(stage, ct.data(), (size_t)nj * sizeof(O2Frame));
  PCC_HIP(hipMemcpyAsync(d_ct, stage, (size_t)nj * sizeof(O2Frame), hipMemcpyHostToDevice, st));
  long long* len_dev = (long long*)(stage + lens_at);
  if (pred) {
    std::vector<O4RefJob> jobs((size_t)nj);
    for (int q = 0; q < nj; ++q) {
      const int f = tree_of(q);
      O4RefJob& j = jobs[(size_t)q];
      const uint32_t* c = level_counts.data() + (size_t)PCC_OCT_CSTRIDE * f;
      j.occ_off = ct[(size_t)q].occ_off;
      j.rb_off = ct[(size_t)q].rb_off;
      j.n_points = fr[f].n;
      j.depth = fr[f].depth;
      int64_t run = 0;
      for (int L = 0; L <= 16; ++L) {
        j.off[L] = run;
        if (L < j.depth) run += (int64_t)c[L];
      }
      for (int a = 0; a < 3; ++a) j.origin[a] = fr[f].origin[a];
      j.ref_keys = pred[q].ref_keys;
      j.ref_n = pred[q].ref_n;
    }
    PCC_TRY(o4_ref_bytes_async(ctx, key_shift, jobs.data(), nj, occ, (uint8_t*)ref.rb, (uint32_t*)ref.ref_n,
                               (unsigned long long*)ref.ref_sum, ref_scratch, ref_need + 256));
    hipLaunchKernelGGL(k_o2_stats<true>, dim3((unsigned)stats_blocks), dim3(256), 0, st, (const uint8_t*)occ, (const O2Frame*)d_ct, nj, cnt, ref);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_o2_enc<true>, dim3((unsigned)chunks), dim3(64), 0, st, (const uint8_t*)occ, (const O2Frame*)d_ct, nj,
                       (const uint32_t*)cnt, rec, work, states, lens_d, words, p0, ref);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_o2_pack<true>, dim3((unsigned)(chunks + nj)), dim3(256), 0, st, (const uint16_t*)work, (const O2Frame*)d_ct, nj,
                       (const uint16_t*)states, (const uint16_t*)lens_d, (const uint32_t*)words, (const uint32_t*)counts,
                       (const uint16_t*)p0, stage + ct_b, len_dev, ref);
    PCC_CHECK_LAUNCH();
  } else {
    hipLaunchKernelGGL(k_o2_stats<false>, dim3((unsigned)stats_blocks), dim3(256), 0, st, (const uint8_t*)occ, (const O2Frame*)d_ct, nj, cnt, ref);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_o2_enc<false>, dim3((unsigned)chunks), dim3(64), 0, st, (const uint8_t*)occ, (const O2Frame*)d_ct, nj,
                       (const uint32_t*)cnt, rec, work, states, lens_d, words, p0, ref);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_o2_pack<false>, dim3((unsigned)(chunks + nj)), dim3(256), 0, st, (const uint16_t*)work, (const O2Frame*)d_ct, nj,
                       (const uint16_t*)states, (const uint16_t*)lens_d, (const uint32_t*)words, (const uint32_t*)counts,
                       (const uint16_t*)p0, stage + ct_b, len_dev, ref);
    PCC_CHECK_LAUNCH();
  }
  PCC_HIP(hipStreamSynchronize(st));
  offs->resize((size_t)nj);
  lens->resize((size_t)nj);
  for (int f = 0; f < nj; ++f) {
    const long long total = ((volatile long long*)len_dev)[f];
    PCC_REQUIRE(total >= 0 && total <= ct[(size_t)f].out_cap, PCC_E_NOMEM, "octree blob v2: frame %d: blob beyond its bound", tree_of(f));
    (*offs)[(size_t)f] = (int64_t)(stage_base + ct_b) + ct[(size_t)f].out_off;
    (*lens)[(size_t)f] = total;
  }
  return PCC_OK;
}

// blob version 2 of the rows d_keys[0 .. n) (Morton-sorted, one frame): the batch of one frame — two synchronisations
// (the level counts size the chunks; the blob's length), the blob itself is written into pinned memory by the packing
// kernel
int pcc_octree2_encode(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int key_shift, int depth, const int32_t origin[3],
                       uint8_t* h_out, int64_t cap, int64_t* h_len) {
  PCC_REQUIRE(ctx && d_keys && h_out && h_len && n >= 1 && n < ((int64_t)1 << 27) && depth >= 1 && depth <= 16, PCC_E_ARG,
              "pcc_octree2_encode: bad argument");
  PCC_REQUIRE(pcc_align((size_t)n) * (size_t)depth < ((size_t)1 << 31), PCC_E_ARG, "pcc_octree2_encode: %lld leaves at depth %d",
              (long long)n, depth);
  O2In one;
  one.lo = 0;
  one.n = n;
  one.depth = depth;
  for (int a = 0; a < 3; ++a) one.origin[a] = origin[a];
  std::vector<int64_t> offs, lens;
  PCC_TRY(o2_encode_batch(ctx, d_keys, key_shift, &one, 1, &offs, &lens));
  PCC_REQUIRE(lens[0] <= cap, PCC_E_NOMEM, "pcc_octree2_encode: blob does not fit %lld bytes", (long long)cap);
  memcpy(h_out, (uint8_t*)ctx->stage + offs[0], (size_t)lens[0]);
  *h_len = lens[0];
  return PCC_OK;
}

// version-2 blobs -> their points, Morton order inside a frame (origin added), concatenated in frame order: on the device
// (d_points) and / or on the host (h_points).  h_point_offsets[nb + 1] receives where every frame's points start;
// h_level_n (16 entries, nullable, nb == 1) the node counts of the levels.  Every header is checked, and the sizes the
// batch announces are summed and checked, before anything is reserved.  `who` names the frame in errors (nullptr: the
// one-blob messages).  One synchronisation.
//
// lod > 0 (octree2_blob.h): blobs or prefixes of them, every frame cut at level Lc = max(depth - lod, 0) — the same
// kernels over the tree of the first N' nodes, whose "points" are the m cells of level Lc: only the plan's bytes are
// uploaded, only the needed chunks launched, and nodes, scan, links and output are sized from N' and m, which the
// stream verifies (k_o2_link: the level boundaries above the cut, the children of the first N' nodes).  The level
// sizes below the cut and n are out of a prefix's reach: they stay bounded by the header checks alone, and nothing is
// sized from them.  A frame with Lc = 0 is its root cube: one cell, origin >> lod, no launch.
static int o2_decode_batch(pcc_ctx* ctx, const uint8_t* const* blobs, const int64_t* lens, int nb, const char* who, int lod,
                           int32_t* d_points, int32_t* h_points, int64_t cap_points, int64_t* h_point_offsets,
                           int64_t* h_level_n) {
  std::vector<O2Info> info((size_t)nb);
  std::vector<O2Plan> plan((size_t)nb);
  int64_t points = 0, nodes = 0, links = 0, bodies = 0;
  int roots = 0;   // frames that are their root cube alone
  h_point_offsets[0] = 0;
  for (int f = 0; f < nb; ++f) {
    O2Info& o = info[(size_t)f];
    O2Plan& pl = plan[(size_t)f];
    if (who) {
      const int v = pcc_octree_blob_version(blobs[f], lens[f]);
      if (v < 0) return o2_frame_error(v, who, f);
      PCC_REQUIRE(v == 2, PCC_E_ARG, "%s: frame %d: blob version %d (this call reads version 2)", who, f, v);
      const int rc = o2_parse(blobs[f], lens[f], lod, true, &o, &pl);
      if (rc != PCC_OK) return o2_frame_error(rc, who, f);
    } else {
      PCC_TRY(o2_parse(blobs[f], lens[f], lod, true, &o, &pl));
    }
    points += pl.m;
    h_point_offsets[f + 1] = points;
    if (pl.n_dec == 0) {
      roots += pl.m ? 1 : 0;
      continue;
    }
    nodes += o2_round(pl.n_dec, 4);
    links += pl.n_dec + pl.m;
    bodies += o2_round(pl.bytes - o.off_p0, 16);
  }
  if (h_level_n) {   // (lod 0 callers only)
    for (int L = 0; L < 16; ++L) h_level_n[L] = 0;
    if (info[0].n)
      for (int L = 0; L < info[0].depth; ++L) h_level_n[L] = info[0].level_n[L];
  }
  PCC_REQUIRE(nodes < ((int64_t)1 << 28) && points < ((int64_t)1 << 31) && links < ((int64_t)1 << 32), PCC_E_ARG,
              "%s: the blobs announce %lld nodes and %lld points in all", who ? who : "pcc_octree2_decode", (long long)nodes,
              (long long)points);
  if (points == 0 || (!d_points && !h_points)) return PCC_OK;
  PCC_REQUIRE(cap_points >= points, PCC_E_NOMEM, "%s: %lld points, capacity %lld", who ? who : "pcc_octree2_decode",
              (long long)points, (long long)cap_points);
  // the table: frames with nodes to decode only
  std::vector<O2DFrame> tab;
  int64_t node_base = 0, link_base = 0, body_off = 0, chunks = 0, lblocks = 0, qblocks = 0;
  for (int f = 0; f < nb; ++f) {
    const O2Info& o = info[(size_t)f];
    const O2Plan& pl = plan[(size_t)f];
    if (pl.n_dec == 0) continue;
    O2DFrame r;
    r.body_off = body_off;
    r.table_off = o.off_table - o.off_p0;
    r.payload_off = o.off_payload - o.off_p0;
    r.n_nodes = pl.n_dec;
    r.start_last = o.n_nodes - o.level_n[o.depth - 1];
    r.start_prev = o.depth >= 2 ? r.start_last - o.level_n[o.depth - 2] : 0;
    r.n_points = pl.m;
    r.n_full = o.n_nodes;
    r.node_base = node_base;
    r.link_base = link_base;
    r.pt_base = h_point_offsets[f];
    int64_t run = 0;
    for (int L = 0; L <= 16; ++L) {
      r.off[L] = run;
      if (L < pl.Lc) run += o.level_n[L];
    }
    r.S = (int32_t)o.S;
    r.nc = (int32_t)pl.chunks;
    r.cb = (int32_t)chunks;
    r.lb = (int32_t)lblocks;
    r.qb = (int32_t)qblocks;
    r.depth = pl.Lc;
    r.lanes_last = (int32_t)pl.lanes;
    r.last_words = (uint32_t)pl.last_words;
    for (int a = 0; a < 3; ++a) r.origin[a] = o.origin[a] >> lod;
    tab.push_back(r);
    node_base += o2_round(pl.n_dec, 4);
    link_base += pl.n_dec + pl.m;
    body_off += o2_round(pl.bytes - o.off_p0, 16);
    chunks += pl.chunks;
    lblocks += nblk(pl.n_dec, 256);
    qblocks += nblk(pl.m, 256);
  }
  const int nf = (int)tab.size();
  hipStream_t st = ctx->stream;
  const size_t tab_b = pcc_align((size_t)nf * sizeof(O2DFrame));
  PCC_TRY(pcc_arena_reserve(ctx, tab_b + pcc_align((size_t)bodies + 16) + pcc_align((size_t)nodes + 16) + 2 * pcc_align((size_t)nodes * 4) +
                                     pcc_align((size_t)links * 4) + (d_points ? 0 : pcc_align((size_t)points * 12)) +
                                     pcc_align((size_t)nf * 4 + 64) + pcc_scan_scratch_bytes(nodes) + 8192));
  // the table and the bodies (p0 | chunk table | payload: 4-byte aligned inside a blob, header 24 + 4 depth + 8) cross in
  // one copy
  uint8_t* d_in = (uint8_t*)pcc_arena_alloc(ctx, tab_b + (size_t)bodies + 16);
  uint8_t* occ = (uint8_t*)pcc_arena_alloc(ctx, (size_t)nodes + 16);
  uint32_t* pc = (uint32_t*)pcc_arena_alloc(ctx, (size_t)nodes * 4);
  uint32_t* excl = (uint32_t*)pcc_arena_alloc(ctx, (size_t)nodes * 4);
  uint32_t* link = (uint32_t*)pcc_arena_alloc(ctx, (size_t)links * 4);
  int32_t* pts = d_points ? d_points : (int32_t*)pcc_arena_alloc(ctx, (size_t)points * 12);
  int32_t* status = (int32_t*)pcc_arena_alloc(ctx, (size_t)nf * 4 + 64);   // per frame | total of the scan
  if (!pts || !status || (nf > 0 && (!d_in || !occ || !pc || !excl || !link))) return PCC_E_NOMEM;
  uint32_t* total = (uint32_t*)(status + nf);
  const O2DFrame* d_tab = (const O2DFrame*)d_in;
  const uint8_t* d_bodies = d_in + tab_b;
  PccProfScope prof(ctx, "octree2_decode", points, info[0].depth, nodes, chunks);
  const size_t in_b = tab_b + (size_t)bodies;
  // a caller's array in pinned host memory receives the points straight from the device; any other one through the
  // staging (a failed query of an ordinary pointer leaves its error behind: cleared here)
  bool direct = false;
  if (h_points) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, h_points) == hipSuccess)
      direct = attr.type == hipMemoryTypeHost;
    else
      (void)hipGetLastError();
  }
  const size_t out_bytes = h_points && !direct ? (size_t)points * 12 : 0;
  const size_t roots_at = pcc_align(in_b) + pcc_align(out_bytes) + (size_t)nf * 4 + 64;
  PCC_TRY(o2_stage_reserve(ctx, roots_at + (size_t)roots * 12));
  uint8_t* stage = (uint8_t*)ctx->stage;
  memcpy(stage, tab.data(), (size_t)nf * sizeof(O2DFrame));
  for (int f = 0, k = 0; f < nb; ++f) {
    const O2Info& o = info[(size_t)f];
    if (plan[(size_t)f].n_dec == 0) continue;
    memcpy(stage + tab_b + tab[(size_t)k].body_off, blobs[f] + o.off_p0, (size_t)(plan[(size_t)f].bytes - o.off_p0));
    ++k;
  }
  // the frames that are their root cube alone: the one cell goes to its row as it is
  int32_t* h_roots = (int32_t*)(stage + roots_at);
  for (int f = 0, k = 0; f < nb && k < roots; ++f) {
    if (plan[(size_t)f].n_dec != 0 || plan[(size_t)f].m == 0) continue;
    for (int a = 0; a < 3; ++a) h_roots[3 * k + a] = info[(size_t)f].origin[a] >> lod;
    PCC_HIP(hipMemcpyAsync(pts + 3 * h_point_offsets[f], h_roots + 3 * k, 12, hipMemcpyHostToDevice, st));
    ++k;
  }
  if (nf > 0) {   // (no frame with nodes: a call of root cubes alone, at a lod at or beyond every depth)
    PCC_HIP(hipMemcpyAsync(d_in, stage, in_b, hipMemcpyHostToDevice, st));
    PCC_HIP(hipMemsetAsync(status, 0, (size_t)nf * 4 + 64, st));
    PCC_HIP(hipMemsetAsync(link, 0, (size_t)links * 4, st));
    hipLaunchKernelGGL(k_o2_dec, dim3((unsigned)chunks), dim3(64), 0, st, d_bodies, d_tab, nf, occ, status);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_o2_popc, dim3(nblk(nodes, 256)), dim3(256), 0, st, (const uint8_t*)occ, nodes, pc);
    PCC_CHECK_LAUNCH();
    PCC_TRY(pcc_scan_exclusive_u32(ctx, pc, excl, nodes, total));
    hipLaunchKernelGGL(k_o2_link, dim3((unsigned)lblocks), dim3(256), 0, st, (const uint8_t*)occ, (const uint32_t*)excl,
                       (const uint32_t*)total, nodes, d_tab, nf, link, status);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_o2_points, dim3((unsigned)qblocks), dim3(256), 0, st, (const uint32_t*)link, d_tab, nf, pts, status);
    PCC_CHECK_LAUNCH();
  }
  uint8_t* stage_out = stage + pcc_align(in_b);
  int32_t* h_status = (int32_t*)(stage_out + pcc_align(out_bytes));
  if (h_points) PCC_HIP(hipMemcpyAsync(direct ? (void*)h_points : (void*)stage_out, pts, (size_t)points * 12, hipMemcpyDeviceToHost, st));
  if (nf > 0) PCC_HIP(hipMemcpyAsync(h_status, status, (size_t)nf * 4, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipStreamSynchronize(st));
  for (int f = 0, k = 0; f < nb; ++f) {
    if (plan[(size_t)f].n_dec == 0) continue;
    const int32_t bad = h_status[k++];
    if (!who)
      PCC_REQUIRE(bad == 0, PCC_E_STREAM, "octree blob v2: corrupt stream (status %d: 1 = words, 2 = empty node, 8 = counts)", bad);
    else
      PCC_REQUIRE(bad == 0, PCC_E_STREAM, "%s: frame %d: octree blob v2: corrupt stream (status %d: 1 = words, 2 = empty node, 8 = counts)",
                  who, f, bad);
  }
  if (h_points && !direct) memcpy(h_points, stage_out, out_bytes);
  return PCC_OK;
}

// version-2 blob -> Morton-ordered points int32 [n, 3] (origin added): the batch of one blob
int pcc_octree2_decode(pcc_ctx* ctx, const uint8_t* h_in, int64_t len, int32_t* d_points, int32_t* h_points, int64_t cap_points,
                       int64_t* h_n_points, int64_t* h_level_n) {
  PCC_REQUIRE(ctx, PCC_E_ARG, "pcc_octree2_decode: null ctx");
  int64_t offs[2] = {0, 0};
  const int rc = o2_decode_batch(ctx, &h_in, &len, 1, nullptr, 0, d_points, h_points, cap_points, offs, h_level_n);
  if (h_n_points && (rc == PCC_OK || offs[1] > 0)) *h_n_points = offs[1];
  return rc;
}

// ---- C-ABI: many frames per call (include/pcc.h) ----------------------------------------------------------------------
// the frames of an encode call: offs[f] = first key of frame f (offs[n_frames] = n), ends[2 f], ends[2 f + 1] = a frame's
// first and last key; the keys are checked (sorted, distinct after the key shift, frame index).  One synchronisation.
static int o2_frame_bounds(const char* who, pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int key_shift,
                           std::vector<int64_t>* offs_out, std::vector<uint64_t>* ends_out) {
  hipStream_t st = ctx->stream;
  std::vector<int64_t>& offs = *offs_out;
  std::vector<uint64_t>& ends = *ends_out;
  offs.assign((size_t)n_frames + 1, 0);
  ends.assign((size_t)2 * n_frames, 0);
  if (n > 0) {
    const size_t offs_b = (size_t)(n_frames + 1) * 8, ends_b = (size_t)n_frames * 16, rd_b = offs_b + ends_b + 8;
    PCC_TRY(pcc_arena_reserve(ctx, rd_b + 256));
    uint8_t* rd = (uint8_t*)pcc_arena_alloc(ctx, rd_b);
    if (!rd) return PCC_E_NOMEM;
    int64_t* d_offs = (int64_t*)rd;
    uint64_t* d_ends = (uint64_t*)(rd + offs_b);
    int32_t* d_flag = (int32_t*)(rd + offs_b + ends_b);
    PCC_TRY(o2_stage_reserve(ctx, rd_b));
    PCC_HIP(hipMemsetAsync(rd, 0, rd_b, st));
    hipLaunchKernelGGL(k_of_check, dim3(nblk(n, 256)), dim3(256), 0, st, d_keys, n, key_shift, n_frames, d_flag);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_of_frames, dim3(nblk(n_frames + 1, 64)), dim3(64), 0, st, d_keys, n, n_frames, d_offs, d_ends);
    PCC_CHECK_LAUNCH();
    PCC_HIP(hipMemcpyAsync(ctx->stage, rd, rd_b, hipMemcpyDeviceToHost, st));
    PCC_HIP(hipStreamSynchronize(st));
    const uint8_t* h = (const uint8_t*)ctx->stage;
    int32_t flag;
    memcpy(&flag, h + offs_b + ends_b, 4);
    PCC_REQUIRE(!(flag & 4), PCC_E_ARG, "%s: a key's frame index is not below n_frames=%d", who, n_frames);
    PCC_REQUIRE(!(flag & 2), PCC_E_ARG, "%s: keys not sorted (pcc_sort_pairs)", who);
    PCC_REQUIRE(!(flag & 1), PCC_E_DUP, "%s: duplicate keys (after the key shift of %d)", who, key_shift);
    memcpy(offs.data(), h, offs_b);
    memcpy(ends.data(), h + offs_b, ends_b);
  }
  return PCC_OK;
}

extern "C" int pcc_octree_encode_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int key_shift,
                                        uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  PCC_REQUIRE(ctx && h_out && h_offsets && n >= 0 && (n == 0 || d_keys) && n < ((int64_t)1 << 27) && n_frames >= 1 &&
                  n_frames <= 65535 && key_shift >= 0 && key_shift % 3 == 0 && key_shift <= 45 && cap >= 0,
              PCC_E_ARG, "pcc_octree_encode_frames: bad argument (n=%lld n_frames=%d key_shift=%d)", (long long)n, n_frames,
              key_shift);
  std::vector<int64_t> offs;
  std::vector<uint64_t> ends;
  PCC_TRY(o2_frame_bounds("pcc_octree_encode_frames", ctx, d_keys, n, n_frames, key_shift, &offs, &ends));
  std::vector<O2In> fr;
  std::vector<int> frame_of;
  for (int f = 0; f < n_frames; ++f) {
    const int64_t lo = offs[(size_t)f], hi = offs[(size_t)f + 1];
    if (hi <= lo) continue;
    O2In g;
    g.lo = lo;
    g.n = hi - lo;
    octree_root(ends[2 * (size_t)f], ends[2 * (size_t)f + 1], key_shift, &g.depth, g.origin);
    fr.push_back(g);
    frame_of.push_back(f);
  }
  std::vector<int64_t> boff, blen;
  if (!fr.empty()) PCC_TRY(o2_encode_batch(ctx, d_keys, key_shift, fr.data(), (int)fr.size(), &boff, &blen));
  // blob f = h_out[h_offsets[f], h_offsets[f + 1]); frames without keys get the 24-byte empty blob
  std::vector<int64_t> len_of((size_t)n_frames, kHeader);
  for (size_t k = 0; k < fr.size(); ++k) len_of[(size_t)frame_of[k]] = blen[k];
  int64_t total = 0;
  for (int f = 0; f < n_frames; ++f) total += len_of[(size_t)f];
  PCC_REQUIRE(total <= cap, PCC_E_NOMEM, "pcc_octree_encode_frames: %lld bytes of blobs, capacity %lld", (long long)total,
              (long long)cap);
  h_offsets[0] = 0;
  for (int f = 0, k = 0; f < n_frames; ++f) {
    uint8_t* dst = h_out + h_offsets[f];
    if (k < (int)fr.size() && frame_of[(size_t)k] == f) {
      memcpy(dst, (const uint8_t*)ctx->stage + boff[(size_t)k], (size_t)blen[(size_t)k]);
      ++k;
    } else {
      memset(dst, 0, kHeader);
      dst[0] = 'O';
      dst[1] = 2;
    }
    h_offsets[f + 1] = h_offsets[f] + len_of[(size_t)f];
  }
  return PCC_OK;
}

// Inter-frame coding (include/pcc.h has the rule of version 4): the reference of a frame is the frame in front of it
// in the call, or with history > 1 the union of its window, the up to `history` frames in front of it — lossless
// coding makes the original the decoded frame, so all frames still encode side by side: the intra frames in one batch
// of version 2, the predicted ones in one batch of version 4.  The unions of all windows of more than one frame are
// formed first, in one merge (o4_merge_async) and one synchronisation for their sizes; a call without such a window
// queues what it queued before history.
static int o2_encode_frames_inter(const char* who, pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int key_shift,
                                  int intra_period, int n_ref_frames, int history, uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  std::vector<int64_t> offs;
  std::vector<uint64_t> ends;
  PCC_TRY(o2_frame_bounds(who, ctx, d_keys, n, n_frames, key_shift, &offs, &ends));
  std::vector<O2In> fr[2];            // [0] intra, [1] predicted
  std::vector<int> frame_of[2];
  std::vector<O4Pred> pred;
  std::vector<int> window;            // of the predicted frames
  std::vector<O4MergeJob> jobs;       // of those with a window of more than one frame
  std::vector<size_t> job_pred;
  std::vector<char> is_intra((size_t)n_frames, 0);   // coded frames written as version 2
  int64_t merged = 0;
  for (int f = n_ref_frames; f < n_frames; ++f) {
    const int64_t lo = offs[(size_t)f], hi = offs[(size_t)f + 1];
    if (hi <= lo) continue;
    const int g = f - n_ref_frames;     // its place among the coded frames
    const bool intra = intra_period > 0 ? g % intra_period == 0 : f == 0;
    const int64_t ref_n = f > 0 ? lo - offs[(size_t)f - 1] : 0;
    const int k = !intra && ref_n > 0 ? 1 : 0;   // a frame whose reference has no points is written as version 2
    O2In in;
    in.lo = lo;
    in.n = hi - lo;
    octree_root(ends[2 * (size_t)f], ends[2 * (size_t)f + 1], key_shift, &in.depth, in.origin);
    fr[k].push_back(in);
    frame_of[k].push_back(f);
    is_intra[(size_t)f] = k ? 0 : 1;
    if (!k) continue;
    // the window: back from f - 1, up to `history` frames, not past a frame without points, not past an intra frame
    int W = 1;
    while (W < history && !is_intra[(size_t)(f - W)] && f - W - 1 >= 0 && offs[(size_t)(f - W)] > offs[(size_t)(f - W - 1)]) ++W;
    window.push_back(W);
    if (W == 1) {
      pred.push_back(O4Pred{d_keys + offs[(size_t)f - 1], ref_n});
      continue;
    }
    const int64_t keys = lo - offs[(size_t)(f - W)];
    PCC_REQUIRE(keys < ((int64_t)1 << 27), PCC_E_ARG, "%s: frame %d: the %d frames of its window hold %lld keys", who, g, W,
                (long long)keys);
    O4MergeJob j;
    j.nl = W;
    j.out = nullptr;   // below: its place in the call's block, `merged` keys in
    for (int i = 0; i < W; ++i) {
      j.list[i] = d_keys + offs[(size_t)(f - W + i)];
      j.n[i] = offs[(size_t)(f - W + i + 1)] - offs[(size_t)(f - W + i)];
    }
    job_pred.push_back(pred.size());
    pred.push_back(O4Pred{nullptr, merged});
    jobs.push_back(j);
    merged += keys;
  }
  struct Own {   // the unions and the merge's scratch; the table on its way to the device
    void* p = nullptr;
    ~Own() { if (p) (void)hipFree(p); }
  } own;
  std::vector<O4MergeDev> tab(jobs.size());
  if (!jobs.empty()) {
    PCC_REQUIRE(merged + 1 < ((int64_t)1 << 31), PCC_E_ARG, "%s: the windows of the call hold %lld keys in all", who, (long long)merged);
    const size_t union_b = pcc_align((size_t)merged * 8), scratch_b = o4_merge_scratch_bytes(merged, (int)jobs.size());
    PCC_HIP(hipMalloc(&own.p, union_b + scratch_b));
    for (size_t i = 0; i < jobs.size(); ++i) {
      jobs[i].out = (uint64_t*)own.p + pred[job_pred[i]].ref_n;
      pred[job_pred[i]].ref_keys = jobs[i].out;
    }
    uint32_t* d_counts = nullptr;
    std::vector<uint32_t> counts(jobs.size());
    int rc = o4_merge_async(ctx, jobs.data(), (int)jobs.size(), key_shift, (char*)own.p + union_b, scratch_b, tab.data(), &d_counts);
    if (rc == PCC_OK && hipMemcpyAsync(counts.data(), d_counts, counts.size() * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
      pcc_set_error("%s: reading the sizes of the merged references failed", who);
      rc = PCC_E_HIP;
    }
    const bool synced = hipStreamSynchronize(ctx->stream) == hipSuccess;   // (also what keeps `tab` and `counts` until the copies are done)
    PCC_TRY(rc);
    PCC_REQUIRE(synced, PCC_E_HIP, "%s: the merge of the reference windows failed", who);
    for (size_t i = 0; i < jobs.size(); ++i) pred[job_pred[i]].ref_n = (int64_t)counts[i];
  }
  // blob f; frames without keys get the 24-byte empty blob, the reference frames none
  std::vector<std::vector<uint8_t>> blob((size_t)n_frames);
  for (int f = n_ref_frames; f < n_frames; ++f) {
    blob[(size_t)f].assign((size_t)kHeader, 0);
    blob[(size_t)f][0] = 'O';
    blob[(size_t)f][1] = 2;
  }
  for (int k = 0; k < 2; ++k) {
    if (fr[k].empty()) continue;
    std::vector<int64_t> boff, blen;
    PCC_TRY(o2_encode_batch(ctx, d_keys, key_shift, fr[k].data(), (int)fr[k].size(), &boff, &blen, k ? pred.data() : nullptr));
    for (size_t i = 0; i < fr[k].size(); ++i) {
      const uint8_t* src = (const uint8_t*)ctx->stage + boff[i];
      blob[(size_t)frame_of[k][i]].assign(src, src + blen[i]);
      if (k) blob[(size_t)frame_of[k][i]][3] = (uint8_t)(window[i] - 1);   // byte 3 of version 4's head: W - 1
    }
  }
  int64_t total = 0;
  for (const auto& b : blob) total += (int64_t)b.size();
  PCC_REQUIRE(total <= cap, PCC_E_NOMEM, "%s: %lld bytes of blobs, capacity %lld", who, (long long)total, (long long)cap);
  h_offsets[0] = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (!blob[(size_t)f].empty()) memcpy(h_out + h_offsets[f], blob[(size_t)f].data(), blob[(size_t)f].size());
    h_offsets[f + 1] = h_offsets[f] + (int64_t)blob[(size_t)f].size();
  }
  return PCC_OK;
}

extern "C" int pcc_octree_encode_frames_inter_hist(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int key_shift,
                                                   int intra_period, int n_ref_frames, int history, uint8_t* h_out, int64_t cap,
                                                   int64_t* h_offsets) {
  const char* who = "pcc_octree_encode_frames_inter_hist";
  PCC_REQUIRE(ctx && h_out && h_offsets && n >= 0 && (n == 0 || d_keys) && n < ((int64_t)1 << 27) && n_frames >= 1 &&
                  n_frames <= 65535 && key_shift >= 0 && key_shift % 3 == 0 && key_shift <= 45 && cap >= 0 && intra_period >= 0 &&
                  history >= 1 && history <= kO4MaxWindow && n_ref_frames >= 0 && n_ref_frames <= history && n_ref_frames < n_frames,
              PCC_E_ARG, "%s: bad argument (n=%lld n_frames=%d key_shift=%d intra_period=%d n_ref_frames=%d history=%d)", who,
              (long long)n, n_frames, key_shift, intra_period, n_ref_frames, history);
  return o2_encode_frames_inter(who, ctx, d_keys, n, n_frames, key_shift, intra_period, n_ref_frames, history, h_out, cap, h_offsets);
}

extern "C" int pcc_octree_encode_frames_inter(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int key_shift,
                                              int intra_period, int ref_first, uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  const char* who = "pcc_octree_encode_frames_inter";
  PCC_REQUIRE(ctx && h_out && h_offsets && n >= 0 && (n == 0 || d_keys) && n < ((int64_t)1 << 27) && n_frames >= 1 &&
                  n_frames <= 65535 && key_shift >= 0 && key_shift % 3 == 0 && key_shift <= 45 && cap >= 0 && intra_period >= 0 &&
                  (ref_first == 0 || ref_first == 1),
              PCC_E_ARG, "%s: bad argument (n=%lld n_frames=%d key_shift=%d intra_period=%d ref_first=%d)", who, (long long)n,
              n_frames, key_shift, intra_period, ref_first);
  return o2_encode_frames_inter(who, ctx, d_keys, n, n_frames, key_shift, intra_period, ref_first, 1, h_out, cap, h_offsets);
}

// Intra or a window, chosen per frame (include/pcc.h has the rule; octree_best_host.h its host side).  Lossless coding
// makes the original the decoded frame, so the choice for one frame changes nothing for another, and every candidate
// of every frame is coded side by side: one batch of version 2 over the coded frames with points, one batch of version
// 4 over all (frame, W) jobs, the levels of a frame built once in it.  In front of them the unions W = 2 .. Wmax of
// every frame in one nested pass (o4_nest_async) and one synchronisation for their sizes.  The version-2 blobs stay in
// the staging while the second batch works behind them; after its last synchronisation all lengths are on the host,
// and only the winners are copied out.
extern "C" int pcc_octree_encode_frames_inter_best(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int key_shift,
                                                   int intra_period, int n_ref_frames, int history, uint8_t* h_out, int64_t cap,
                                                   int64_t* h_offsets) {
  const char* who = "pcc_octree_encode_frames_inter_best";
  PCC_REQUIRE(ctx && h_out && h_offsets && n >= 0 && (n == 0 || d_keys) && n < ((int64_t)1 << 27) && n_frames >= 1 &&
                  n_frames <= 65535 && key_shift >= 0 && key_shift % 3 == 0 && key_shift <= 45 && cap >= 0 && intra_period >= 0 &&
                  history >= 1 && history <= kO4MaxWindow && n_ref_frames >= 0 && n_ref_frames <= history && n_ref_frames < n_frames,
              PCC_E_ARG, "%s: bad argument (n=%lld n_frames=%d key_shift=%d intra_period=%d n_ref_frames=%d history=%d)", who,
              (long long)n, n_frames, key_shift, intra_period, n_ref_frames, history);
  std::vector<int64_t> offs;
  std::vector<uint64_t> ends;
  PCC_TRY(o2_frame_bounds(who, ctx, d_keys, n, n_frames, key_shift, &offs, &ends));
  std::vector<int> wmax;
  o4_best_windows(offs.data(), n_frames, n_ref_frames, intra_period, history, &wmax);
  std::vector<O2In> fr[2];         // [0] every coded frame with points, [1] those with a window
  std::vector<int> frame_of[2];
  std::vector<int> job_tree, job_w;   // the version-4 jobs: index into fr[1], window
  std::vector<O4Pred> pred;
  std::vector<O4NestJob> nests;       // of the frames with Wmax >= 2
  std::vector<size_t> nest_job;       // the job of a nest's window 1
  int64_t room = 0, listed = 0;       // keys: of all unions, of all nests' lists
  for (int f = n_ref_frames; f < n_frames; ++f) {
    if (wmax[(size_t)f] < 0) continue;
    O2In in;
    in.lo = offs[(size_t)f];
    in.n = offs[(size_t)f + 1] - in.lo;
    octree_root(ends[2 * (size_t)f], ends[2 * (size_t)f + 1], key_shift, &in.depth, in.origin);
    fr[0].push_back(in);
    frame_of[0].push_back(f);
    const int Wm = wmax[(size_t)f];
    if (Wm == 0) continue;
    const int64_t keys = offs[(size_t)f] - offs[(size_t)(f - Wm)];
    PCC_REQUIRE(keys < ((int64_t)1 << 27), PCC_E_ARG, "%s: frame %d: the %d frames of its window hold %lld keys", who, f - n_ref_frames, Wm,
                (long long)keys);
    O4NestJob nj;
    nj.nl = Wm;
    int64_t run = 0;
    for (int W = 1; W <= Wm; ++W) {   // list W - 1 = the frame W in front; union W's place in the call's block: below
      nj.list[W - 1] = d_keys + offs[(size_t)(f - W)];
      nj.n[W - 1] = offs[(size_t)(f - W + 1)] - offs[(size_t)(f - W)];
      run += nj.n[W - 1];
      nj.out[W - 1] = nullptr;
      job_tree.push_back((int)fr[1].size());
      job_w.push_back(W);
      pred.push_back(W == 1 ? O4Pred{nj.list[0], nj.n[0]} : O4Pred{nullptr, room});
      if (W >= 2) room += run;
    }
    if (Wm >= 2) {
      nest_job.push_back(pred.size() - (size_t)Wm);
      nests.push_back(nj);
      listed += run;
      PCC_REQUIRE(room < ((int64_t)1 << 31) && listed + 1 < ((int64_t)1 << 31), PCC_E_ARG,
                  "%s: frame %d: the windows of the call hold %lld keys in all", who, f - n_ref_frames, (long long)room);
    }
    fr[1].push_back(in);
    frame_of[1].push_back(f);
  }
  struct Own {   // the unions and the nested pass's scratch
    void* p = nullptr;
    ~Own() { if (p) (void)hipFree(p); }
  } own;
  std::vector<O4MergeDev> tab(nests.size());
  std::vector<O4NestOut> outs(nests.size());
  if (!nests.empty()) {
    // before anything of the candidates is launched: one block for the unions, sum over frames and W of the keys of the
    // windows' lists (the bound of sum |U_W|, whose sizes only the pass itself gives), and the pass's scratch
    const size_t union_b = pcc_align((size_t)room * 8), scratch_b = o4_nest_scratch_bytes(listed, (int)nests.size());
    if (hipMalloc(&own.p, union_b + scratch_b) != hipSuccess) {
      (void)hipGetLastError();
      own.p = nullptr;
      pcc_set_error("%s: the unions of the call's windows do not fit: %lld keys in %d frames' windows take %lld bytes of device memory", who,
                    (long long)room, (int)nests.size(), (long long)(union_b + scratch_b));
      return PCC_E_NOMEM;
    }
    for (size_t i = 0; i < nests.size(); ++i)
      for (int W = 2; W <= nests[i].nl; ++W) {
        O4Pred& p = pred[nest_job[i] + (size_t)W - 1];
        nests[i].out[W - 1] = (uint64_t*)own.p + p.ref_n;
        p.ref_keys = nests[i].out[W - 1];
      }
    uint32_t* d_counts = nullptr;
    std::vector<uint32_t> counts(nests.size() * kO4MaxWindow);
    int rc = o4_nest_async(ctx, nests.data(), (int)nests.size(), key_shift, (char*)own.p + union_b, scratch_b, tab.data(), outs.data(),
                           &d_counts);
    if (rc == PCC_OK && hipMemcpyAsync(counts.data(), d_counts, counts.size() * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
      pcc_set_error("%s: reading the sizes of the merged references failed", who);
      rc = PCC_E_HIP;
    }
    const bool synced = hipStreamSynchronize(ctx->stream) == hipSuccess;   // (also what keeps `tab`, `outs` and `counts` until the copies are done)
    PCC_TRY(rc);
    PCC_REQUIRE(synced, PCC_E_HIP, "%s: the merge of the reference windows failed", who);
    for (size_t i = 0; i < nests.size(); ++i)
      for (int W = 2; W <= nests[i].nl; ++W) pred[nest_job[i] + (size_t)W - 1].ref_n = (int64_t)counts[i * kO4MaxWindow + (size_t)W - 1];
  }
  std::vector<O4BestCand> cands;
  size_t stage_used = 0;
  if (!fr[0].empty()) {
    std::vector<int64_t> boff, blen;
    PCC_TRY(o2_encode_batch(ctx, d_keys, key_shift, fr[0].data(), (int)fr[0].size(), &boff, &blen));
    for (size_t i = 0; i < fr[0].size(); ++i) {
      cands.push_back(O4BestCand{frame_of[0][i], 0, boff[i], blen[i]});
      stage_used = std::max(stage_used, (size_t)(boff[i] + blen[i]));
    }
  }
  if (!job_tree.empty()) {
    std::vector<int64_t> boff, blen;
    PCC_TRY(o2_encode_batch(ctx, d_keys, key_shift, fr[1].data(), (int)fr[1].size(), &boff, &blen, pred.data(), job_tree.data(),
                            (int)job_tree.size(), (size_t)o2_round((int64_t)stage_used, 256)));
    for (size_t j = 0; j < job_tree.size(); ++j) cands.push_back(O4BestCand{frame_of[1][(size_t)job_tree[j]], job_w[j], boff[j], blen[j]});
  }
  std::vector<int64_t> choice;
  o4_best_choose(cands.data(), (int64_t)cands.size(), n_frames, &choice);
  int64_t need = 0;
  const int64_t wrote = o4_best_copy((const uint8_t*)ctx->stage, (int64_t)ctx->stage_cap, cands.data(), choice.data(), n_frames, n_ref_frames,
                                     h_out, cap, h_offsets, &need);
  PCC_REQUIRE(wrote != -2, PCC_E_HIP, "%s: a blob outside the staging", who);
  PCC_REQUIRE(wrote >= 0, PCC_E_NOMEM, "%s: %lld bytes of blobs, capacity %lld", who, (long long)need, (long long)cap);
  return PCC_OK;
}

static int o2_decode_frames(const char* who, pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                            int lod, int32_t* d_points, int32_t* h_points, int64_t cap_points, int64_t* h_point_offsets) {
  PCC_REQUIRE(ctx && h_blobs && h_lens && h_point_offsets && n_frames >= 1 && n_frames <= 65535, PCC_E_ARG,
              "%s: bad argument (n_frames=%d)", who, n_frames);
  PCC_REQUIRE(lod >= 0 && lod <= kO2MaxLod, PCC_E_ARG, "%s: level of detail %d outside 0 .. %d", who, lod, kO2MaxLod);
  return o2_decode_batch(ctx, h_blobs, h_lens, n_frames, who, lod, d_points, h_points, cap_points, h_point_offsets, nullptr);
}

extern "C" int pcc_octree_decode_frames(pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                                        int32_t* d_points, int32_t* h_points, int64_t cap_points, int64_t* h_point_offsets) {
  return o2_decode_frames("pcc_octree_decode_frames", ctx, h_blobs, h_lens, n_frames, 0, d_points, h_points, cap_points,
                          h_point_offsets);
}

extern "C" int pcc_octree_decode_frames_lod(pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                                            int lod, int32_t* d_points, int32_t* h_points, int64_t cap_points,
                                            int64_t* h_point_offsets) {
  return o2_decode_frames("pcc_octree_decode_frames_lod", ctx, h_blobs, h_lens, n_frames, lod, d_points, h_points, cap_points,
                          h_point_offsets);
}

// host only: what level `lod` of a version-2 or version-4 blob needs (bytes of its shortest prefix) and gives (cells)
extern "C" int pcc_octree_lod_info(const uint8_t* h_in, int64_t len, int lod, int64_t* h_bytes, int64_t* h_cells) {
  PCC_REQUIRE(lod >= 0 && lod <= kO2MaxLod, PCC_E_ARG, "pcc_octree_lod_info: level of detail %d outside 0 .. %d", lod, kO2MaxLod);
  if (h_in && len >= kO4Header && h_in[0] == 'O' && h_in[1] == 4) {   // a predicted frame: the same formulas over its offsets
    O4Info o4;
    O4Plan pl4;
    PCC_TRY(o4_parse_lod(h_in, len, lod, false, &o4, &pl4));
    if (h_bytes) *h_bytes = pl4.bytes;
    if (h_cells) *h_cells = pl4.m;
    return PCC_OK;
  }
  const int v = pcc_octree_blob_version(h_in, len);
  if (v < 0) return v;
  PCC_REQUIRE(v == 2, PCC_E_ARG, "pcc_octree_lod_info: blob version %d (levels of detail are a property of versions 2 and 4)", v);
  O2Info o;
  O2Plan pl;
  PCC_TRY(o2_parse(h_in, len, lod, false, &o, &pl));
  if (h_bytes) *h_bytes = pl.bytes;
  if (h_cells) *h_cells = pl.m;
  return PCC_OK;
}

// ---- C-ABI: the geometry slot, one call each (utils.gpcc_encode / gpcc_decode, shared/utils.py:169-240) -------------
extern "C" int pcc_octree_encode_version(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int key_shift, int version,
                                         uint8_t* h_out, int64_t cap, int64_t* h_len) {
  PCC_REQUIRE(ctx && h_out && h_len && n >= 0 && (n == 0 || d_keys) && version >= 0 && version <= 3, PCC_E_ARG,
              "pcc_octree_encode: bad argument");
  if (version == 0) version = n > PCC_OCTREE_V2_MIN_LEAVES ? 2 : (n >= PCC_OCTREE_V3_MIN_LEAVES ? 3 : 1);
  PCC_REQUIRE(version != 3 || (n >= 2 && n <= 8 * (int64_t)pcc_octree_small_max()), PCC_E_ARG,
              "pcc_octree_encode: blob version 3 takes 2 .. %lld leaves (n=%lld)", 8 * (long long)pcc_octree_small_max(), (long long)n);
  const int64_t zero = 0;
  const int32_t org0[3] = {0, 0, 0};
  if (n == 0) {
    PCC_TRY(pcc_octree_pack(nullptr, &zero, 0, 0, org0, h_out, cap, h_len));
    h_out[1] = (uint8_t)version;
    return PCC_OK;
  }
  uint64_t* ends = (uint64_t*)ctx->pinned;
  PCC_HIP(hipMemcpyAsync(&ends[0], d_keys, 8, hipMemcpyDeviceToHost, ctx->stream));
  PCC_HIP(hipMemcpyAsync(&ends[1], d_keys + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
  PCC_HIP(hipStreamSynchronize(ctx->stream));
  int depth;
  int32_t origin[3];
  octree_root(ends[0], ends[1], key_shift, &depth, origin);
  if (version == 2) return pcc_octree2_encode(ctx, d_keys, n, key_shift, depth, origin, h_out, cap, h_len);
  if (version == 3) {   // parts under the frame's root: one workgroup each on the GPU, one after the other on this thread
    const int K = pcc_octree_parts_for(n);
    PCC_REQUIRE(n <= (int64_t)K * pcc_octree_small_max() / 2, PCC_E_ARG, "pcc_octree_encode: %lld leaves in %d parts", (long long)n, K);
    constexpr int kStride = 20;
    const int64_t cap_occ = n * depth + 4 * K + 4;
    uint8_t* d_buf = nullptr;
    PCC_HIP(hipMalloc((void**)&d_buf, (size_t)cap_occ + 256 + (size_t)K * kStride * 4));
    uint32_t* d_counts = (uint32_t*)(d_buf + (((size_t)cap_occ + 255) & ~(size_t)255));
    std::vector<uint8_t> occ((size_t)cap_occ);
    std::vector<uint32_t> counts((size_t)K * kStride);
    int rc = pcc_octree_parts_async(ctx, d_keys, n, key_shift, depth, K, d_buf, cap_occ, d_counts, kStride);
    if (rc == PCC_OK && (hipMemcpyAsync(occ.data(), d_buf, (size_t)cap_occ, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         hipMemcpyAsync(counts.data(), d_counts, counts.size() * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         hipStreamSynchronize(ctx->stream) != hipSuccess)) {
      pcc_set_error("pcc_octree_encode: reading the parts back failed");
      rc = PCC_E_HIP;
    }
    (void)hipFree(d_buf);
    PCC_TRY(rc);
    std::vector<std::vector<uint8_t>> parts((size_t)K);
    int64_t start = 0;
    for (int k = 0; k < K; ++k) {
      const uint32_t* c = counts.data() + (size_t)k * kStride;
      const int64_t np = (int64_t)c[depth];
      std::vector<int64_t> level_n((size_t)depth, 0);
      int64_t nodes = 0;
      for (int L = 0; L < depth; ++L) { level_n[(size_t)L] = np ? (int64_t)c[L] : 0; nodes += level_n[(size_t)L]; }
      PCC_REQUIRE(start + np <= n && nodes <= np * depth, PCC_E_ARG, "pcc_octree_encode: part %d: %lld leaves behind %lld of %lld, %lld nodes",
                  k, (long long)np, (long long)start, (long long)n, (long long)nodes);
      const size_t off = ((((size_t)start * depth) + 3) & ~(size_t)3) + 4 * (size_t)k;
      parts[(size_t)k].resize((size_t)(64 + 2 * nodes + 16));
      int64_t len = 0;
      PCC_TRY(pcc_octree_pack(np ? occ.data() + off : nullptr, np ? level_n.data() : &zero, np ? depth : 0, np, np ? origin : org0,
                              parts[(size_t)k].data(), (int64_t)parts[(size_t)k].size(), &len));
      parts[(size_t)k].resize((size_t)len);
      start += np;
    }
    PCC_REQUIRE(start == n, PCC_E_ARG, "pcc_octree_encode: the parts hold %lld of %lld leaves", (long long)start, (long long)n);
    return pcc_octree_join_parts(depth, origin, n, parts.data(), K, h_out, cap, h_len);
  }
  uint8_t* d_occ = nullptr;
  PCC_HIP(hipMalloc((void**)&d_occ, (size_t)n * depth));
  std::vector<int64_t> level_n((size_t)depth, 0);
  int rc = pcc_octree_levels(ctx, d_keys, n, key_shift, depth, d_occ, n * depth, level_n.data());
  std::vector<uint8_t> occ;
  if (rc == PCC_OK) {
    int64_t tot = 0;
    for (int64_t v : level_n) tot += v;
    occ.resize((size_t)std::max<int64_t>(tot, 1));
    if (hipMemcpy(occ.data(), d_occ, (size_t)tot, hipMemcpyDeviceToHost) != hipSuccess) rc = PCC_E_HIP;
  }
  (void)hipFree(d_occ);
  PCC_TRY(rc);
  return pcc_octree_pack(occ.data(), level_n.data(), depth, n, origin, h_out, cap, h_len);
}

extern "C" int pcc_octree_encode(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int key_shift, uint8_t* h_out,
                                 int64_t cap, int64_t* h_len) {
  return pcc_octree_encode_version(ctx, d_keys, n, key_shift, 0, h_out, cap, h_len);
}

extern "C" int pcc_octree_blob_version(const uint8_t* h_in, int64_t len) {
  if (!h_in || len < kHeader || h_in[0] != 'O' || h_in[1] < 1 || h_in[1] > 3) {
    pcc_set_error("not an octree blob (len=%lld)", (long long)len);
    return PCC_E_STREAM;
  }
  return h_in[1];
}

extern "C" int pcc_octree_decode_ctx(pcc_ctx* ctx, const uint8_t* h_in, int64_t len, int32_t* h_points, int64_t cap_points,
                                     int64_t* h_n_points) {
  const int v = pcc_octree_blob_version(h_in, len);
  if (v < 0) return v;
  if (v != 2) return pcc_octree_decode(h_in, len, h_points, cap_points, h_n_points);   // versions 1 and 3: host decoders
  return pcc_octree2_decode(ctx, h_in, len, nullptr, h_points, cap_points, h_n_points, nullptr);
}

extern "C" int pcc_octree_decode_dev(pcc_ctx* ctx, const uint8_t* h_in, int64_t len, int32_t* d_points, int64_t cap_points,
                                     int64_t* h_n_points, int64_t* h_level_n) {
  const int v = pcc_octree_blob_version(h_in, len);
  if (v < 0) return v;
  PCC_REQUIRE(ctx, PCC_E_ARG, "pcc_octree_decode_dev: null ctx");
  if (v == 2) return pcc_octree2_decode(ctx, h_in, len, d_points, nullptr, cap_points, h_n_points, h_level_n);
  // version 1: the serial host decoder, then one upload
  int64_t n = 0;
  PCC_TRY(pcc_octree_peek(h_in, len, &n, nullptr, nullptr));
  if (h_n_points) *h_n_points = n;
  int64_t level_n[16];
  for (int L = 0; L < 16; ++L) level_n[L] = 0;
  if (n && d_points) {
    PCC_REQUIRE(cap_points >= n, PCC_E_NOMEM, "pcc_octree_decode_dev: %lld points, capacity %lld", (long long)n, (long long)cap_points);
    std::vector<int32_t> pts;
    PCC_TRY(pcc_octree_unpack_vec(h_in, len, &pts, level_n));
    PCC_REQUIRE((int64_t)pts.size() == 3 * n, PCC_E_STREAM, "pcc_octree_decode_dev: decoded %zu points, announced %lld", pts.size() / 3,
                (long long)n);
    PCC_TRY(o2_stage_reserve(ctx, (size_t)n * 12));
    memcpy(ctx->stage, pts.data(), (size_t)n * 12);
    PCC_HIP(hipMemcpyAsync(d_points, ctx->stage, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    PCC_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (h_level_n)
    for (int L = 0; L < 16; ++L) h_level_n[L] = level_n[L];
  return PCC_OK;
}
