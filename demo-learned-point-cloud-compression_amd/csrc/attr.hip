// attr.hip — lossless per-point attributes (intensity, RGB: uint8 or uint16, 1..4 channels) beside the geometry blobs
// of pcc_octree_encode_frames, coded by the lane-parallel adaptive binary rANS scheme of blob version 2 (lanerans.h).
//
// Attribute blob, version 1 (one per frame; little-endian):
//
//   'A' 1 bpv c | u32 n | u32 payload_len | u32 S | u32 n_chunks | u16 p0[nctx] | u32 words[n_chunks] | chunk payloads
//   (n == 0: the 12 bytes up to payload_len = 0, nothing more)
//   bpv             bytes per value, 1 (uint8) or 2 (uint16); c channels, 1 .. 4
//   chunk k, lane l : points [(64 k + l) S, (64 k + l + 1) S) below n, S c <= 512 values (attr_blob.h attr_layout)
//   payload         = 64 x (state lo, state hi) | u16 len[64] | words of lane 0 | words of lane 1 | ..: every lane has
//                     its own run of 16-bit renormalisation words, in the order its decoder consumes them (as version 2)
//
// A lane codes its points in order, the c channels of a point one after the other.  Value v of channel ch of the run's
// s-th point is predicted from the same channel earlier in the run: pred = 0 (s = 0), v[s-1] (s = 1), else the rounded
// mean (v[s-1] + v[s-2] + 1) >> 1.  The residual wraps to the value width: r = ((v - pred + h) & mask) - h, h = 2^(8 bpv
// - 1) (the decoder's v = (pred + r) & mask), and is binarised as
//   zero flag (r != 0) | sign (r < 0) | prefix: k = floor(log2 |r|) ones and a zero (no zero when k = kmax = 8 bpv - 1)
//   | suffix: bits k-1 .. 0 of |r|
// Context = (channel, bucket of the magnitude of the channel's previous residual in the run (edges 2, 5, 12, 30; 0 for
// the run's first point), position): positions 0 zero flag, 1 sign, 2 + i prefix bit i, 2 + kmax + j suffix bit j, so
// nctx = c x 5 x 16 bpv.  Model: version 2's (12-bit probabilities, adaptation shift 4, every lane's model starts from
// the frame's p0, a counting pass), integer only.  The blob depends on the geometry through n alone.
// tests/attr_ref.py restates the format in numpy.
//
// Attribute blob, version 2 (attr_blob.h has the layout and the rule): the values of every coarser level of detail are a
// prefix of its bytes.  The same coder over the residuals in INTRODUCTION order (k_a2_size / k_a2_scan / k_a2_place), each
// value predicted from the Morton-first point of the next larger cell; a decoder at a level reads the level's bytes,
// decodes its residuals and sums them along every cell's chain (k_a2_walk).  tests/attr2_ref.py restates it in numpy.
//
// Near-lossless, versions 4 and 7 (attr_blob.h has the rule and the layout; e = max_error, q = 2 e + 1): version 1's and
// version 2's streams over the INDICES j of a closed prediction loop instead of wrapped residuals.  Encoder: one pass in
// front of the counting pass runs the loop over the merged values and leaves the j where the PRED = false coder reads
// its residuals — k_a4_quant per (lane run, channel), k_a7_quant per point along its chain of first() — and k_a_stats /
// k_a_enc<false> code them as they code version 2's.  Decoder: k_a_dec<true> returns the j, then k_a4_recon redoes
// the loop of every run, or k_a2_walk<true> sums the chain, scales by q and clamps.  tests/attr_nl_ref.py restates both
// kinds in numpy.
//
// Cross-channel kinds, versions 8, 11, 13 and 14 (attr_blob.h has the rule; the cross forms of 1, 2, 4 and 7 for frames
// of two and more channels): what the plain kind would code for a channel of the mask is coded as its wrapped difference
// to the channel before it.  Encoder: one elementwise pass (k_ax_fwd) in front of the counting pass, over the array the
// PRED = false coder reads; for version 8 it first writes version 1's run residuals there.  Decoder: k_a_dec<true>
// returns the differences, k_ax_inv undoes them in place, and the plain kind's last step follows (k_a8_recon redoes
// version 1's predictor).  Launched for these kinds only.  tests/attr_cross_ref.py restates them in numpy.
//
// Transform-coded, version 19 (attr_blob.h has the rule and the layout; q = qstep): lossy, an integer lifting transform
// over the binary splits of the Morton tree.  Encoder: the coding order at bit granularity (k_at_size / k_at_scan /
// k_at_place), one synchronisation that tells which of the 48 sublevels hold a point, one k_at_lift<true> per such
// sublevel bottom-up over the merged values in place (all frames of the call in one launch), the mean (k_at_mean), and
// k_a_stats / k_a_enc<false> / k_a_pack<.., TR> over the indices.  Decoder (pcc_attr_decode_frames_lod at lod 0, against
// the cells): the same order stage, k_a_dec<true>, k_at_root, k_at_lift<false> top-down, k_at_store.
// tests/attr_transform_ref.py restates the kind in numpy.
//
// Version 21 (attr_blob.h has the rule and the layout): version 19 with a colour word and one step per channel.  The
// frames' steps and colour words travel in a table of their own (aux: 5 words per frame).  Encoder: version 19's
// launches with k_at_lift<true, const int32_t*> and k_a_pack<.., TR, const int32_t*> (the same statements, one argument
// more), and k_ac_fwd between the merge and the order stage of a call with colour = 1.  Decoder: version 19's with
// k_at_lift<false, const int32_t*>, and k_ac_store in place of k_at_store where a frame of the call has colour = 1.
// tests/attr_colour_ref.py restates the kind in numpy.
//
// Version 22 (attr_blob.h has the rule and the layout): version 21 under weights a decoder at a cut can form, its levels
// of detail 0 .. K prefixes of the blob.  Encoder: version 21's launches, behind the order stage k_as_flag (the K-cell
// firsts) and the device-wide scan, k_as_counts (version 2's 16 counts, from the sublevels' counts), k_as_lift<true> in
// place of k_at_lift, and k_a_pack<true, true, false, true, const int32_t*, int> for the head; the K-cell totals are
// sums of the sublevel counts that the order stage's one synchronisation already brings back.  Decoder
// (pcc_attr_decode_frames_lod at lod 0 .. K, against the cells of that lod): the order stage on the cell keys, the lane
// decoder on the level's prefix as version 2's, the cells' counts against the head's, k_as_flag and the scan, k_at_root,
// k_as_lift<false> per occupied sublevel, k_ac_store.  tests/attr_scalable_ref.py restates the kind in numpy.
//
// Versions 19 and 21 under a byte target per frame (pcc_attr_encode_frames_rate; include/pcc.h has the ladder and the
// search): no format of its own.  Merge, colour transform and order stage as above, k_ar_lift (k_at_lift<true> without
// its quantiser: the raw differences and the pairs' weights stay) and k_ar_mean once; then per stage of the search
// k_ar_quant over a table of candidate rows (a frame at a rung) and k_a_stats / k_a_enc<false> over the rows as frames
// of their own; the rows' lengths from their chunks' words; k_ar_gather and k_a_pack<.., TR[, const int32_t*]> over the
// winners alone.  tests/attr_rate_ref.py restates ladder and search in numpy.
//
// Versions 25 and 26 (attr_blob.h has the rule): version 2's stream over the residuals of a predictor from up to three
// Morton-first points of the coarser cells around a point.  The kernels are attr_nbr.h's.  Encoder: version 2's launches
// with k_an_place in place of k_a2_place (and k_ax_fwd<false> for a frame of version 26); k_a_pack writes version 2's /
// 11's head and a_enc_emit sets the version byte.  Decoder (pcc_attr_decode_frames_lod): the order stage with k_an_plan in
// place of k_a2_place, k_a_dec<true> (k_ax_inv), then k_an_recon once per occupied size of introduction, 16 down to 0.
// tests/attr_nbr_ref.py restates both kinds in numpy.
//
// Versions 28 and 31 (attr_blob.h has the rule): version 7's stream over the indices of the same predictor in a closed
// loop, over decoded values.  The kernels are attr_nbr.h's.  Encoder: version 7's launches with k_anl_plan in place of
// k_a2_place<true, true> and k_anl_quant, once per size of introduction 16 down to 0, in place of k_a7_quant (k_ax_fwd<false>
// for a frame of version 31); k_a_pack writes version 7's / 14's head and a_enc_emit sets the version byte.  Decoder: the
// launches of 25 / 26 with k_anl_recon.  tests/attr_nbr_nl_ref.py restates both kinds in numpy.
//
// Host side: the kinds share one encode sequence (a_encode_frames over an AEncKind, the entry point's kind resolved
// once) and one decode-call skeleton (ADecCall: accounting, rows, layout, upload, status) under the three decoders, each
// of which keeps its parser, its side tables, its arena arrays and its kernels; DESIGN.md, "attr.hip: one encode path,
// shared decode helpers", "attr.hip: the host code of kinds 8 to 21, folded" and "attr.hip: version 22 and the byte
// budget, folded".  The two encode entry points (a_encode_frames, pcc_attr_encode_frames_rate) share their front
// (a_enc_front over an AEncPlan) and their tail (a_enc_emit).
#include "common.h"
#include "lanerans.h"
#include "attr_blob.h"

#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

namespace {

constexpr uint32_t kAL = 1u << 16;
constexpr int kAMaxCtx = 4 * kAttrBuckets * 32;   // c = 4, uint16

__host__ __device__ inline int a_bucket(uint32_t m) { return (m >= 2) + (m >= 5) + (m >= 12) + (m >= 30); }

// the decisions of residual r in coding order: emit(position, bit)
template <typename Emit>
__device__ __forceinline__ void a_binarise(int r, int kmax, Emit emit) {
  emit(0, r != 0 ? 1u : 0u);
  if (r == 0) return;
  emit(1, r < 0 ? 1u : 0u);
  const uint32_t m = (uint32_t)(r < 0 ? -r : r);
  const int k = 31 - __clz(m);
  for (int i = 0; i < kmax; ++i) {
    const uint32_t bit = i < k ? 1u : 0u;
    emit(2 + i, bit);
    if (!bit) break;
  }
  for (int j = k - 1; j >= 0; --j) emit(2 + kmax + j, (m >> j) & 1u);
}

// the predictor inside a lane's run (versions 1 and 4) from the previous two values a = v[s-1], b = v[s-2]: nothing, a,
// their rounded mean.  T = uint32_t (values) or int (reconstructions: the shift is arithmetic)
template <typename I, typename T>
__host__ __device__ __forceinline__ T a_pred(I s, T a, T b) {
  return s == 0 ? (T)0 : (s == 1 ? a : (a + b + 1) >> 1);
}

// value ch of a row of bpv-byte little-endian values at p: zero-extended, sign-extended, stored.  Indexed as the
// kernels always indexed (p[ch] | p[2 ch], p[2 ch + 1]; the store's first byte at p[bpv ch]) and not through p + bpv ch:
// that form compiles k_a_merge and k_a2_walk<false> to other instructions than they have had.  ch = 0: one value at p
__device__ __forceinline__ uint32_t a_load(const uint8_t* p, int bpv, int ch = 0) {
  return bpv == 1 ? (uint32_t)p[ch] : (uint32_t)p[2 * ch] | ((uint32_t)p[2 * ch + 1] << 8);
}
__device__ __forceinline__ int a_load_s(const uint8_t* p, int bpv, int ch = 0) {
  return bpv == 1 ? (int)(int8_t)p[ch] : (int)(int16_t)((uint32_t)p[2 * ch] | ((uint32_t)p[2 * ch + 1] << 8));
}
__device__ __forceinline__ void a_store(uint8_t* p, int bpv, uint32_t val, int ch = 0) {
  p[bpv * ch] = (uint8_t)val;
  if (bpv == 2) p[2 * ch + 1] = (uint8_t)(val >> 8);
}

// residual of point i (run position s) in channel ch of a frame's merged values v[n][c]; PRED = false (version 2): v
// holds the residuals themselves, wrapped to the value width, and the lane codes what it is handed
template <bool PRED = true>
__device__ __forceinline__ int a_resid(const uint16_t* __restrict__ v, int64_t i, int64_t s, int c, int ch, uint32_t mask, int half) {
  const uint32_t x = v[i * c + ch];
  if constexpr (!PRED) return (int)((x + (uint32_t)half) & mask) - half;
  const uint32_t a = s >= 1 ? v[(i - 1) * c + ch] : 0u, b = s >= 2 ? v[(i - 2) * c + ch] : 0u;
  const uint32_t pred = a_pred(s, a, b);
  return (int)((x - pred + (uint32_t)half) & mask) - half;
}

// ---- encoder -----------------------------------------------------------------------------------------------------
// one frame (>= 1 point) of an encode call
struct AFrame {
  int64_t in_off;            // its values as they came: bytes into the call's input
  int64_t row0, rows;        // its input rows among the call's sorted keys
  int64_t u0, n;             // its points: runs [u0, u0 + n) of the call's run starts
  int64_t val_off;           // its merged values (uint16 [n][c]) in the call's merged array
  int64_t rec_off;           // 16-bit words of records (and of word regions) of the frames in front of it
  int64_t out_off, out_cap;  // its blob in the output staging: offset, bound
  int32_t S, nc, cb, sb, sn, mb;   // chunks: S, count, first (of the call); stats blocks: first, count; merge blocks
  int32_t c, bpv, nctx, ctx_off, T;   // T: records (and words) a lane may leave, S c 16 bpv
  int32_t e;                          // max_error of versions 4 and 7 (in what was padding: no other field moves)
};
static_assert(sizeof(AFrame) == 120, "AFrame: the rows of versions 1 and 2 keep their size");

// index of the quantised prediction error d = v - p: sgn(d) floor((|d| + e) / q), q = 2 e + 1
__device__ __forceinline__ int a_quant(int d, int e, int q) {
  const int m = (int)((uint32_t)((d < 0 ? -d : d) + e) / (uint32_t)q);
  return d < 0 ? -m : m;
}

// merged value of every point: the rounded mean (sum + cnt / 2) / cnt of the run of equal keys behind it (order-free).
// Frame f owns blocks [mb, mb + ceil(n / 256)); perm[t] is the input row of sorted key t, runs[u] the first sorted key
// of run u, n_keys the call's key count.
__global__ __launch_bounds__(256) void k_a_merge(const uint8_t* __restrict__ in, const AFrame* __restrict__ tab, int nf,
                                                 const uint32_t* __restrict__ perm, const uint32_t* __restrict__ runs,
                                                 int64_t n_runs, int64_t n_keys, uint16_t* __restrict__ merged) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].mb; });
  const AFrame& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.mb) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const int c = h.c, bpv = h.bpv;
  const int64_t u = h.u0 + i;
  const int64_t t0 = runs[u], t1 = u + 1 < n_runs ? (int64_t)runs[u + 1] : n_keys;
  uint64_t sum[4] = {0, 0, 0, 0};
  int64_t cnt = 0;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t row = (int64_t)perm[t] - h.row0;
    if (row < 0 || row >= h.rows) continue;   // not a row of this frame: the keys were not sorted frame by frame
    const uint8_t* p = in + h.in_off + row * c * bpv;
    for (int ch = 0; ch < c; ++ch)
      sum[ch] += a_load(p, bpv, ch);
    ++cnt;
  }
  if (cnt == 0) cnt = 1;
  for (int ch = 0; ch < c; ++ch) merged[h.val_off + i * c + ch] = (uint16_t)((sum[ch] + (uint64_t)(cnt / 2)) / (uint64_t)cnt);
}

// Version 4: the closed loop of every (lane run, channel) over the frame's merged values, frame = blockIdx.y.  The
// predictor is built from the reconstructions v^ = p + j q (unclamped), as the decoder will build it; index j of point
// i, channel ch goes to idx[val_off + i c + ch] wrapped to the value width, where the PRED = false coder reads it.
// One thread per (run, channel), channel fastest: the chain is a few integer operations per value and the loads do not
// depend on it, so they are issued eight values ahead; the threads of a run's channels share their cache lines.
__global__ __launch_bounds__(256) void k_a4_quant(const uint16_t* __restrict__ merged, const AFrame* __restrict__ tab,
                                                  uint16_t* __restrict__ idx) {
  const AFrame& h = tab[blockIdx.y];
  const int c = h.c, e = h.e, q = 2 * e + 1;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t base = t / c * h.S;
  const int ch = (int)(t % c);
  if (base >= h.n) return;
  const int npts = (int)std::min<int64_t>(h.S, h.n - base);
  const uint32_t mask = (1u << (8 * h.bpv)) - 1u;
  const uint16_t* v = merged + h.val_off + base * c + ch;
  uint16_t* o = idx + h.val_off + base * c + ch;
  int a = 0, b = 0;   // v^[s - 1], v^[s - 2]
  for (int s0 = 0; s0 < npts; s0 += 8) {
    int x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = s0 + k < npts ? (int)v[(int64_t)(s0 + k) * c] : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int s = s0 + k;
      if (s < npts) {
        const int p = a_pred(s, a, b);
        const int j = a_quant(x[k] - p, e, q);
        b = a;
        a = p + j * q;
        o[(int64_t)s * c] = (uint16_t)((uint32_t)j & mask);
      }
    }
  }
}

// zeros and ones seen per context over the whole frame: cnt[2 (ctx_off + ctx) + bit]; frame f takes blocks [sb, sb + sn)
template <bool PRED>
__global__ __launch_bounds__(256) void k_a_stats(const uint16_t* __restrict__ merged, const AFrame* __restrict__ tab, int nf,
                                                 uint32_t* __restrict__ cnt_all) {
  __shared__ uint32_t s_cnt[2 * kAMaxCtx];
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].sb; });
  const AFrame& h = tab[f];
  const uint16_t* v = merged + h.val_off;
  const int c = h.c, P = attr_positions(h.bpv), kmax = 8 * h.bpv - 1, half = 1 << kmax;
  const uint32_t mask = (1u << (8 * h.bpv)) - 1u;
  const int64_t b = (int64_t)blockIdx.x - h.sb, nb = h.sn, S = h.S;
  for (int i = threadIdx.x; i < 2 * h.nctx; i += blockDim.x) s_cnt[i] = 0u;
  __syncthreads();
  for (int64_t i = b * blockDim.x + threadIdx.x; i < h.n; i += nb * blockDim.x) {
    const int64_t s = i % S;
    for (int ch = 0; ch < c; ++ch) {
      const int bk = s == 0 ? 0 : a_bucket((uint32_t)abs(a_resid<PRED>(v, i - 1, s - 1, c, ch, mask, half)));
      const int cbase = (ch * kAttrBuckets + bk) * P;
      a_binarise(a_resid<PRED>(v, i, s, c, ch, mask, half), kmax,
                 [&](int pos, uint32_t bit) { atomicAdd(&s_cnt[2 * (cbase + pos) + bit], 1u); });
    }
  }
  __syncthreads();
  uint32_t* cnt = cnt_all + 2 * (int64_t)h.ctx_off;
  for (int i = threadIdx.x; i < 2 * h.nctx; i += blockDim.x)
    if (s_cnt[i]) atomicAdd(&cnt[i], s_cnt[i]);
}

// One wave per chunk (dynamic LDS: the reciprocal table, then the models [ctx][lane] with a dummy row).  Forward pass:
// every lane walks its points with its own model and leaves one record per coded decision (probability of a one |
// bit << 15) in rec[chunk][k][lane]; backward pass: the lane's rANS steps over its records in reverse (lockstep to the
// wave's longest list, the rest masked), every renormalisation word stored downwards from the end of the lane's own
// T-word region of `work` ([chunk][lane][T]: a step emits at most one word).  states / lens / words_out as k_o2_enc.
template <bool PRED>
__global__ __launch_bounds__(64) void k_a_enc(const uint16_t* __restrict__ merged, const AFrame* __restrict__ tab, int nf,
                                              const uint32_t* __restrict__ cnt_all, uint16_t* __restrict__ rec_all,
                                              uint16_t* __restrict__ work_all, uint16_t* __restrict__ states,
                                              uint16_t* __restrict__ lens, uint32_t* __restrict__ words_out,
                                              uint16_t* __restrict__ p0_all) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
  uint32_t* s_rcp = s_dyn;
  uint16_t* s_model = reinterpret_cast<uint16_t*>(s_dyn + 4096);
  const int lane = threadIdx.x;
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].cb; });
  const AFrame& h = tab[f];
  const int64_t cg = blockIdx.x, ck = cg - h.cb;
  const int c = h.c, P = attr_positions(h.bpv), kmax = 8 * h.bpv - 1, half = 1 << kmax, nctx = h.nctx, T = h.T;
  const uint32_t mask = (1u << (8 * h.bpv)) - 1u;
  const uint32_t* cnt = cnt_all + 2 * (int64_t)h.ctx_off;
  const uint16_t* v = merged + h.val_off;
  for (int ctx = lane; ctx < nctx; ctx += kLanes) {
    const uint32_t p = o2_p0(cnt[2 * ctx], cnt[2 * ctx + 1]);
    if (ck == 0) p0_all[h.ctx_off + ctx] = (uint16_t)p;
    for (int l = 0; l < kLanes; ++l) s_model[ctx * kLanes + l] = (uint16_t)p;
  }
  lr_load_rcp(s_rcp, lane);
  __syncthreads();
  uint16_t* rec = rec_all + h.rec_off + ck * (int64_t)kLanes * T;
  const int64_t base = (ck * kLanes + lane) * h.S;
  const int64_t npts = std::max<int64_t>(0, std::min<int64_t>(h.S, h.n - base));
  int K = 0;
  uint32_t bk = 0;   // 4 bits per channel: the bucket of its previous residual
  for (int64_t s = 0; s < npts; ++s) {
    for (int ch = 0; ch < c; ++ch) {
      const int r = a_resid<PRED>(v, base + s, s, c, ch, mask, half);
      const int cbase = (ch * kAttrBuckets + (int)((bk >> (4 * ch)) & 15u)) * P;
      a_binarise(r, kmax, [&](int pos, uint32_t bit) {
        const int at = (cbase + pos) * kLanes + lane;
        const uint32_t p = s_model[at];
        rec[(int64_t)K * kLanes + lane] = (uint16_t)(p | (bit << 15));
        ++K;
        s_model[at] = (uint16_t)o2_adapt(p, bit);
      });
      bk = (bk & ~(15u << (4 * ch))) | ((uint32_t)a_bucket((uint32_t)abs(r)) << (4 * ch));
    }
  }
  __syncthreads();   // the records of the wave before they are read back

  // backward pass
  int kmax_w = K;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) kmax_w = std::max(kmax_w, __shfl_xor(kmax_w, d, 64));
  constexpr int kAhead = 8;
  const int kr = (kmax_w + kAhead - 1) / kAhead * kAhead;
  uint16_t* reg_w = reinterpret_cast<uint16_t*>(uniform_u64((uint64_t)(work_all + h.rec_off + ck * (int64_t)kLanes * T)));
  const __amdgpu_buffer_rsrc_t reg_rs = __builtin_amdgcn_make_buffer_rsrc(reg_w, 0, (int)(uint32_t)(kLanes * T * 2), 0x00027000);
  int wp = T;   // words [wp, T) of the lane's region are written
  const uint32_t lane_off = (uint32_t)lane * (uint32_t)T * 2u;
  uint32_t x = kAL;
  auto fetch = [&](int t) -> uint32_t { return rec[(int64_t)(t < 0 ? 0 : (t < T ? t : T - 1)) * kLanes + lane]; };
  uint32_t R[kAhead];
#pragma unroll
  for (int d = 0; d < kAhead; ++d) R[d] = fetch(kr - 1 - d);
  for (int t0 = kr - 1; t0 >= 0; t0 -= kAhead) {
#pragma unroll
    for (int d = 0; d < kAhead; ++d) {
      const int t = t0 - d;
      const uint32_t r = t < K ? R[d] : 0u;   // records beyond the lane's own count: nothing coded
      R[d] = fetch(t - kAhead);
      const uint32_t p1 = r & 0xFFFu, bit = r >> 15;
      const bool act = r != 0u;
      const uint32_t freq = bit ? p1 : 4096u - p1, start = bit ? 4096u - p1 : 0u, rcp = s_rcp[freq & 4095u];
      const bool need = act && x >= (freq << 20);
      wp -= need ? 1 : 0;
      __builtin_amdgcn_raw_buffer_store_b16((unsigned short)x, reg_rs, need ? lane_off + (uint32_t)wp * 2u : 0xFFFFFFF0u, 0, 0);
      x = need ? x >> 16 : x;
      const uint32_t q0 = __umulhi(x, rcp);
      const uint32_t r0 = x - q0 * freq;
      const bool over = r0 >= freq;
      const uint32_t qd = q0 + (over ? 1u : 0u), rem = r0 - (over ? freq : 0u);
      x = act ? (qd << 12) + rem + start : x;
    }
  }
  states[cg * 2 * kLanes + 2 * lane] = (uint16_t)x;
  states[cg * 2 * kLanes + 2 * lane + 1] = (uint16_t)(x >> 16);
  const uint32_t len = (uint32_t)(T - wp);
  lens[cg * kLanes + lane] = (uint16_t)len;
  uint32_t tot = len;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) tot += (uint32_t)__shfl_xor((int)tot, d, 64);
  if (lane == 0) words_out[cg] = 3u * kLanes + tot;
}

// version 21's table of steps and colour words (5 words per frame: q[4], colour), the one argument more of the
// kernels that read it (Aux = const int32_t*); the instantiations without it keep their arguments
__device__ __forceinline__ const int32_t* a_aux() { return nullptr; }
__device__ __forceinline__ const int32_t* a_aux(const int32_t* p) { return p; }
// version 22: the sender's K behind the table (Aux = const int32_t*, int)
__device__ __forceinline__ const int32_t* a_aux(const int32_t* p, int) { return p; }
__device__ __forceinline__ int a_aux_k(const int32_t*, int k) { return k; }

// the blobs, assembled where `out_all` points (pinned host memory), frame f's at out_off: frame f owns workgroups
// [cb + f, cb + f + nc + 1) — workgroup k < nc of them moves chunk k, workgroup nc writes the header; len_out[f] =
// bytes, or -1 (out_cap).  V2: the head of attribute blob version 2, with the frame's 16 values-per-level counts
// (cells_all[16 f + k], attr_blob.h) and the sender's level of detail.  NL: the heads of versions 4 / 7, the frame's
// max_error behind payload_len and everything else one word later.  XC (a call with cross-channel frames): frame f with
// cross_all[f] = m != 0 gets the cross form of the version byte and its mask above the channels of byte 3.  TR (with NL
// and without V2): version 19's head — version 4's with q = h.e where e stands, byte 19 and the slod nibble.  TC (with
// TR): version 21's head — byte 21, and where q stands the colour word and the frame's c steps (aux_all[5 f + 4] and
// aux_all[5 f + ch], a_aux(aux...)), everything else c words later.  SC (with V2, NL, TR and TC; Aux = const int32_t*,
// int): version 22's head — byte 22, K behind the steps and version 2's 16 counts behind K
template <bool V2, bool NL = false, bool XC = false, bool TR = false, typename... Aux>
__global__ __launch_bounds__(256) void k_a_pack(const uint16_t* __restrict__ work_all, const AFrame* __restrict__ tab, int nf,
                                                const uint16_t* __restrict__ states_all, const uint16_t* __restrict__ lens_all,
                                                const uint32_t* __restrict__ words_all, const uint16_t* __restrict__ p0_all,
                                                uint8_t* __restrict__ out_all, long long* __restrict__ len_out,
                                                const uint32_t* __restrict__ cells_all, int slod,
                                                const int32_t* __restrict__ cross_all, Aux... aux) {
  constexpr bool TC = sizeof...(Aux) > 0, SC = sizeof...(Aux) > 1;
  __shared__ unsigned long long s_sum[256];
  __shared__ uint32_t s_off[kLanes + 1];
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].cb + i; });
  const AFrame& h = tab[f];
  const int64_t k = (int64_t)blockIdx.x - h.cb - f, nc = h.nc, cap = h.out_cap;
  const uint32_t* words = words_all + h.cb;
  uint8_t* out = out_all + h.out_off;
  unsigned long long part = 0;
  const int64_t upto = k < nc ? k : nc;
  for (int64_t j = threadIdx.x; j < upto; j += blockDim.x) part += words[j];
  s_sum[threadIdx.x] = part;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
    __syncthreads();
  }
  const unsigned long long before = s_sum[0];
  constexpr int X0 = NL ? 1 : 0;
  int X = X0;
  if constexpr (TC) X = 1 + h.c + (SC ? 1 : 0);
  const unsigned long long head = (unsigned long long)((V2 ? kAttr2Head : kAttrHead + 8) + 4 * X) + 2ull * h.nctx + 4ull * nc;
  if (k == nc) {
    const unsigned long long total = head + before * 2;
    const bool fits = (long long)total <= cap;
    if (threadIdx.x == 0) {
      len_out[f] = fits ? (long long)total : -1;
      __threadfence_system();
    }
    if (!fits) return;
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
    if (threadIdx.x == 0) {
      o32[0] = (uint32_t)'A' | ((NL ? (V2 ? 7u : 4u) : (V2 ? 2u : 1u)) << 8) | ((uint32_t)(h.bpv | (V2 ? slod << 4 : 0)) << 16) | ((uint32_t)h.c << 24);
      if constexpr (XC) {
        const uint32_t m = (uint32_t)cross_all[f];
        if (m) out[1] = (uint8_t)attr_version(V2, NL, true), out[3] = (uint8_t)((uint32_t)h.c | (m << 4));
      }
      if constexpr (TR) out[1] = (uint8_t)kAttrTVersion, out[2] = (uint8_t)(h.bpv | (slod << 4));
      o32[1] = (uint32_t)h.n;
      o32[2] = (uint32_t)(total - kAttrHead);
      if constexpr (TC) {
        out[1] = (uint8_t)(SC ? kAttrSVersion : kAttrCVersion);
        const int32_t* aux_all = a_aux(aux...);
        o32[3] = (uint32_t)aux_all[5 * f + 4];
        for (int ch = 0; ch < h.c; ++ch) o32[4 + ch] = (uint32_t)aux_all[5 * f + ch];
        if constexpr (SC) o32[4 + h.c] = (uint32_t)a_aux_k(aux...);
      } else if constexpr (NL) {
        o32[3] = (uint32_t)h.e;
      }
      o32[(V2 ? 19 : 3) + X] = (uint32_t)h.S;
      o32[(V2 ? 20 : 4) + X] = (uint32_t)h.nc;
    }
    if constexpr (V2) {
      if (threadIdx.x < 16) o32[3 + X + threadIdx.x] = cells_all[16 * f + threadIdx.x];
    }
    uint16_t* o16 = reinterpret_cast<uint16_t*>(o32 + (V2 ? 21 : 5) + X);
    for (int i = threadIdx.x; i < h.nctx; i += blockDim.x) o16[i] = p0_all[h.ctx_off + i];
    uint32_t* wt = reinterpret_cast<uint32_t*>(o16 + h.nctx);
    for (int64_t j = threadIdx.x; j < nc; j += blockDim.x) wt[j] = words[j];
    return;
  }
  if ((long long)(head + (before + words[k]) * 2) > cap) return;   // the header block reports it
  uint16_t* dst = reinterpret_cast<uint16_t*>(out + head) + before;
  lr_stage_chunk(work_all + h.rec_off, k, h.T, states_all + h.cb * 2 * kLanes, lens_all + h.cb * kLanes, s_off, dst);
}

// ---- decoder -----------------------------------------------------------------------------------------------------
// status (int32) per frame: OR of 1 = a lane ran out of words or did not use all of its words, 4 = a lane's final
// state is not the encoder's initial one
//
// one frame (>= 1 point) of a decode call
struct ADFrame {
  int64_t body_off;               // p0 | chunk table | payload of its blob in the call's uploaded bodies (4-aligned)
  int64_t table_off, payload_off; // from body_off
  int64_t n, out_off;             // points; its values in the output: bytes
  int32_t S, nc, cb, c, bpv, nctx;
  // version 2 at a level of detail: n stays the whole blob's values, nc counts the chunks the level needs, n_dec its
  // values (the first n_dec of the introduction sequence), last_words the words of chunk nc - 1 that were uploaded.
  // Versions 1 and 4: n_dec = n, every chunk whole.  max_error: the e of versions 4 and 7
  int64_t n_dec;
  int32_t last_words, max_error;
};

// avail: the words of the chunk that are there to read (cw; fewer in the last chunk of a level of detail).  V2 (the
// rows of versions 2, 4 and 7): no prediction inside the run, the values written are what was coded (version 2: the
// residuals, in introduction order); a lane whose run the level cuts short stops there and is exempt from the end
// checks, a lane behind it does nothing.
template <bool IN_LDS, bool V2>
__device__ __forceinline__ void a_decode_chunk(uint16_t* s_model, const uint16_t* __restrict__ s_words,
                                               const uint16_t* __restrict__ p /* the chunk in the stream */, uint32_t cw,
                                               uint32_t avail, const ADFrame& h, int64_t ck, int lane, uint8_t* __restrict__ out, int& bad) {
  uint32_t x = (uint32_t)p[2 * lane] | ((uint32_t)p[2 * lane + 1] << 16);
  const uint32_t my_len = p[2 * kLanes + lane];
  uint32_t incl = my_len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
    incl += lane >= d ? o : 0u;
  }
  const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
  if (3u * kLanes + total != cw) {   // wave-uniform
    bad |= 1;
    return;
  }
  const uint32_t rbase = 3u * kLanes + incl - my_len, rend = rbase + my_len;
  uint32_t pos = rbase;
  auto word_at = [&](uint32_t i) -> uint32_t {
    const uint32_t ic = i < avail ? i : avail - 1;   // a lane at the end of the chunk's last run looks one word too far: never used
    if constexpr (IN_LDS) return s_words[ic];
    return p[ic];
  };
  uint32_t nextw = word_at(pos);
  const int c = h.c, bpv = h.bpv, P = attr_positions(bpv), kmax = 8 * bpv - 1;
  const uint32_t mask = (1u << (8 * bpv)) - 1u;
  const int64_t base = (ck * kLanes + lane) * h.S;
  int npts = (int)std::max<int64_t>(0, std::min<int64_t>(h.S, h.n - base));
  bool whole = true;
  if constexpr (V2) {
    const int cut = (int)std::max<int64_t>(0, std::min<int64_t>(h.S, h.n_dec - base));
    whole = cut == npts;
    npts = cut;
  }
  const int a_dummy = h.nctx * kLanes + lane;
  // the lane's place in its binarisation: phase 0 zero flag, 1 sign, 2 prefix (i ones so far), 3 suffix (i bits left)
  int s = 0, ch = 0, phase = 0, i = 0;
  uint32_t acc = 0, neg = 0, bk = 0;
  uint64_t v1 = 0, v2 = 0;   // the channels' previous two values, 16 bits each
  while (__ballot(s < npts)) {
    const bool act = s < npts;
    const int cpos = phase == 0 ? 0 : (phase == 1 ? 1 : (phase == 2 ? 2 + i : 1 + kmax + i));
    const int at = act ? ((ch * kAttrBuckets + (int)((bk >> (4 * ch)) & 15u)) * P + cpos) * kLanes + lane : a_dummy;
    const uint32_t p1 = s_model[at];
    const uint32_t cum = x & 4095u;
    const uint32_t bit = cum >= 4096u - p1 ? 1u : 0u;
    const uint32_t start = bit ? 4096u - p1 : 0u, freq = bit ? p1 : 4096u - p1;
    const uint32_t xn = freq * (x >> 12) + cum - start;
    x = act ? xn : x;
    s_model[at] = (uint16_t)o2_adapt(p1, bit);
    const bool need = act && x < kAL;
    bad |= (need && pos >= rend) ? 1 : 0;
    x = need ? (x << 16) | nextw : x;
    pos += need ? 1u : 0u;
    nextw = word_at(pos);   // every step (the same word again when nothing was consumed): no branch
    // the next place in the binarisation, and whether the value is complete (its magnitude m)
    bool done = false;
    uint32_t m = 0;
    int nphase = phase, ni = i;
    uint32_t nacc = acc;
    if (phase == 0) {
      done = bit == 0u;
      nphase = 1;
    } else if (phase == 1) {
      neg = bit;
      nphase = 2;
      ni = 0;
    } else if (phase == 2) {
      const int k = i + (int)bit;
      if (bit == 0u || k == kmax) {
        done = k == 0;
        m = 1;
        nphase = 3;
        ni = k;
        nacc = 1;
      } else {
        ni = k;
      }
    } else {
      nacc = 2 * acc + bit;
      ni = i - 1;
      done = ni == 0;
      m = nacc;
    }
    phase = nphase;
    i = ni;
    acc = nacc;
    if (act && done) {
      const uint32_t sh = 16u * (uint32_t)ch;
      const uint32_t a = (uint32_t)(v1 >> sh) & 0xFFFFu, b = (uint32_t)(v2 >> sh) & 0xFFFFu;
      const uint32_t pred = V2 ? 0u : a_pred(s, a, b);
      const uint32_t val = (pred + (neg ? 0u - m : m)) & mask;
      const int64_t o = ((base + s) * c + ch) * bpv;
      a_store(out + o, bpv, val);
      v2 = (v2 & ~(0xFFFFull << sh)) | ((uint64_t)a << sh);
      v1 = (v1 & ~(0xFFFFull << sh)) | ((uint64_t)val << sh);
      bk = (bk & ~(15u << (4 * ch))) | ((uint32_t)a_bucket(m) << (4 * ch));
      phase = 0;
      neg = 0;
      ++ch;
      if (ch == c) {
        ch = 0;
        ++s;
      }
    }
  }
  if (whole && pos != rend) bad |= 1;   // every word of the run consumed
  if (whole && x != kAL) bad |= 4;      // back at the encoder's initial state
}

// block = chunk of the call: frame f owns blocks [cb, cb + nc).  Dynamic LDS: the models (nctx_max + 1 rows of 64),
// then lds_words words for a chunk's payload
template <bool V2>
__global__ __launch_bounds__(64) void k_a_dec(const uint8_t* __restrict__ bodies, const ADFrame* __restrict__ tab, int nf,
                                              int model_rows, int lds_words, uint8_t* __restrict__ out_all,
                                              int32_t* __restrict__ status_all) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
  uint16_t* s_model = reinterpret_cast<uint16_t*>(s_dyn);
  uint16_t* s_words = s_model + (int64_t)model_rows * kLanes;
  const int lane = threadIdx.x;
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].cb; });
  const ADFrame& h = tab[f];
  const int64_t ck = (int64_t)blockIdx.x - h.cb;
  const uint8_t* body = bodies + h.body_off;
  const uint16_t* p0 = reinterpret_cast<const uint16_t*>(body);
  const uint32_t* table = reinterpret_cast<const uint32_t*>(body + h.table_off);
  const uint16_t* payload = reinterpret_cast<const uint16_t*>(body + h.payload_off);
  for (int ctx = 0; ctx < h.nctx; ++ctx) s_model[ctx * kLanes + lane] = p0[ctx];
  unsigned long long before = 0;
  for (int64_t j = lane; j < ck; j += kLanes) before += table[j];
  for (int d = 32; d >= 1; d >>= 1) before += __shfl_xor(before, d, 64);
  const uint32_t cw = (uint32_t)__builtin_amdgcn_readfirstlane((int)table[ck]);
  const uint16_t* p = payload + before;
  int bad = 0;
  uint32_t avail = cw;
  if constexpr (V2) {
    if (ck == h.nc - 1) avail = (uint32_t)h.last_words;
  }
  if (avail <= (uint32_t)lds_words) {
    for (uint32_t i = lane; i < avail; i += kLanes) s_words[i] = p[i];
    __syncthreads();
    a_decode_chunk<true, V2>(s_model, s_words, p, cw, avail, h, ck, lane, out_all + h.out_off, bad);
  } else {
    a_decode_chunk<false, V2>(s_model, s_words, p, cw, avail, h, ck, lane, out_all + h.out_off, bad);
  }
  const unsigned long long b1 = __ballot((bad & 1) != 0), b4 = __ballot((bad & 4) != 0);
  if (lane == 0 && (b1 | b4) != 0ull) atomicOr(status_all + f, (b1 ? 1 : 0) | (b4 ? 4 : 0));
}

// Version 4, behind k_a_dec<true>: the decoder's side of k_a4_quant's loop, frame = blockIdx.y, one thread per (lane
// run, channel).  idx_all / out_all: the frames' [n][c] values of bpv bytes at out_off, the indices j as the coder
// wrapped them / the values clamped to the value width.  An encoder's reconstruction never leaves [-e, mask + e]:
// status |= 16 where one does (and the loop goes on from the nearest value inside).
__global__ __launch_bounds__(256) void k_a4_recon(const ADFrame* __restrict__ tab, const uint8_t* __restrict__ idx_all,
                                                  uint8_t* __restrict__ out_all, int32_t* __restrict__ status_all) {
  const ADFrame& h = tab[blockIdx.y];
  const int c = h.c, bpv = h.bpv, e = h.max_error, q = 2 * e + 1;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t base = t / c * h.S;
  const int ch = (int)(t % c);
  if (base >= h.n) return;
  const int npts = (int)std::min<int64_t>(h.S, h.n - base);
  const int mask = (1 << (8 * bpv)) - 1;
  const uint8_t* r = idx_all + h.out_off + (base * c + ch) * bpv;
  uint8_t* o = out_all + h.out_off + (base * c + ch) * bpv;
  int a = 0, b = 0;   // v^[s - 1], v^[s - 2]
  bool bad = false;
  for (int s = 0; s < npts; ++s) {
    const int64_t at = (int64_t)s * c * bpv;
    const int j = a_load_s(r + at, bpv);
    const int p = a_pred(s, a, b);
    int64_t x = (int64_t)p + (int64_t)j * q;
    if (x < -e || x > mask + e) {
      bad = true;
      x = x < -e ? -e : mask + e;
    }
    b = a;
    a = (int)x;
    const int val = a < 0 ? 0 : (a > mask ? mask : a);
    a_store(o + at, bpv, (uint32_t)val);
  }
  if (bad) atomicOr(status_all + blockIdx.y, 16);
}

// ---- version 2: the introduction order ----------------------------------------------------------------------------
// (attr_blob.h states the rule.)  One row per frame (>= 1 point) of a call, for the encoder over the call's distinct
// sorted keys and for the decoder over the cells its geometry decode left in HBM: frame f's points are [pt0, pt0 + n)
// of the call's, it owns blocks [blk0, blk0 + ceil(n / 256)) of the three kernels below.  shift: the encoder's
// key_shift (keys of cells: a multiple of 3 low bits are zero), the decoder's level of detail (cells p >> lod, biased
// by 32768 >> lod, lod counting from the points the sender had).
struct A2Order {
  int64_t pt0, n;
  int32_t blk0, shift;
};
constexpr int kA2Bins = 17;   // sizes of introduction 0 .. 16

__device__ __forceinline__ uint64_t a2_cell_key(const int32_t* __restrict__ cells, int64_t i, int bias) {
  const int32_t* q = cells + 3 * i;
  return (pcc_spread3((uint32_t)(q[0] + bias)) << 2) | (pcc_spread3((uint32_t)(q[1] + bias)) << 1) | pcc_spread3((uint32_t)(q[2] + bias));
}

// s(i) of every point, its rank among the points of its block with the same s (packed[i] = s << 8 | rank) and the
// block's count per s (hist[17 block + s]); FROM_CELLS: the keys of the cells are computed here and kept (keys_out)
template <bool FROM_CELLS>
__global__ __launch_bounds__(256) void k_a2_size(const void* __restrict__ src, const A2Order* __restrict__ tab, int nf,
                                                 uint64_t* __restrict__ keys_out, uint16_t* __restrict__ packed,
                                                 uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_cnt[4][kA2Bins];
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  const bool act = i < h.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bin = kA2Bins;   // none
  if (act) {
    uint64_t key, prev = 0;
    int sh = 0;
    if constexpr (FROM_CELLS) {
      const int32_t* cells = static_cast<const int32_t*>(src);
      const int bias = 32768 >> h.shift;
      key = a2_cell_key(cells, h.pt0 + i, bias);
      if (i > 0) prev = a2_cell_key(cells, h.pt0 + i - 1, bias);
      keys_out[h.pt0 + i] = key;
    } else {
      const uint64_t* keys = static_cast<const uint64_t*>(src);
      key = keys[h.pt0 + i];
      if (i > 0) prev = keys[h.pt0 + i - 1];
      sh = h.shift;
    }
    const uint64_t x = ((key ^ prev) & 0xFFFFFFFFFFFFull) >> sh;
    bin = i == 0 ? 16 : (x ? (63 - __clzll((long long)x)) / 3 : 0);
  }
  int lr = 0;
#pragma unroll
  for (int b = 0; b < kA2Bins; ++b) {
    const unsigned long long m = __ballot(bin == b);
    if (bin == b) lr = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave][b] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (act) {
    for (int w = 0; w < wave; ++w) lr += (int)s_cnt[w][bin];
    packed[h.pt0 + i] = (uint16_t)((bin << 8) | lr);
  }
  if (threadIdx.x < kA2Bins)
    hist[(int64_t)blockIdx.x * kA2Bins + threadIdx.x] =
        s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
}

// one block per frame: hist[17 block + s] becomes the number of points of size s in the frame's blocks in front of it;
// bins[17 f + s] = the points of a larger size (where size s starts in the introduction order), cells[16 f + k] =
// #{s >= k}
__global__ __launch_bounds__(256) void k_a2_scan(const A2Order* __restrict__ tab, uint32_t* __restrict__ hist,
                                                 uint32_t* __restrict__ bins, uint32_t* __restrict__ cells) {
  __shared__ uint32_t s_w[4][kA2Bins];
  const int f = blockIdx.x;
  const A2Order& h = tab[f];
  const int64_t nb = (h.n + 255) / 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry[kA2Bins];
#pragma unroll
  for (int b = 0; b < kA2Bins; ++b) carry[b] = 0u;
  for (int64_t t0 = 0; t0 < nb; t0 += 256) {
    const int64_t blk = t0 + threadIdx.x;
    const bool in = blk < nb;
    uint32_t* row = hist + (h.blk0 + blk) * kA2Bins;
    uint32_t v[kA2Bins], inc[kA2Bins];
#pragma unroll
    for (int b = 0; b < kA2Bins; ++b) {
      v[b] = in ? row[b] : 0u;
      uint32_t x = v[b];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)x, d, 64);
        x += lane >= d ? o : 0u;
      }
      inc[b] = x;
      if (lane == 63) s_w[wave][b] = x;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < kA2Bins; ++b) {
      uint32_t pre = carry[b];
      for (int w = 0; w < wave; ++w) pre += s_w[w][b];
      if (in) row[b] = pre + inc[b] - v[b];
      carry[b] += s_w[0][b] + s_w[1][b] + s_w[2][b] + s_w[3][b];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint32_t run = 0;
#pragma unroll
    for (int b = kA2Bins - 1; b >= 0; --b) {
      bins[f * kA2Bins + b] = run;
      run += carry[b];
      if (b < 16) cells[f * 16 + b] = run;
    }
  }
}

// first(i): the first key of the frame not below key_i with its low `bits` bits cleared (bits = 3 (s + 1), + the
// encoder's key_shift); searched in [0, i], so the result never lies behind i
__device__ __forceinline__ int64_t a2_first(const uint64_t* __restrict__ keys, int64_t i, int bits) {
  const uint64_t low = bits >= 48 ? 0xFFFFFFFFFFFFull : (1ull << bits) - 1ull;
  const uint64_t t = keys[i] & ~low;
  int64_t lo = 0, hi = i;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the place of every point in the introduction order and its predictor.  ENC: the residual of its merged value against
// the predictor's goes to that place of resid ([n][c] per frame at val_off, wrapped to the value width); otherwise
// (decoder; KEEP) place and predictor are kept: rank[pt0 + i], first[pt0 + i].  ENC and KEEP: the encoder of version 7,
// whose k_a7_quant follows the kept predictors instead of searching again
template <bool ENC, bool KEEP = !ENC>
__global__ __launch_bounds__(256) void k_a2_place(const uint64_t* __restrict__ keys_all, const A2Order* __restrict__ tab, int nf,
                                                  const uint16_t* __restrict__ packed, const uint32_t* __restrict__ hist,
                                                  const uint32_t* __restrict__ bins, const AFrame* __restrict__ ftab,
                                                  const uint16_t* __restrict__ merged, uint16_t* __restrict__ resid,
                                                  uint32_t* __restrict__ rank, uint32_t* __restrict__ first) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const uint32_t pk = packed[h.pt0 + i];
  const int s = (int)(pk >> 8);
  const int64_t r = (int64_t)bins[f * kA2Bins + s] + hist[(int64_t)blockIdx.x * kA2Bins + s] + (pk & 255u);
  const int64_t j = i > 0 ? a2_first(keys_all + h.pt0, i, 3 * (s + 1) + (ENC ? h.shift : 0)) : 0;
  if constexpr (ENC && !KEEP) {
    const AFrame& a = ftab[f];
    const uint32_t mask = (1u << (8 * a.bpv)) - 1u;
    if (r >= h.n) return;   // cannot happen: the places are a permutation of the frame's points
    for (int ch = 0; ch < a.c; ++ch) {
      const uint32_t v = merged[a.val_off + i * a.c + ch], pv = i > 0 ? merged[a.val_off + j * a.c + ch] : 0u;
      resid[a.val_off + r * a.c + ch] = (uint16_t)((v - pv) & mask);
    }
  } else {
    rank[h.pt0 + i] = (uint32_t)r;
    first[h.pt0 + i] = (uint32_t)j;
  }
}

// Version 7, encoder, behind k_a2_place<true, true>: point i follows first() up to point 0 (at most 17 links, each to a
// strictly larger size of introduction, so strictly downwards in Morton index), then walks back down quantising every
// member of the chain against the running reconstruction v^ (what that member's own thread computes too: its chain is
// the tail of this one), and writes its own index j to its place rank[i] of idx, wrapped to the value width.  No thread
// waits for another; the chain's 17 indices stay in registers (every loop is unrolled to constant subscripts).
__global__ __launch_bounds__(256) void k_a7_quant(const A2Order* __restrict__ tab, int nf, const AFrame* __restrict__ ftab,
                                                  const uint16_t* __restrict__ merged, const uint32_t* __restrict__ rank,
                                                  const uint32_t* __restrict__ first, uint16_t* __restrict__ idx) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const AFrame& a = ftab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const int64_t r = rank[h.pt0 + i];
  if (r >= h.n) return;   // cannot happen: the places are a permutation of the frame's points
  uint32_t chain[kA2Bins];
  int len = 0;
  int64_t j = i;
#pragma unroll
  for (int step = 0; step < kA2Bins; ++step) {
    if (j >= 0) {
      chain[step] = (uint32_t)j;
      len = step + 1;
      const int64_t nj = j > 0 ? (int64_t)first[h.pt0 + j] : -1;
      j = nj < j ? nj : -1;   // first(j) < j for every j > 0
    }
  }
  const int c = a.c, e = a.e, q = 2 * e + 1;
  const uint32_t mask = (1u << (8 * a.bpv)) - 1u;
  const uint16_t* v = merged + a.val_off;
  for (int ch = 0; ch < c; ++ch) {
    int vh = 0, jj = 0;
#pragma unroll
    for (int step = kA2Bins - 1; step >= 0; --step) {
      if (step < len) {
        jj = a_quant((int)v[(int64_t)chain[step] * c + ch] - vh, e, q);
        vh += jj * q;
      }
    }
    idx[a.val_off + r * c + ch] = (uint16_t)((uint32_t)jj & mask);
  }
}

// decoder: the value of point (cell) i = the wrapped sum of the residuals along i -> first(i) -> .. -> 0, at most 17
// links since every link leads to a strictly larger size.  Every index is checked against the frame's value count;
// status |= 8 where a walk leaves it or does not end at point 0.  resid_all / out_all: the frames' [m][c] values of bpv
// bytes at out_off, residuals in introduction order / values in Morton order.
// NL (version 7): the same walk over the indices j, sign-extended from the value width; the value is their sum times
// q = 2 e + 1, clamped to the value width.  status |= 16 where the sum of a complete walk lies outside [-e, mask + e],
// which no encoder's reconstruction does.
template <bool NL>
__global__ __launch_bounds__(256) void k_a2_walk(const A2Order* __restrict__ tab, int nf, const ADFrame* __restrict__ ftab,
                                                 const uint32_t* __restrict__ rank, const uint32_t* __restrict__ first,
                                                 const uint8_t* __restrict__ resid_all, uint8_t* __restrict__ out_all,
                                                 int32_t* __restrict__ status_all) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const ADFrame& a = ftab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const int c = a.c, bpv = a.bpv;
  const uint8_t* resid = resid_all + a.out_off;
  uint32_t acc[4] = {0u, 0u, 0u, 0u};   // NL: sums of int32 in two's complement
  int64_t j = i;
  bool ok = false;
  for (int step = 0; step < kA2Bins; ++step) {
    const int64_t r = rank[h.pt0 + j];
    if (r >= h.n) break;
    const uint8_t* q = resid + r * c * bpv;
    for (int ch = 0; ch < c; ++ch) acc[ch] += NL ? (uint32_t)a_load_s(q, bpv, ch) : a_load(q, bpv, ch);
    if (j == 0) {
      ok = true;
      break;
    }
    const int64_t nj = first[h.pt0 + j];
    if (nj >= j) break;
    j = nj;
  }
  uint8_t* o = out_all + a.out_off + i * c * bpv;
  if constexpr (!NL) {
    if (!ok) atomicOr(status_all + f, 8);
    for (int ch = 0; ch < c; ++ch) a_store(o, bpv, acc[ch], ch);
  } else {
    const int e = a.max_error, mask = (1 << (8 * bpv)) - 1;
    bool far = false;
    for (int ch = 0; ch < c; ++ch) {
      const int64_t x = (int64_t)(int32_t)acc[ch] * (2 * e + 1);
      far |= x < -e || x > mask + e;
      a_store(o, bpv, (uint32_t)(x < 0 ? 0 : (x > mask ? mask : x)), ch);
    }
    if (!ok || far) atomicOr(status_all + f, (ok ? 0 : 8) | (ok && far ? 16 : 0));
  }
}

// ---- cross-channel kinds (versions 8, 11, 13, 14; attr_blob.h states the rule) -------------------------------------
// Elementwise passes: one thread per point, the point's channels in registers, frame = blockIdx.y.  cross[f]: the
// frame's mask m, bit ch - 1 set where channel ch is coded against channel ch - 1.  A point's c values are 2 c (or bpv c)
// consecutive bytes and a wave's 64 points one contiguous stretch, read value by value: a frame's rows start wherever the
// frames in front of it end (c = 3 leaves no 8-byte alignment), and the passes stand beside a coder that walks the same
// values one decision at a time.
//
// x of a point's w[0 .. c), wrapped to the value width: from the last channel down, so that every difference is taken
// against the original w of the channel before it; and its inverse, from channel 1 up
__device__ __forceinline__ void a_cross_fwd(uint32_t (&w)[4], int c, int m, uint32_t mask) {
#pragma unroll
  for (int ch = 3; ch >= 1; --ch)
    if (ch < c && ((m >> (ch - 1)) & 1)) w[ch] = (w[ch] - w[ch - 1]) & mask;
}
__device__ __forceinline__ void a_cross_inv(uint32_t (&w)[4], int c, int m, uint32_t mask) {
#pragma unroll
  for (int ch = 1; ch <= 3; ++ch)
    if (ch < c && ((m >> (ch - 1)) & 1)) w[ch] = (w[ch] + w[ch - 1]) & mask;
}

// Encoder, in front of the counting pass.  RUN = false (versions 11, 13, 14): in place over the [n][c] array that
// k_a2_place<true>, k_a4_quant or k_a7_quant left for the coder; a frame with m = 0 keeps what it has.  RUN = true
// (version 8): w is version 1's residual inside the lane's run, computed here from the merged values (run position
// s = i % S) and written to src for EVERY frame of the call, so that the PRED = false coder serves them all: a frame
// with m = 0 gets the bytes of its plain kind, which codes these residuals under the same contexts.
template <bool RUN>
__global__ __launch_bounds__(256) void k_ax_fwd(const AFrame* __restrict__ tab, const int32_t* __restrict__ cross,
                                                const uint16_t* __restrict__ merged, uint16_t* __restrict__ src) {
  const AFrame& h = tab[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const int c = h.c, m = cross[blockIdx.y];
  if (!RUN && m == 0) return;
  const uint32_t mask = (1u << (8 * h.bpv)) - 1u;
  uint16_t* o = src + h.val_off + i * c;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if constexpr (RUN) {
    const uint16_t* v = merged + h.val_off + i * c;
    const int64_t s = i % h.S;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < c) {
        const uint32_t a = s >= 1 ? v[ch - c] : 0u, b = s >= 2 ? v[ch - 2 * c] : 0u;
        w[ch] = ((uint32_t)v[ch] - a_pred(s, a, b)) & mask;
      }
  } else {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < c) w[ch] = o[ch];
  }
  a_cross_fwd(w, c, m, mask);
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
    if (ch < c) o[ch] = (uint16_t)w[ch];
}

// Decoder, behind k_a_dec<true>: the inverse, in place over the frame's first n_dec points (all of them; the values of
// a level of detail for versions 11 and 14, whose rows stand in introduction order).  data_all: the frames' [n_dec][c]
// values of bpv bytes at out_off, as the coder wrapped them
__global__ __launch_bounds__(256) void k_ax_inv(const ADFrame* __restrict__ tab, const int32_t* __restrict__ cross,
                                                uint8_t* __restrict__ data_all) {
  const ADFrame& h = tab[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h.n_dec) return;
  const int c = h.c, bpv = h.bpv;
  const uint32_t mask = (1u << (8 * bpv)) - 1u;
  uint8_t* p = data_all + h.out_off + i * c * bpv;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
    if (ch < c) w[ch] = a_load(p, bpv, ch);
  a_cross_inv(w, c, cross[blockIdx.y], mask);
#pragma unroll
  for (int ch = 1; ch < 4; ++ch)
    if (ch < c) a_store(p, bpv, w[ch], ch);
}

// Version 8, behind k_ax_inv: version 1's predictor inside the run over the residuals, modulo 2^(8 bpv) as
// a_decode_chunk<.., false> applies it, in place; frame = blockIdx.y, one thread per (lane run, channel) as k_a4_recon
__global__ __launch_bounds__(256) void k_a8_recon(const ADFrame* __restrict__ tab, uint8_t* __restrict__ data_all) {
  const ADFrame& h = tab[blockIdx.y];
  const int c = h.c, bpv = h.bpv;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t base = t / c * h.S;
  const int ch = (int)(t % c);
  if (base >= h.n) return;
  const int npts = (int)std::min<int64_t>(h.S, h.n - base);
  const uint32_t mask = (1u << (8 * bpv)) - 1u;
  uint8_t* o = data_all + h.out_off + (base * c + ch) * bpv;
  uint32_t a = 0, b = 0;   // v[s - 1], v[s - 2]
  for (int s = 0; s < npts; ++s) {
    const int64_t at = (int64_t)s * c * bpv;
    const uint32_t val = (a_pred(s, a, b) + a_load(o + at, bpv)) & mask;
    b = a;
    a = val;
    a_store(o + at, bpv, val);
  }
}

// ---- version 19: the transform over the binary splits of the Morton tree (attr_blob.h states the rule) --------------
// The coding order is version 2's introduction order at bit granularity: 49 sublevels b = 0 .. 48 in place of 17 sizes,
// found by the same three steps (k_at_size / k_at_scan / k_at_place are k_a2_size / k_a2_scan / k_a2_place over 49
// bins; the rows are A2Order's: shift = the encoder's key_shift, the decoder's slod).  What they leave is, per frame,
// where every sublevel starts in the coding order and how many points it holds (bins[98 f + b], bins[98 f + 49 + b]) and
// the Morton index of every place (inv[pt0 + r]); the host reads the counts and launches k_at_lift once per sublevel
// that holds a point in any frame of the call, over the most points a frame has there.
constexpr int kATBins = 49;

template <bool FROM_CELLS>
__global__ __launch_bounds__(256) void k_at_size(const void* __restrict__ src, const A2Order* __restrict__ tab, int nf,
                                                 uint64_t* __restrict__ keys_out, uint16_t* __restrict__ packed,
                                                 uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_cnt[4][kATBins];
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  const bool act = i < h.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bin = kATBins;   // none
  if (act) {
    uint64_t key, prev = 0;
    int sh = 0;
    if constexpr (FROM_CELLS) {
      const int32_t* cells = static_cast<const int32_t*>(src);
      const int bias = 32768 >> h.shift;
      key = a2_cell_key(cells, h.pt0 + i, bias);
      if (i > 0) prev = a2_cell_key(cells, h.pt0 + i - 1, bias);
      keys_out[h.pt0 + i] = key;
    } else {
      const uint64_t* keys = static_cast<const uint64_t*>(src);
      key = keys[h.pt0 + i];
      if (i > 0) prev = keys[h.pt0 + i - 1];
      sh = h.shift;
    }
    const uint64_t x = ((key ^ prev) & 0xFFFFFFFFFFFFull) >> sh;
    bin = i == 0 ? 48 : (x ? 63 - __clzll((long long)x) : 0);
  }
  int lr = 0;
  for (int b = 0; b < kATBins; ++b) {
    const unsigned long long m = __ballot(bin == b);
    if (bin == b) lr = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave][b] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (act) {
    for (int w = 0; w < wave; ++w) lr += (int)s_cnt[w][bin];
    packed[h.pt0 + i] = (uint16_t)((bin << 8) | lr);
  }
  if (threadIdx.x < kATBins)
    hist[(int64_t)blockIdx.x * kATBins + threadIdx.x] =
        s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
}

// one block per frame, thread b < 49 owns sublevel b: hist[49 block + b] becomes the number of points of sublevel b in
// the frame's blocks in front of it (a serial walk over the frame's blocks, 49 neighbouring words per step); then
// bins[98 f + b] = the points of a higher sublevel, bins[98 f + 49 + b] = the points of sublevel b
__global__ __launch_bounds__(64) void k_at_scan(const A2Order* __restrict__ tab, uint32_t* __restrict__ hist,
                                                uint32_t* __restrict__ bins) {
  __shared__ uint32_t s_tot[kATBins];
  const int f = blockIdx.x, b = threadIdx.x;
  const A2Order& h = tab[f];
  const int64_t nb = (h.n + 255) / 256;
  if (b < kATBins) {
    uint32_t run = 0;
    uint32_t* col = hist + (int64_t)h.blk0 * kATBins + b;
    for (int64_t k0 = 0; k0 < nb; k0 += 8) {   // eight loads in flight
      uint32_t v[8];
#pragma unroll
      for (int d = 0; d < 8; ++d) v[d] = k0 + d < nb ? col[(k0 + d) * kATBins] : 0u;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        if (k0 + d < nb) col[(k0 + d) * kATBins] = run;
        run += v[d];
      }
    }
    s_tot[b] = run;
  }
  __syncthreads();
  if (b < kATBins) {
    uint32_t above = 0;
    for (int k = b + 1; k < kATBins; ++k) above += s_tot[k];
    bins[f * 2 * kATBins + b] = above;
    bins[f * 2 * kATBins + kATBins + b] = s_tot[b];
  }
}

// inv[pt0 + r] = the Morton index of the point at place r of the frame's coding order
__global__ __launch_bounds__(256) void k_at_place(const A2Order* __restrict__ tab, int nf, const uint16_t* __restrict__ packed,
                                                  const uint32_t* __restrict__ hist, const uint32_t* __restrict__ bins,
                                                  uint32_t* __restrict__ inv) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const uint32_t pk = packed[h.pt0 + i];
  const int b = (int)(pk >> 8);
  const int64_t r = (int64_t)bins[f * 2 * kATBins + b] + hist[(int64_t)blockIdx.x * kATBins + b] + (pk & 255u);
  if (r >= h.n) return;   // cannot happen: the places are a permutation of the frame's points
  inv[h.pt0 + r] = (uint32_t)i;
}

// floor(a / w), w > 0
__device__ __forceinline__ int64_t at_floor_div(int64_t a, int64_t w) {
  const int64_t d = a / w;
  return d - ((a % w != 0 && a < 0) ? 1 : 0);
}

// s = max(2, isqrt(floor(q^2 w / (wa wb)))): the quotient is at most 2 q^2 < 2^31, which a double holds exactly; the
// root's estimate is corrected in integers
__device__ __forceinline__ int64_t at_root2(uint64_t v) {   // max(2, isqrt(v)), v < 2^52
  uint64_t r = (uint64_t)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r < 2 ? 2 : (int64_t)r;
}
__device__ __forceinline__ int64_t at_step(int64_t q, int64_t wa, int64_t wb) {
  return at_root2((uint64_t)(q * q) * (uint64_t)(wa + wb) / ((uint64_t)wa * (uint64_t)wb));
}

// The pair that thread j = blockIdx.x blockDim.x + threadIdx.x takes at sublevel t of frame f (h = tab[f]): place r =
// bins[..][t] + j of the frame's coding order, point i = inv[place], and lo, the first key of the frame not below
// key_i with its bits bit and lower cleared (bit = t + shift <= 47; shift: the low bits of an encoder's keys that are
// not the cells').  false: no pair (j beyond the sublevel's count, or a place or point outside the frame: cannot
// happen).  t_hi: the first key beyond the subtree of key_i above bit, what at_upper searches for
struct ATPair {
  int64_t r, i, lo;
  uint64_t t_hi;
};
__device__ __forceinline__ bool at_pair(const uint64_t* __restrict__ keys, const A2Order& h, const uint32_t* __restrict__ bins,
                                        const uint32_t* __restrict__ inv, int f, int t, int shift, ATPair& p) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (int64_t)bins[f * 2 * kATBins + kATBins + t]) return false;
  p.r = (int64_t)bins[f * 2 * kATBins + t] + j;
  if (p.r >= h.n) return false;
  p.i = inv[h.pt0 + p.r];
  if (p.i <= 0 || p.i >= h.n) return false;
  const int bit = t + shift;
  const uint64_t key = keys[p.i], low = (1ull << bit) - 1ull;
  const uint64_t t_lo = key & ~((low << 1) | 1ull);
  p.t_hi = (key | low) + 1ull;
  int64_t lo = 0, hi = p.i;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < t_lo) lo = mid + 1; else hi = mid;
  }
  p.lo = lo;
  return true;
}
// the end of the pair's right half: the first key of the frame behind key_i that is not below t_hi (n: none)
__device__ __forceinline__ int64_t at_upper(const uint64_t* __restrict__ keys, int64_t i, int64_t n, uint64_t t_hi) {
  int64_t a = i + 1, b = n;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (keys[mid] < t_hi) a = mid + 1; else b = mid;
  }
  return a;
}

// the index of a difference hh under step s, wrapped to the value width: sgn(hh) min((|hh| + s / 2) / s, H - 1)
__device__ __forceinline__ uint32_t at_quant(int64_t hh, int64_t s, int64_t H, uint32_t mask) {
  const int64_t m = std::min<int64_t>(((hh < 0 ? -hh : hh) + s / 2) / s, H - 1);
  return (uint32_t)(hh < 0 ? -m : m) & mask;
}

// The pairs of sublevel t, frame = blockIdx.y: thread j takes place bins[..][t] + j of the frame's coding order, point
// i = inv[place]; lo and hi by two binary searches in the frame's keys (at_pair, at_upper; an encoder's keys carry
// key_shift low bits that are not the cells').  ENC: val = the frame's merged values, lifted in place (a node's value
// lies between its children's, so it stays a uint16), the index (at_quant) to the point's place of idx, wrapped to the
// value width.  Otherwise (decoder): x_all
// the decoded indices in coding order (bpv bytes each, at out_off), val_all int64 [n][c] at element out_off; status |= 8
// where the keys give a pair without a left or a right leaf (keys that are not sorted and distinct).  PC (version 21):
// one step per channel, q[ch] = aux_all[5 f + ch], in place of the frame's one q (Aux = const int32_t*, one argument
// more); the two searches serve every channel, at_step runs once per channel.
template <bool ENC, typename... Aux>
__global__ __launch_bounds__(256) void k_at_lift(const uint64_t* __restrict__ keys_all, const A2Order* __restrict__ tab,
                                                 const uint32_t* __restrict__ bins, const uint32_t* __restrict__ inv, int t,
                                                 const AFrame* __restrict__ etab, uint16_t* __restrict__ val_e, uint16_t* __restrict__ idx,
                                                 const ADFrame* __restrict__ dtab, const uint8_t* __restrict__ x_all,
                                                 int64_t* __restrict__ val_d, int32_t* __restrict__ status_all, Aux... aux) {
  constexpr bool PC = sizeof...(Aux) > 0;
  [[maybe_unused]] const int32_t* aux_all = a_aux(aux...);
  const int f = blockIdx.y;
  const A2Order& h = tab[f];
  const uint64_t* keys = keys_all + h.pt0;
  ATPair p;
  if (!at_pair(keys, h, bins, inv, f, t, ENC ? h.shift : 0, p)) return;
  const int64_t r = p.r, i = p.i, lo = p.lo, a = at_upper(keys, i, h.n, p.t_hi);
  const int64_t wa = i - lo, wb = a - i, w = wa + wb;
  if constexpr (ENC) {
    const AFrame& fr = etab[f];
    if (wa < 1) return;   // cannot happen: the keys are sorted and distinct
    const int c = fr.c;
    int64_t s = PC ? 0 : at_step(fr.e, wa, wb);
    const int64_t H = (int64_t)1 << (8 * fr.bpv - 1);
    const uint32_t mask = (1u << (8 * fr.bpv)) - 1u;
    uint16_t* v = val_e + fr.val_off;
    for (int ch = 0; ch < c; ++ch) {
      if constexpr (PC) s = at_step(aux_all[5 * f + ch], wa, wb);
      const int64_t va = v[lo * c + ch], hh = (int64_t)v[i * c + ch] - va;
      v[lo * c + ch] = (uint16_t)(va + at_floor_div(wb * hh, w));
      idx[fr.val_off + r * c + ch] = (uint16_t)at_quant(hh, s, H, mask);
    }
  } else {
    const ADFrame& fr = dtab[f];
    if (wa < 1) {
      atomicOr(status_all + f, 8);
      return;
    }
    const int c = fr.c, bpv = fr.bpv;
    int64_t s = PC ? 0 : at_step(fr.max_error, wa, wb);
    const uint8_t* x = x_all + fr.out_off + r * c * bpv;
    int64_t* v = val_d + fr.out_off;
    for (int ch = 0; ch < c; ++ch) {
      if constexpr (PC) s = at_step(aux_all[5 * f + ch], wa, wb);
      const int64_t hh = (int64_t)a_load_s(x, bpv, ch) * s;   // |x| < 2^15, s < 2^16; wb < 2^27: no product leaves int64
      const int64_t va = v[lo * c + ch] - at_floor_div(wb * hh, w);
      v[lo * c + ch] = va;
      v[i * c + ch] = va + hh;
    }
  }
}

// encoder, behind the last sublevel: x[0] = val[0] - H to place 0; one thread per (frame, channel)
__global__ __launch_bounds__(256) void k_at_mean(const AFrame* __restrict__ tab, int nf, const uint16_t* __restrict__ val,
                                                 uint16_t* __restrict__ idx) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, f = t >> 2, ch = t & 3;
  if (f >= nf || ch >= tab[f].c) return;
  const AFrame& h = tab[f];
  idx[h.val_off + ch] = (uint16_t)(((uint32_t)val[h.val_off + ch] - (1u << (8 * h.bpv - 1))) & ((1u << (8 * h.bpv)) - 1u));
}

// decoder, in front of the first sublevel: val[0] = x[0] + H
__global__ __launch_bounds__(256) void k_at_root(const ADFrame* __restrict__ tab, int nf, const uint8_t* __restrict__ x_all,
                                                 int64_t* __restrict__ val) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, f = t >> 2, ch = t & 3;
  if (f >= nf || ch >= tab[f].c) return;
  const ADFrame& h = tab[f];
  val[h.out_off + ch] = (int64_t)a_load_s(x_all + h.out_off, h.bpv, ch) + ((int64_t)1 << (8 * h.bpv - 1));
}

// decoder, behind the last sublevel: the clamp and the narrowing store, frame = blockIdx.y, one thread per value
__global__ __launch_bounds__(256) void k_at_store(const ADFrame* __restrict__ tab, const int64_t* __restrict__ val,
                                                  uint8_t* __restrict__ out_all) {
  const ADFrame& h = tab[blockIdx.y];
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= h.n * h.c) return;
  const int64_t mask = ((int64_t)1 << (8 * h.bpv)) - 1, x = val[h.out_off + k];
  a_store(out_all + h.out_off + k * h.bpv, h.bpv, (uint32_t)(x < 0 ? 0 : (x > mask ? mask : x)));
}

// ---- version 21: the colour transform (attr_blob.h states the rule) ------------------------------------------------
// encoder, between the merge and the order stage: R, G, B of every point of a frame whose aux_all[5 f + 4] is 1 become
// Y, Co, Cg in place (all three in 0 .. mask); frame = blockIdx.y, one thread per point, a fourth channel untouched
__global__ __launch_bounds__(256) void k_ac_fwd(const AFrame* __restrict__ tab, const int32_t* __restrict__ aux_all,
                                                uint16_t* __restrict__ val) {
  const int f = blockIdx.y;
  const AFrame& h = tab[f];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h.n || h.c < 3 || aux_all[5 * f + 4] != 1) return;
  uint16_t* v = val + h.val_off + i * h.c;
  const int H = 1 << (8 * h.bpv - 1);
  const int R = v[0], G = v[1], B = v[2];
  const int co = R - B, t = B + (co >> 1), cg = G - t;
  v[0] = (uint16_t)(t + (cg >> 1));
  v[1] = (uint16_t)((co >> 1) + H);
  v[2] = (uint16_t)((cg >> 1) + H);
}

// decoder, in place of k_at_store for a call with a colour frame (version 21) and for every call of version 22:
// k_at_store's clamp, the inverse colour transform of a frame whose aux_all[5 f + 4] is 1, the second clamp and the
// narrowing store; frame = blockIdx.y, one thread per value of the frame's n_dec points (versions 19 and 21: all of
// them, n_dec = n; version 22: its cells at the level of detail, while h.n stays the whole blob's for the lane decoder)
__global__ __launch_bounds__(256) void k_ac_store(const ADFrame* __restrict__ tab, const int32_t* __restrict__ aux_all,
                                                  const int64_t* __restrict__ val, uint8_t* __restrict__ out_all) {
  const int f = blockIdx.y;
  const ADFrame& h = tab[f];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h.n_dec) return;
  const int c = h.c, bpv = h.bpv;
  const int64_t mask = ((int64_t)1 << (8 * bpv)) - 1;
  int x[4] = {0, 0, 0, 0};
  for (int ch = 0; ch < c; ++ch) {
    const int64_t a = val[h.out_off + i * c + ch];
    x[ch] = (int)(a < 0 ? 0 : (a > mask ? mask : a));
  }
  if (c >= 3 && aux_all[5 * f + 4] == 1) {
    const int H = 1 << (8 * bpv - 1), m = (int)mask;
    const int co = 2 * (x[1] - H), cg = 2 * (x[2] - H), t = x[0] - (cg >> 1);
    const int G = cg + t, B = t - (co >> 1), R = B + co;
    x[0] = R < 0 ? 0 : (R > m ? m : R);
    x[1] = G < 0 ? 0 : (G > m ? m : G);
    x[2] = B < 0 ? 0 : (B > m ? m : B);
  }
  uint8_t* o = out_all + h.out_off + i * c * bpv;
  for (int ch = 0; ch < c; ++ch) a_store(o, bpv, (uint32_t)x[ch], ch);
}

// ---- version 22: weights a decoder at a cut can form (attr_blob.h states the rule) ---------------------------------
// Behind the order stage, over the same rows and blocks.  K: the frame's deepest cut (etab[f].e for the encoder, whose
// call has one K; dtab[f].max_error for the decoder, whose blobs each bring their own).  lod3 = 3 j for a decoder at cut
// j (its bins are sublevels t - 3 j), 0 for the encoder.
//
// flags[pt0 + i] = 1 where point (cell) i is the first of its K-cell, that is where its sublevel is 3 K or higher; the
// call's last point also clears the one word behind the flags, so that their exclusive scan g has an entry for every
// frame's end
__global__ __launch_bounds__(256) void k_as_flag(const A2Order* __restrict__ tab, int nf, const uint16_t* __restrict__ packed,
                                                 const AFrame* __restrict__ etab, const ADFrame* __restrict__ dtab, int lod3,
                                                 uint32_t* __restrict__ flags) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const int K = etab ? etab[f].e : dtab[f].max_error;
  flags[h.pt0 + i] = (int)(packed[h.pt0 + i] >> 8) + lod3 >= 3 * K ? 1u : 0u;
  if (f == nf - 1 && i == h.n - 1) flags[h.pt0 + h.n] = 0u;
}

// encoder: version 2's 16 counts from the sublevels' starts and counts, cells[16 f + k] = #{i : b(i) >= 3 k}
__global__ __launch_bounds__(256) void k_as_counts(const uint32_t* __restrict__ bins, int nf, uint32_t* __restrict__ cells) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, f = t >> 4, k = t & 15;
  if (f >= nf) return;
  cells[t] = bins[f * 2 * kATBins + 3 * k] + bins[f * 2 * kATBins + kATBins + 3 * k];
}

// k_at_lift under version 22's weights, one thread per pair for all channels, the same places, searches and arrays.
// g: the exclusive scan of k_as_flag's flags over the call's points (differences inside a frame count its K-cells).
// Bin t of the call's keys is the absolute sublevel t + lod3.  At 3 K and above: two lower bounds and two differences
// of g; below: one lower bound, no hi, weights 1 : 1 and a step that depends on the sublevel alone.  M from the
// frame's K-cell count (the points of sublevel 3 K and above, in bins) and the blob's n.
template <bool ENC>
__global__ __launch_bounds__(256) void k_as_lift(const uint64_t* __restrict__ keys_all, const A2Order* __restrict__ tab,
                                                 const uint32_t* __restrict__ bins, const uint32_t* __restrict__ inv, int t,
                                                 const uint32_t* __restrict__ g_all, int lod3, const AFrame* __restrict__ etab,
                                                 uint16_t* __restrict__ val_e, uint16_t* __restrict__ idx,
                                                 const ADFrame* __restrict__ dtab, const uint8_t* __restrict__ x_all,
                                                 int64_t* __restrict__ val_d, int32_t* __restrict__ status_all,
                                                 const int32_t* __restrict__ aux_all) {
  const int f = blockIdx.y;
  const A2Order& h = tab[f];
  const uint64_t* keys = keys_all + h.pt0;
  const uint32_t* g = g_all + h.pt0;
  ATPair p;
  if (!at_pair(keys, h, bins, inv, f, t, ENC ? h.shift : 0, p)) return;
  const int64_t r = p.r, i = p.i, lo = p.lo;
  const int K3 = 3 * (ENC ? etab[f].e : dtab[f].max_error), ta = t + lod3, tk = K3 - lod3;   // 0 <= tk <= 45
  const bool inside = ta < K3;
  int64_t ca = 1, cb = 1, M = 1;
  if (!inside) {
    const int64_t a = at_upper(keys, i, h.n, p.t_hi);
    const int64_t gi = g[i], C = (int64_t)bins[f * 2 * kATBins + tk] + bins[f * 2 * kATBins + kATBins + tk];
    const int64_t n_all = ENC ? h.n : dtab[f].n;
    ca = gi - (int64_t)g[lo];
    cb = (int64_t)g[a] - gi;
    M = C > 0 ? std::max<int64_t>(1, (2 * n_all + C) / (2 * C)) : 1;
  }
  const bool broken = lo >= i || ca < 1 || cb < 1;   // cannot happen with sorted, distinct keys
  const int64_t w = ca + cb;
  const int c = ENC ? etab[f].c : dtab[f].c;
  // s[ch] = max(2, isqrt(v)): v = floor(q^2 w / (ca cb M)) <= 2 q^2, or floor(2 q^2 / 2^floor(2 t / 3))
  const auto step = [&](int ch) -> int64_t {
    const uint64_t q = (uint64_t)aux_all[5 * f + ch], q2 = q * q;
    return at_root2(inside ? (2 * q2) >> (2 * ta / 3) : q2 * (uint64_t)w / ((uint64_t)ca * (uint64_t)cb * (uint64_t)M));
  };
  if constexpr (ENC) {
    const AFrame& fr = etab[f];
    if (broken) return;
    const int64_t H = (int64_t)1 << (8 * fr.bpv - 1);
    const uint32_t mask = (1u << (8 * fr.bpv)) - 1u;
    uint16_t* v = val_e + fr.val_off;
    for (int ch = 0; ch < c; ++ch) {
      const int64_t s = step(ch);
      const int64_t va = v[lo * c + ch], hh = (int64_t)v[i * c + ch] - va;
      v[lo * c + ch] = (uint16_t)(va + (inside ? hh >> 1 : at_floor_div(cb * hh, w)));
      idx[fr.val_off + r * c + ch] = (uint16_t)at_quant(hh, s, H, mask);
    }
  } else {
    const ADFrame& fr = dtab[f];
    if (broken) {
      atomicOr(status_all + f, 8);
      return;
    }
    const int bpv = fr.bpv;
    const uint8_t* x = x_all + fr.out_off + r * c * bpv;
    int64_t* v = val_d + fr.out_off;
    for (int ch = 0; ch < c; ++ch) {
      const int64_t hh = (int64_t)a_load_s(x, bpv, ch) * step(ch);   // |x| < 2^15, s < 2^17; cb < 2^27: no product leaves int64
      const int64_t va = v[lo * c + ch] - (inside ? hh >> 1 : at_floor_div(cb * hh, w));
      v[lo * c + ch] = va;
      v[i * c + ch] = va + hh;
    }
  }
}

// ---- versions 19 and 21 under a byte target (include/pcc.h states the ladder and the search) ------------------------
// The forward lift does not depend on the step: k_ar_lift is the encoder branch of k_at_lift without its quantiser and
// runs once per call; k_ar_quant then forms the indices of any number of candidate rows (a frame at a rung of its
// ladder) from what it left, and the rows go through k_a_stats / k_a_enc<false> as frames of their own.
//
// k_ar_lift: launched as k_at_lift<true> is.  val = the merged values, lifted in place; the raw difference hh of the
// point at place r to hh_all[val_off + r c + ch] (|hh| < 2^16), the pair's weights to wts[pt0 + r] (wa, wb < 2^27)
__global__ __launch_bounds__(256) void k_ar_lift(const uint64_t* __restrict__ keys_all, const A2Order* __restrict__ tab,
                                                 const uint32_t* __restrict__ bins, const uint32_t* __restrict__ inv, int t,
                                                 const AFrame* __restrict__ etab, uint16_t* __restrict__ val,
                                                 int32_t* __restrict__ hh_all, uint2* __restrict__ wts) {
  const int f = blockIdx.y;
  const A2Order& h = tab[f];
  const uint64_t* keys = keys_all + h.pt0;
  ATPair p;
  if (!at_pair(keys, h, bins, inv, f, t, h.shift, p)) return;
  const int64_t r = p.r, i = p.i, lo = p.lo, a = at_upper(keys, i, h.n, p.t_hi);
  const int64_t wa = i - lo, wb = a - i, w = wa + wb;
  if (wa < 1) return;   // cannot happen: the keys are sorted and distinct
  const AFrame& fr = etab[f];
  const int c = fr.c;
  wts[h.pt0 + r] = make_uint2((uint32_t)wa, (uint32_t)wb);
  uint16_t* v = val + fr.val_off;
  for (int ch = 0; ch < c; ++ch) {
    const int64_t va = v[lo * c + ch], hh = (int64_t)v[i * c + ch] - va;
    v[lo * c + ch] = (uint16_t)(va + at_floor_div(wb * hh, w));
    hh_all[fr.val_off + r * c + ch] = (int32_t)hh;
  }
}

// behind the last sublevel: val[0] - H to place 0, where k_at_mean leaves x[0]; one thread per (frame, channel)
__global__ __launch_bounds__(256) void k_ar_mean(const AFrame* __restrict__ tab, int nf, const uint16_t* __restrict__ val,
                                                 int32_t* __restrict__ hh_all) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, f = t >> 2, ch = t & 3;
  if (f >= nf || ch >= tab[f].c) return;
  const AFrame& h = tab[f];
  hh_all[h.val_off + ch] = (int32_t)val[h.val_off + ch] - (1 << (8 * h.bpv - 1));
}

// one candidate row: frame `src_off / pt0` at the steps q
struct ARRow {
  int64_t src_off;   // the frame's differences, hh_all[src_off + r c + ch]
  int64_t pt0;       // its places among the call's points, wts[pt0 + r]
  int64_t dst_off;   // the row's indices, idx[dst_off + r c + ch]: the val_off of the row's AFrame
  int64_t vals;      // n c
  int32_t blk0;      // the row owns blocks [blk0, blk0 + ceil(vals / 256)) of its launch
  int32_t c, bpv, pad;
  int32_t q[4];
};

// the quantiser of k_at_lift over the rows [0, nr) of a launch, one thread per value, neighbouring threads neighbouring
// values: 4 bytes in (the weights of a point are read by its c threads from one line), 2 bytes out.  Place 0 is copied
__global__ __launch_bounds__(256) void k_ar_quant(const ARRow* __restrict__ rows, int nr, const int32_t* __restrict__ hh_all,
                                                  const uint2* __restrict__ wts, uint16_t* __restrict__ idx) {
  const int row = o2_find(nr, blockIdx.x, [&](int i) { return (int64_t)rows[i].blk0; });
  const ARRow& h = rows[row];
  const int64_t k = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (k >= h.vals) return;
  const int c = h.c;
  const int64_t r = k / c;
  const int ch = (int)(k - r * c);
  const int64_t H = (int64_t)1 << (8 * h.bpv - 1);
  const uint32_t mask = (1u << (8 * h.bpv)) - 1u;
  const int64_t hh = hh_all[h.src_off + k];
  uint32_t x = (uint32_t)hh & mask;
  if (r > 0) {
    const uint2 wt = wts[h.pt0 + r];
    x = at_quant(hh, at_step(h.q[ch], wt.x, wt.y), H, mask);
  }
  idx[h.dst_off + k] = (uint16_t)x;
}

// the winners' chunk words, final states and lane lengths, from where the coder left them (chunk src of the call's
// candidate chunks) to a table that k_a_pack can walk (chunk dst); pick = blockIdx.y
struct ARPick {
  int32_t src, dst, nc, pad;
};
__global__ __launch_bounds__(256) void k_ar_gather(const ARPick* __restrict__ picks, const uint32_t* __restrict__ words,
                                                   const uint16_t* __restrict__ states, const uint16_t* __restrict__ lens,
                                                   uint32_t* __restrict__ words_o, uint16_t* __restrict__ states_o,
                                                   uint16_t* __restrict__ lens_o) {
  const ARPick p = picks[blockIdx.y];
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < (int64_t)p.nc) words_o[p.dst + t] = words[p.src + t];
  if (t < (int64_t)p.nc * kLanes) lens_o[(int64_t)p.dst * kLanes + t] = lens[(int64_t)p.src * kLanes + t];
  if (t < (int64_t)p.nc * 2 * kLanes) states_o[(int64_t)p.dst * 2 * kLanes + t] = states[(int64_t)p.src * 2 * kLanes + t];
}

}  // namespace

#include "attr_nbr.h"   // versions 25, 26, 28 and 31: k_an_place, k_an_plan, k_an_recon; k_anl_plan, k_anl_quant, k_anl_recon

static inline int64_t a_round(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
static inline size_t merged_b_of(int64_t vals) { return pcc_align((size_t)vals * 2); }

// sub-tables behind one another in one upload, each on pcc_align's boundary: add(b) = where a table of b bytes starts
// (b = 0: a table the call does not have, which takes no room).  bytes: all of them, padded; end: where the last table
// with data ends, the bytes an upload of the tables alone has to carry
struct ATables {
  size_t bytes = 0, end = 0;
  size_t add(size_t b) {
    const size_t at = bytes;
    if (b) end = at + b;
    bytes += pcc_align(b);
    return at;
  }
};

// version 19, what encoder and decoder share: the order stage over the call's keys (src: the encoder's distinct sorted
// keys, or the decoder's cells, whose keys go to keys_out), then the sublevels' starts and counts read back into h_bins
// (pinned; 98 per frame) behind one synchronisation.  grid[t] = the blocks of k_at_lift at sublevel t: 0 where no frame
// of the call has a point there
static int a_t_order(hipStream_t st, bool from_cells, const void* src, uint64_t* keys_out, const A2Order* d_ord, int nf,
                     int64_t blocks, uint16_t* packed, uint32_t* hist, uint32_t* bins, uint32_t* inv, uint32_t* h_bins,
                     unsigned (&grid)[kATBins]) {
  hipLaunchKernelGGL((from_cells ? k_at_size<true> : k_at_size<false>), dim3((unsigned)blocks), dim3(256), 0, st, src, d_ord, nf, keys_out,
                     packed, hist);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_at_scan, dim3((unsigned)nf), dim3(64), 0, st, d_ord, hist, bins);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_at_place, dim3((unsigned)blocks), dim3(256), 0, st, d_ord, nf, (const uint16_t*)packed, (const uint32_t*)hist,
                     (const uint32_t*)bins, inv);
  PCC_CHECK_LAUNCH();
  PCC_HIP(hipMemcpyAsync(h_bins, bins, (size_t)nf * 2 * kATBins * 4, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipStreamSynchronize(st));
  for (int t = 0; t < kATBins; ++t) {
    uint32_t most = 0;
    for (int f = 0; f < nf; ++f) {
      const uint32_t cnt = ((volatile uint32_t*)h_bins)[f * 2 * kATBins + kATBins + t];
      most = std::max(most, cnt);
    }
    grid[t] = nblk(most, 256);
  }
  return PCC_OK;
}

// version 22, what encoder and decoder share behind the order stage: the K-cell firsts of the call's points (k_as_flag)
// and their exclusive scan, *g (points + 1 entries).  a_s_cells_bytes: what the two arrays and the scan take of the arena
static size_t a_s_cells_bytes(int64_t points) { return 2 * pcc_align((size_t)(points + 1) * 4) + pcc_scan_scratch_bytes(points + 1) + 512; }
static int a_s_cells(pcc_ctx* ctx, hipStream_t st, const A2Order* d_ord, int nf, int64_t blocks, const uint16_t* packed, const AFrame* etab,
                     const ADFrame* dtab, int lod3, int64_t points, const uint32_t** g) {
  uint32_t* flags = (uint32_t*)pcc_arena_alloc(ctx, (size_t)(points + 1) * 4);
  uint32_t* scan = (uint32_t*)pcc_arena_alloc(ctx, (size_t)(points + 1) * 4);
  if (!flags || !scan) return PCC_E_NOMEM;
  hipLaunchKernelGGL(k_as_flag, dim3((unsigned)blocks), dim3(256), 0, st, d_ord, nf, packed, etab, dtab, lod3, flags);
  PCC_CHECK_LAUNCH();
  PCC_TRY(pcc_scan_exclusive_u32(ctx, flags, scan, points + 1, nullptr));
  *g = scan;
  return PCC_OK;
}

// the encoder's order stage of versions 19 and up: its arrays over the call's points (u of them in `blocks` blocks of
// nf frames) from the arena, and a_t_order over the distinct sorted keys
struct ATOrder {
  uint16_t* packed;
  uint32_t *hist, *bins, *inv;
  unsigned grid[kATBins];
};
static size_t a_t_order_bytes(int64_t u, int64_t blocks, int nf) {
  return pcc_align((size_t)u * 2) + pcc_align((size_t)blocks * kATBins * 4) + pcc_align((size_t)nf * 2 * kATBins * 4) + pcc_align((size_t)u * 4);
}
static int a_t_order_enc(pcc_ctx* ctx, hipStream_t st, const uint64_t* d_keys, const A2Order* d_ord, int nf, int64_t blocks, int64_t u,
                         uint32_t* h_bins, ATOrder* o) {
  o->packed = (uint16_t*)pcc_arena_alloc(ctx, pcc_align((size_t)u * 2));
  o->hist = (uint32_t*)pcc_arena_alloc(ctx, pcc_align((size_t)blocks * kATBins * 4));
  o->bins = (uint32_t*)pcc_arena_alloc(ctx, pcc_align((size_t)nf * 2 * kATBins * 4));
  o->inv = (uint32_t*)pcc_arena_alloc(ctx, pcc_align((size_t)u * 4));
  if (!o->packed || !o->hist || !o->bins || !o->inv) return PCC_E_NOMEM;
  return a_t_order(st, false, (const void*)d_keys, nullptr, d_ord, nf, blocks, o->packed, o->hist, o->bins, o->inv, h_bins, o->grid);
}

// one sublevel of the lift over all frames of a call: forward (ENC; etab, merged, idx) or inverse (dtab, x, val,
// status).  d_aux (version 21): the frames' steps and colour words; the lift then takes a step per channel from it.
// g (version 22, with d_aux): the scan of the K-cell firsts, and k_as_lift at lod3 in place of k_at_lift
template <bool ENC>
static int a_launch_lift(hipStream_t st, unsigned blocks, int nf, const uint64_t* keys, const A2Order* d_ord, const uint32_t* bins,
                         const uint32_t* inv, int t, const AFrame* etab, uint16_t* merged, uint16_t* idx, const ADFrame* dtab,
                         const uint8_t* x, int64_t* val, int32_t* status, const int32_t* d_aux, const uint32_t* g = nullptr,
                         int lod3 = 0) {
  if (g)
    hipLaunchKernelGGL(k_as_lift<ENC>, dim3(blocks, (unsigned)nf), dim3(256), 0, st, keys, d_ord, bins, inv, t, g, lod3, etab, merged, idx, dtab,
                       x, val, status, d_aux);
  else if (d_aux)
    hipLaunchKernelGGL((k_at_lift<ENC, const int32_t*>), dim3(blocks, (unsigned)nf), dim3(256), 0, st, keys, d_ord, bins, inv, t, etab, merged,
                       idx, dtab, x, val, status, d_aux);
  else
    hipLaunchKernelGGL(k_at_lift<ENC>, dim3(blocks, (unsigned)nf), dim3(256), 0, st, keys, d_ord, bins, inv, t, etab, merged, idx, dtab, x, val,
                       status);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// version 19, encoder, behind k_a_merge: the order stage, one k_at_lift<true> per occupied sublevel bottom-up over the
// merged values in place, and the mean; idx then holds x in coding order where the PRED = false coder reads it
// version 22 (cells_out: receives where the frames' 16 counts lie): k_as_flag and the scan behind the order stage,
// k_as_lift in place of k_at_lift, and k_as_counts for the head
static int a_t_forward(pcc_ctx* ctx, hipStream_t st, const uint64_t* d_keys, const A2Order* d_ord, const AFrame* d_tab, int nf,
                       int64_t blocks, int64_t points, uint16_t* merged, uint16_t* idx, uint32_t* h_bins, const int32_t* d_aux,
                       uint32_t** cells_out = nullptr) {
  ATOrder o;
  PCC_TRY(a_t_order_enc(ctx, st, d_keys, d_ord, nf, blocks, points, h_bins, &o));
  const uint32_t* g = nullptr;
  if (cells_out) {
    PCC_TRY(a_s_cells(ctx, st, d_ord, nf, blocks, o.packed, d_tab, nullptr, 0, points, &g));
    *cells_out = (uint32_t*)pcc_arena_alloc(ctx, (size_t)nf * 64);
    if (!*cells_out) return PCC_E_NOMEM;
    hipLaunchKernelGGL(k_as_counts, dim3(nblk(16 * (int64_t)nf, 256)), dim3(256), 0, st, (const uint32_t*)o.bins, nf, *cells_out);
    PCC_CHECK_LAUNCH();
  }
  for (int t = 0; t < kATBins - 1; ++t) {
    if (!o.grid[t]) continue;
    PCC_TRY(a_launch_lift<true>(st, o.grid[t], nf, d_keys, d_ord, o.bins, o.inv, t, d_tab, merged, idx, nullptr, nullptr, nullptr, nullptr, d_aux,
                                g));
  }
  hipLaunchKernelGGL(k_at_mean, dim3(nblk(4 * (int64_t)nf, 256)), dim3(256), 0, st, d_tab, nf, (const uint16_t*)merged, idx);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// ======================================================================== C-ABI (include/pcc.h)
// what an encode entry point asks for, resolved once.  The table of kinds (attr_blob.h):
//   version   v2  nl  tr  tc   e           between k_a_merge and the coder
//   1                          0           nothing (the coder predicts inside the run)
//   2         x                0           order stage, residuals against first()
//   4             x            max_error   k_a4_quant
//   7         x   x            max_error   order stage (kept), k_a7_quant
//   19            x   x        qstep       [k_ac_fwd,] order stage at bit granularity, lift, mean (a_t_forward)
//   21            x   x   x    1 (unread)  as 19, the steps and the colour word in the aux table
//   22            x   x   x    K           as 21 with k_as_flag, the scan and k_as_lift; version 2's counts in the head
// nl: an index stream with one u32 (e, q, or the colour word) directly behind payload_len, so versions 19 and 21 run as
// version 4 does with a_t_forward in place of k_a4_quant.  A frame with a mask in h_cross is coded as the cross form
// of the call's version (8, 11, 13, 14)
struct AEncKind {
  int version;               // the version byte of a frame without a mask
  bool v2, nl, tr, tc;
  int e;                     // AFrame::e
  int64_t n_kept;            // >= 0 (pcc_attr_encode_frames_kept): the sorted keys behind it belong to dropped rows; -1: none dropped
  const int32_t* h_cross;    // per frame the cross-channel mask m (0: the frame's plain kind), or nullptr
  const int32_t* h_qsteps;   // version 21: q[4]
  int colour;                // version 21: 0 | 1
  int K;                     // version 22: the deepest cut (0: another kind)
  bool nbr = false;          // versions 25 / 26: version 2's call with k_an_place for k_a2_place and their version bytes;
                             // with nl, versions 28 / 31: version 7's call with k_anl_plan and k_anl_quant size by size
  bool keyed() const { return v2 || tr; }   // d_keys and key_shift are read
};
static AEncKind a_kind_plain(int version, int64_t n_kept, int max_error, const int32_t* h_cross) {
  const bool v2 = version == 2, nl = max_error > 0;
  return AEncKind{attr_version(v2, nl, false), v2, nl, false, false, max_error, n_kept, h_cross, nullptr, 0, 0};
}
// versions 25 and 26: version 2's kind under the neighbour predictor
static AEncKind a_kind_nbr(int64_t n_kept, const int32_t* h_cross) {
  AEncKind k = a_kind_plain(2, n_kept, 0, h_cross);
  k.version = kAttrNVersion;
  k.nbr = true;
  return k;
}
// versions 28 and 31: version 7's kind under the neighbour predictor's closed loop
static AEncKind a_kind_nbr_nl(int64_t n_kept, int max_error, const int32_t* h_cross) {
  AEncKind k = a_kind_plain(2, n_kept, max_error, h_cross);
  k.version = kAttrNLVersion;
  k.nbr = true;
  return k;
}
static AEncKind a_kind_transform(int64_t n_kept, int qstep, const int32_t* h_qsteps, int colour, int K = 0) {
  const bool tc = h_qsteps != nullptr;
  return AEncKind{K ? kAttrSVersion : (tc ? kAttrCVersion : kAttrTVersion), false, true, true, tc, K ? K : (tc ? 1 : qstep), n_kept, nullptr,
                  h_qsteps, colour, K};
}

// bytes of a blob in front of its chunk payloads: the kind's head, p0 and the chunk table
static int64_t a_head_bytes(const AEncKind& k, int c, int nctx, int64_t nc) {
  const int64_t head = k.K ? attr_s_head(c) : k.tc ? attr_c_head(c) : (k.tr ? kAttrTHead : (k.v2 ? kAttr2Head : kAttrHead + 8) + (k.nl ? 4 : 0));
  return head + 2 * nctx + 4 * nc;
}

// the template arguments of a kind's coder: k_a_stats / k_a_enc<PRED>, k_a_pack<V2, NL, XC, TR> (a_launch_pack)
template <bool V2_, bool NL_, bool XC_, bool TR_ = false>
struct ACoder {
  static constexpr bool V2 = V2_, NL = NL_, XC = XC_, TR = TR_;
  static constexpr bool PRED = !V2 && !NL && !XC;   // only version 1 predicts inside the run, and not beside cross-channel frames
};

// the arguments every encode entry point shares, checked; *n_keys = the sorted keys that belong to kept rows (no run may
// reach a dropped row's key)
static int a_check_call(const char* who, const AEncKind& k, pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets,
                        const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames, const uint32_t* d_perm,
                        const uint32_t* d_run_starts, int64_t n_unique, const uint64_t* d_keys, int key_shift, uint8_t* h_out,
                        int64_t cap, int64_t* h_offsets, int64_t* n_keys) {
  const bool drops = k.n_kept >= 0;
  PCC_REQUIRE(ctx && h_value_offsets && h_format && h_rows && h_points && h_out && h_offsets && n_frames >= 1 &&
                  n_frames <= 65535 && n_unique >= 0 && cap >= 0,
              PCC_E_ARG, "%s: bad argument (n_frames=%d)", who, n_frames);
  PCC_REQUIRE(!drops || k.n_kept <= h_rows[n_frames], PCC_E_ARG, "%s: %lld kept rows of %lld", who, (long long)k.n_kept,
              (long long)h_rows[n_frames]);
  *n_keys = drops ? k.n_kept : h_rows[n_frames];
  PCC_REQUIRE(h_rows[0] == 0 && h_rows[n_frames] < ((int64_t)1 << 27) && n_unique <= *n_keys &&
                  (*n_keys == 0 || (d_values && d_perm && d_run_starts)),
              PCC_E_ARG, "%s: %lld rows, %lld points", who, (long long)*n_keys, (long long)n_unique);
  PCC_REQUIRE(!k.keyed() || (key_shift >= 0 && key_shift <= 45 && key_shift % 3 == 0 && (*n_keys == 0 || d_keys)), PCC_E_ARG,
              "%s: bad argument (key_shift=%d)", who, key_shift);
  PCC_REQUIRE(!k.K || k.K + key_shift / 3 <= kAttrMaxLod, PCC_E_ARG, "%s: scalable_to %d with key_shift %d: beyond level of detail %d", who,
              k.K, key_shift, kAttrMaxLod);
  return PCC_OK;
}

// frame f of an encode call, checked as its kind asks.  *r: its row of the coder's table but for its places in the
// call's arrays (u0, val_off, rec_off, ctx_off, out_off, cb, sb, mb), which the caller counts; r->n = 0: no points, no row
static int a_check_frame(const char* who, const AEncKind& k, int f, const int64_t* h_value_offsets, const int32_t* h_format,
                         const int64_t* h_rows, const int64_t* h_points, AFrame* r) {
  const int bpv = h_format[f] & 0xFF, c = h_format[f] >> 8;
  const int64_t rows = h_rows[f + 1] - h_rows[f], n = h_points[f];
  PCC_REQUIRE((bpv == 1 || bpv == 2) && c >= 1 && c <= 4, PCC_E_ARG, "%s: frame %d: format %d", who, f,
              h_format[f]);
  PCC_REQUIRE(rows >= 0 && n >= 0 && n <= rows && ((n == 0) == (rows == 0) || (k.n_kept >= 0 && n == 0)) &&
                  h_value_offsets[f] >= 0, PCC_E_ARG,
              "%s: frame %d: %lld rows, %lld points", who, f, (long long)rows, (long long)n);
  PCC_REQUIRE(!k.nl || k.tc || (uint32_t)k.e <= attr_max_error(bpv), PCC_E_ARG,
              "%s: frame %d: %s %d with %d bytes per value (at most %u)", who, f, k.tr ? "qstep" : "max_error", k.e, bpv,
              attr_max_error(bpv));
  if (k.tc) {
    for (int ch = 0; ch < c; ++ch)
      PCC_REQUIRE(k.h_qsteps[ch] >= 1 && (uint32_t)k.h_qsteps[ch] <= attr_max_error(bpv), PCC_E_ARG,
                  "%s: frame %d: qstep %d of channel %d with %d bytes per value (1 .. %u)", who, f, k.h_qsteps[ch], ch, bpv,
                  attr_max_error(bpv));
    PCC_REQUIRE(!k.colour || c >= 3, PCC_E_ARG, "%s: frame %d: the colour transform needs 3 channels, the frame has %d", who, f, c);
  }
  const int32_t m = k.h_cross ? k.h_cross[f] : 0;
  PCC_REQUIRE(m >= 0 && m < (1 << (c - 1)), PCC_E_ARG, "%s: frame %d: cross-channel mask %d with %d channels", who, f, m, c);
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  *r = AFrame{};
  r->e = k.e;
  r->in_off = h_value_offsets[f];
  r->row0 = h_rows[f];
  r->rows = rows;
  r->n = n;
  r->c = c;
  r->bpv = bpv;
  r->nctx = attr_contexts(bpv, c);
  r->T = (int32_t)(S * c * attr_positions(bpv));
  // a coded decision emits at most one word: the bound follows the frame's decisions, not its chunks' regions
  r->out_cap = a_head_bytes(k, c, r->nctx, nc) + 2 * (3 * kLanes * nc + std::min<int64_t>(nc * kLanes * r->T, (int64_t)attr_positions(bpv) * c * n));
  r->S = (int32_t)S;
  r->nc = (int32_t)nc;
  r->sn = (int32_t)std::min<unsigned>(nblk(n, 256), 256u);
  return PCC_OK;
}

// What the encode entry points share of a call: its arguments checked and its frames laid out.  The frames with points
// (nf of them; frame_of: which of the call's) get a row of the coder's table with their places among the call's points,
// merged values, merge blocks and output staging; the places among the coder's own arrays (rec_off, ctx_off, cb, sb) are
// the caller's, which codes the frames once (a_encode_frames) or as candidate rows (pcc_attr_encode_frames_rate)
struct AEncPlan {
  int64_t n_keys = 0;           // the sorted keys that belong to kept rows (a_check_call)
  std::vector<AFrame> tab;
  std::vector<A2Order> order;   // their order rows (read by the keyed kinds)
  std::vector<int> frame_of;
  std::vector<int32_t> cross;   // their masks
  std::vector<int32_t> aux;     // the transform kinds: their q[4] and the colour word (version 19: q in every channel)
  bool xc = false;              // one of the masks is not 0
  int64_t n_max = 0;            // the most points of a frame
  int64_t u = 0, vals = 0, out_bytes = 0, merge_blocks = 0, nctx_max = 0;
  int nf() const { return (int)tab.size(); }
};

// a_check_call, then frame by frame a_check_frame, the frame's row where it has points (row: nullptr where it has none)
// and per_frame(f, row): the caller's own checks of frame f and its places in row; last the points against the runs
template <typename PerFrame>
static int a_enc_front(const char* who, const AEncKind& k, pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets,
                       const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames, const uint32_t* d_perm,
                       const uint32_t* d_run_starts, int64_t n_unique, const uint64_t* d_keys, int key_shift, uint8_t* h_out, int64_t cap,
                       int64_t* h_offsets, AEncPlan* pl, PerFrame&& per_frame) {
  PCC_TRY(a_check_call(who, k, ctx, d_values, h_value_offsets, h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys,
                       key_shift, h_out, cap, h_offsets, &pl->n_keys));
  for (int f = 0; f < n_frames; ++f) {
    AFrame r;
    PCC_TRY(a_check_frame(who, k, f, h_value_offsets, h_format, h_rows, h_points, &r));
    AFrame* row = nullptr;
    if (r.n > 0) {
      const int32_t m = k.h_cross ? k.h_cross[f] : 0;
      pl->cross.push_back(m);
      pl->xc |= m != 0;
      if (k.tr) {
        for (int ch = 0; ch < 4; ++ch) pl->aux.push_back(ch < r.c ? (k.h_qsteps ? k.h_qsteps[ch] : k.e) : 0);
        pl->aux.push_back(k.colour);
      }
      r.u0 = pl->u;
      r.val_off = pl->vals;
      r.out_off = pl->out_bytes;
      r.mb = (int32_t)pl->merge_blocks;
      pl->tab.push_back(r);
      pl->order.push_back(A2Order{r.u0, r.n, r.mb, key_shift});
      pl->frame_of.push_back(f);
      pl->n_max = std::max(pl->n_max, r.n);
      pl->u += r.n;
      pl->vals += r.n * r.c;
      pl->out_bytes += a_round(r.out_cap, 16);
      pl->merge_blocks += nblk(r.n, 256);
      pl->nctx_max = std::max<int64_t>(pl->nctx_max, r.nctx);
      row = &pl->tab.back();
    }
    PCC_TRY(per_frame(f, row));
  }
  PCC_REQUIRE(pl->u == n_unique, PCC_E_ARG, "%s: the frames have %lld points, the runs %lld", who, (long long)pl->u, (long long)n_unique);
  return PCC_OK;
}

// the blobs of a call on their way out: frame f's length (the empty blob's where it has no points) and where it lies in
// the staging (-1: nowhere)
struct AEncOut {
  std::vector<int64_t> len_of, off_of;
  explicit AEncOut(int n_frames) : len_of((size_t)n_frames, kAttrHead), off_of((size_t)n_frames, -1) {}
  // row i of the plan: the length k_a_pack reported for it, its blob at out_off behind the tab_b bytes of tables
  int take(const char* who, const AEncPlan& pl, int i, long long total, size_t tab_b) {
    const AFrame& r = pl.tab[(size_t)i];
    const int f = pl.frame_of[(size_t)i];
    PCC_REQUIRE(total >= 0 && total <= r.out_cap, PCC_E_NOMEM, "%s: frame %d: blob beyond its bound", who, f);
    len_of[(size_t)f] = total;
    off_of[(size_t)f] = (int64_t)tab_b + r.out_off;
    return PCC_OK;
  }
};

// the end of an encode call: the blobs against the capacity, out of the staging one behind the other, the 12-byte
// empty blob of a frame without points (its kind's version byte, or the cross form's under a mask), and h_offsets
static int a_enc_emit(const char* who, const AEncKind& k, pcc_ctx* ctx, const int32_t* h_format, int n_frames, int key_shift,
                      const AEncOut& o, uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  int64_t total = 0;
  for (int f = 0; f < n_frames; ++f) total += o.len_of[(size_t)f];
  PCC_REQUIRE(total <= cap, PCC_E_NOMEM, "%s: %lld bytes of blobs, capacity %lld", who, (long long)total, (long long)cap);
  h_offsets[0] = 0;
  for (int f = 0; f < n_frames; ++f) {
    uint8_t* dst = h_out + h_offsets[f];
    if (o.off_of[(size_t)f] >= 0) {
      memcpy(dst, (const uint8_t*)ctx->stage + o.off_of[(size_t)f], (size_t)o.len_of[(size_t)f]);
      // versions 25 / 26: k_a_pack wrote version 2's / 11's head, which is theirs but for the version byte
      // (versions 28 / 31: version 7's / 14's)
      if (k.nbr) dst[1] = (uint8_t)attr_version(true, k.nl, dst[1] == attr_version(true, k.nl, true), true);
    } else {
      const int32_t m = k.h_cross ? k.h_cross[f] : 0;
      memset(dst, 0, kAttrHead);
      dst[0] = 'A';
      dst[1] = (uint8_t)(m ? attr_version(k.v2, k.nl, true, k.nbr) : k.version);
      dst[2] = (uint8_t)((h_format[f] & 0xFF) | (k.keyed() ? (key_shift / 3) << 4 : 0));
      dst[3] = (uint8_t)((h_format[f] >> 8) | (m << 4));
    }
    h_offsets[f + 1] = h_offsets[f] + o.len_of[(size_t)f];
  }
  return PCC_OK;
}

// what k_a_enc leaves per chunk besides the words: one array of the arena, carved into the chunks' word counts | their
// lanes' final states | their lanes' lengths
struct ASmall {
  uint32_t* words = nullptr;
  uint16_t *states = nullptr, *lens = nullptr;
  static size_t bytes(int64_t chunks) { return pcc_align((size_t)chunks * (4 + 2 * kLanes * 2 + kLanes * 2)); }
  ASmall() = default;
  ASmall(char* p, int64_t chunks)
      : words((uint32_t*)p), states((uint16_t*)(p + (size_t)chunks * 4)), lens(states + (size_t)chunks * 2 * kLanes) {}
  ASmall from(int64_t cb) const {   // the same arrays from chunk cb on
    ASmall s = *this;
    s.words += cb, s.states += cb * 2 * kLanes, s.lens += cb * kLanes;
    return s;
  }
};

// k_a_pack over `blocks` workgroups (the rows' chunks and one per row) in the Aux form of the kind: version 22's (TR with
// V2: d_aux, K), version 21's (TR and a table d_aux), or none
template <bool V2, bool NL, bool XC, bool TR>
static int a_launch_pack(hipStream_t st, unsigned blocks, const uint16_t* work, const AFrame* d_tab, int nf, const ASmall& sm,
                         const uint16_t* p0, uint8_t* out, long long* len_out, const uint32_t* cells, int slod, const int32_t* d_cross,
                         const int32_t* d_aux, int K) {
  const auto launch = [&](auto kernel, auto... aux) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, work, d_tab, nf, (const uint16_t*)sm.states, (const uint16_t*)sm.lens,
                       (const uint32_t*)sm.words, p0, out, len_out, cells, slod, d_cross, aux...);
  };
  if constexpr (TR && V2) {
    launch(k_a_pack<V2, NL, XC, TR, const int32_t*, int>, d_aux, K);
  } else if constexpr (TR) {
    if (d_aux) launch(k_a_pack<V2, NL, XC, TR, const int32_t*>, d_aux);
    else launch(k_a_pack<V2, NL, XC, TR>);
  } else {
    launch(k_a_pack<V2, NL, XC, TR>);
  }
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// the encoder of every kind: k_a_merge, the kind's passes of the table above, k_ax_fwd in a call with any m != 0 among
// its frames with points (every frame is then coded with PRED = false), counting pass, coder, blobs
static int a_encode_frames(const char* who, const AEncKind& k, pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets,
                           const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames,
                           const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique, const uint64_t* d_keys,
                           int key_shift, uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  const bool v2 = k.v2, nl = k.nl, tr = k.tr, tc = k.tc, sc = k.K > 0, keyed = k.keyed();
  AEncPlan pl;
  int64_t run_threads = 0;   // k_a4_quant: the most (run, channel) pairs of a frame
  int64_t rec_words = 0, chunks = 0, stats_blocks = 0, ctxs = 0;
  PCC_TRY(a_enc_front(who, k, ctx, d_values, h_value_offsets, h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys,
                      key_shift, h_out, cap, h_offsets, &pl, [&](int, AFrame* r) -> int {
                        if (!r) return PCC_OK;
                        r->rec_off = rec_words;
                        r->ctx_off = (int32_t)ctxs;
                        r->cb = (int32_t)chunks;
                        r->sb = (int32_t)stats_blocks;
                        run_threads = std::max<int64_t>(run_threads, (int64_t)r->nc * kLanes * r->c);
                        rec_words += (int64_t)r->nc * kLanes * r->T;
                        chunks += r->nc;
                        stats_blocks += r->sn;
                        ctxs += r->nctx;
                        return PCC_OK;
                      }));
  const int nf = pl.nf();
  const bool xc = pl.xc;
  const int64_t u = pl.u, vals = pl.vals, merge_blocks = pl.merge_blocks, n_max = pl.n_max;
  AEncOut out(n_frames);
  hipStream_t st = ctx->stream;
  if (nf > 0) {
    // the rows | the masks (a call with cross-channel frames) | steps and colour (version 21) | the order rows
    ATables lay;
    lay.add((size_t)nf * sizeof(AFrame));
    const size_t cross_at = lay.add(xc ? (size_t)nf * 4 : 0), aux_at = lay.add(tc ? (size_t)nf * 20 : 0);
    const size_t ord_at = lay.add(keyed ? (size_t)nf * sizeof(A2Order) : 0), tab_b = lay.bytes;
    const size_t merged_b = merged_b_of(vals), cnt_b = pcc_align((size_t)ctxs * 8), p0_b = pcc_align((size_t)ctxs * 2);
    const size_t rec_b = pcc_align((size_t)rec_words * 2), small_b = ASmall::bytes(chunks);
    // the order stage's (versions 2 and 7): packed | hist | 17 bin bases, then 16 counts per frame; rank, first (7)
    const size_t pk_b = pcc_align((size_t)u * 2), hist_b = pcc_align((size_t)merge_blocks * kA2Bins * 4);
    const size_t bins_b = pcc_align((size_t)nf * 33 * 4), link_b = pcc_align((size_t)u * 4);
    // src is one more array of the merged values' size.  The sum counts it twice for version 2 and the links for
    // version 4 too (one of them beside a_t_order_bytes', which has version 19's): it is what these calls have always
    // reserved, and no call reserves less than it did
    const size_t order_b = v2 ? 2 * merged_b + pk_b + hist_b + bins_b : 0, nl_b = nl ? merged_b + (tr ? 1 : 2) * link_b : 0;
    const size_t x8_b = xc && !v2 && !nl ? merged_b : 0;   // version 8: the run residuals
    const size_t tr_b = (tr ? a_t_order_bytes(u, merge_blocks, nf) : 0) + (sc ? a_s_cells_bytes(u) + pcc_align((size_t)nf * 64) : 0);
    // versions 28 / 31: the reconstructions (one more array of the merged values' size), every point's choice, 3 words
    const size_t picks_b = pcc_align((size_t)u * 12), nbr_nl_b = k.nbr && nl ? merged_b + picks_b : 0;
    PCC_TRY(pcc_arena_reserve(ctx, tab_b + merged_b + cnt_b + p0_b + 2 * rec_b + small_b + order_b + nl_b + x8_b + tr_b + nbr_nl_b + 8192));
    AFrame* d_tab = (AFrame*)pcc_arena_alloc(ctx, tab_b);
    uint16_t* merged = (uint16_t*)pcc_arena_alloc(ctx, merged_b);
    uint32_t* cnt = (uint32_t*)pcc_arena_alloc(ctx, cnt_b);
    uint16_t* p0 = (uint16_t*)pcc_arena_alloc(ctx, p0_b);
    uint16_t* rec = (uint16_t*)pcc_arena_alloc(ctx, rec_b);
    uint16_t* work = (uint16_t*)pcc_arena_alloc(ctx, rec_b);
    char* small = (char*)pcc_arena_alloc(ctx, small_b);
    // what the lanes code: the merged values (version 1), their residuals in introduction order (2), the indices (4, 7);
    // a call with cross-channel frames: the run residuals (8) and all of these after k_ax_fwd
    uint16_t* src = v2 || nl || xc ? (uint16_t*)pcc_arena_alloc(ctx, merged_b) : merged;
    if (!d_tab || !merged || !cnt || !p0 || !rec || !work || !small || !src) return PCC_E_NOMEM;
    const ASmall sm(small, chunks);
    const A2Order* d_ord = (const A2Order*)((const uint8_t*)d_tab + ord_at);
    const int32_t* d_cross = xc ? (const int32_t*)((const uint8_t*)d_tab + cross_at) : nullptr;
    const int32_t* d_aux = tc ? (const int32_t*)((const uint8_t*)d_tab + aux_at) : nullptr;
    // staging: the table on its way to the device | the blobs | their lengths
    const size_t lens_at = tab_b + (size_t)pl.out_bytes;
    const size_t tcnt_at = lens_at + (size_t)nf * 8 + 64;   // version 19: the sublevels' starts and counts, read back
    PCC_TRY(o2_stage_reserve(ctx, tcnt_at + (tr ? (size_t)nf * 2 * kATBins * 4 : 0) + 64));
    uint8_t* stage = (uint8_t*)ctx->stage;
    memcpy(stage, pl.tab.data(), (size_t)nf * sizeof(AFrame));
    if (xc) memcpy(stage + cross_at, pl.cross.data(), (size_t)nf * 4);
    if (tc) memcpy(stage + aux_at, pl.aux.data(), (size_t)nf * 20);
    if (keyed) memcpy(stage + ord_at, pl.order.data(), (size_t)nf * sizeof(A2Order));
    long long* len_dev = (long long*)(stage + lens_at);
    PccProfScope prof(ctx, "attr_encode", u, nf, chunks, 0);
    PCC_HIP(hipMemcpyAsync(d_tab, stage, lay.end, hipMemcpyHostToDevice, st));
    PCC_HIP(hipMemsetAsync(cnt, 0, (size_t)ctxs * 8, st));
    hipLaunchKernelGGL(k_a_merge, dim3((unsigned)merge_blocks), dim3(256), 0, st, (const uint8_t*)d_values, (const AFrame*)d_tab, nf,
                       d_perm, d_run_starts, n_unique, pl.n_keys, merged);
    PCC_CHECK_LAUNCH();
    // the introduction order of the frames' points.  keep = false (version 2): the residuals against the predictors go
    // to src; keep (version 7): places and predictors are kept for k_a7_quant
    uint32_t *cells = nullptr, *rank = nullptr, *first = nullptr;
    auto a_order_stage = [&](bool keep) -> int {
      if (keep) {
        rank = (uint32_t*)pcc_arena_alloc(ctx, link_b);
        first = (uint32_t*)pcc_arena_alloc(ctx, link_b);
      }
      uint16_t* packed = (uint16_t*)pcc_arena_alloc(ctx, pk_b);
      uint32_t* hist = (uint32_t*)pcc_arena_alloc(ctx, hist_b);
      uint32_t* bins = (uint32_t*)pcc_arena_alloc(ctx, bins_b);
      if ((keep && (!rank || !first)) || !packed || !hist || !bins) return PCC_E_NOMEM;
      cells = bins + (size_t)nf * kA2Bins;
      hipLaunchKernelGGL(k_a2_size<false>, dim3((unsigned)merge_blocks), dim3(256), 0, st, (const void*)d_keys, d_ord, nf,
                         (uint64_t*)nullptr, packed, hist);
      PCC_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_a2_scan, dim3((unsigned)nf), dim3(256), 0, st, d_ord, hist, bins, cells);
      PCC_CHECK_LAUNCH();
      if (k.nbr && !nl) {   // versions 25 / 26: the residuals against the neighbour predictor, in one pass of its own
        hipLaunchKernelGGL(k_an_place, dim3((unsigned)merge_blocks), dim3(256), 0, st, d_keys, d_ord, nf, (const uint16_t*)packed,
                           (const uint32_t*)hist, (const uint32_t*)bins, (const AFrame*)d_tab, (const uint16_t*)merged, src);
        PCC_CHECK_LAUNCH();
        return PCC_OK;
      }
      if (k.nbr) {
        // versions 28 / 31: every point's choice once (rank holds the inverse of the places), then the closed loop size
        // by size, all frames in one grid.  The host has no count per size and does not wait for one: a frame of n
        // points on a lattice of L bits per axis has at most min(n, 8^(L - s)) points of size s < L, point 0 alone at
        // 16 and none between, so sizes L .. 15 are not launched and the others get a grid of that bound; the ranges
        // themselves are the order stage's, on the device, and a block beyond a range returns at once
        uint32_t* picks = (uint32_t*)pcc_arena_alloc(ctx, picks_b);
        uint16_t* recon = (uint16_t*)pcc_arena_alloc(ctx, merged_b);
        if (!picks || !recon) return PCC_E_NOMEM;
        hipLaunchKernelGGL(k_anl_plan, dim3((unsigned)merge_blocks), dim3(256), 0, st, d_keys, d_ord, nf, (const uint16_t*)packed,
                           (const uint32_t*)hist, (const uint32_t*)bins, rank, picks);
        PCC_CHECK_LAUNCH();
        const int L = 16 - key_shift / 3;
        for (int s = kA2Bins - 1; s >= 0; --s) {
          if (s < 16 && s >= L) continue;
          const int64_t most = s == 16 ? 1 : (3 * (L - s) >= 27 ? n_max : std::min<int64_t>(n_max, (int64_t)1 << (3 * (L - s))));
          hipLaunchKernelGGL(k_anl_quant, dim3(nblk(most, 256), (unsigned)nf), dim3(256), 0, st, d_ord, (const AFrame*)d_tab,
                             (const uint32_t*)bins, s, (const uint32_t*)rank, (const uint32_t*)picks, (const uint16_t*)merged, recon, src);
          PCC_CHECK_LAUNCH();
        }
        return PCC_OK;
      }
      const auto place = keep ? k_a2_place<true, true> : k_a2_place<true, false>;
      hipLaunchKernelGGL(place, dim3((unsigned)merge_blocks), dim3(256), 0, st, d_keys, d_ord, nf, (const uint16_t*)packed,
                         (const uint32_t*)hist, (const uint32_t*)bins, (const AFrame*)d_tab, (const uint16_t*)merged,
                         keep ? (uint16_t*)nullptr : src, rank, first);
      PCC_CHECK_LAUNCH();
      return PCC_OK;
    };
    if (v2) PCC_TRY(a_order_stage(nl));
    if (tr) {
      if (tc && k.colour) {
        hipLaunchKernelGGL(k_ac_fwd, dim3(nblk(n_max, 256), (unsigned)nf), dim3(256), 0, st, (const AFrame*)d_tab, d_aux, merged);
        PCC_CHECK_LAUNCH();
      }
      PCC_TRY(a_t_forward(ctx, st, d_keys, d_ord, (const AFrame*)d_tab, nf, merge_blocks, u, merged, src, (uint32_t*)(stage + tcnt_at), d_aux,
                          sc ? &cells : nullptr));
    } else if (nl && !v2) {
      hipLaunchKernelGGL(k_a4_quant, dim3(nblk(run_threads, 256), (unsigned)nf), dim3(256), 0, st, (const uint16_t*)merged,
                         (const AFrame*)d_tab, src);
      PCC_CHECK_LAUNCH();
    } else if (nl && !k.nbr) {
      hipLaunchKernelGGL(k_a7_quant, dim3((unsigned)merge_blocks), dim3(256), 0, st, d_ord, nf, (const AFrame*)d_tab,
                         (const uint16_t*)merged, (const uint32_t*)rank, (const uint32_t*)first, src);
      PCC_CHECK_LAUNCH();
    }
    if (xc) {
      const auto fwd = !v2 && !nl ? k_ax_fwd<true> : k_ax_fwd<false>;
      hipLaunchKernelGGL(fwd, dim3(nblk(n_max, 256), (unsigned)nf), dim3(256), 0, st, (const AFrame*)d_tab, d_cross,
                         (const uint16_t*)merged, src);
      PCC_CHECK_LAUNCH();
    }
    // counting pass, coder, blobs
    const size_t lds = 4096 * 4 + (size_t)(pl.nctx_max + 1) * kLanes * 2;   // <= 98 KB (c = 4, uint16)
    auto a_code = [&](auto coder) -> int {
      using K = decltype(coder);
      constexpr bool PRED = K::PRED;
      hipLaunchKernelGGL(k_a_stats<PRED>, dim3((unsigned)stats_blocks), dim3(256), 0, st, (const uint16_t*)src, (const AFrame*)d_tab, nf, cnt);
      PCC_CHECK_LAUNCH();
      PCC_HIP(hipFuncSetAttribute((const void*)k_a_enc<PRED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(k_a_enc<PRED>, dim3((unsigned)chunks), dim3(64), lds, st, (const uint16_t*)src, (const AFrame*)d_tab, nf,
                         (const uint32_t*)cnt, rec, work, sm.states, sm.lens, sm.words, p0);
      PCC_CHECK_LAUNCH();
      return a_launch_pack<K::V2, K::NL, K::XC, K::TR>(st, (unsigned)(chunks + nf), work, d_tab, nf, sm, p0, stage + tab_b, len_dev, cells,
                                                       key_shift / 3, d_cross, d_aux, k.K);
    };
    // by the version byte of the call's frames with a mask, where it has any, else of its plain frames
    int rc = PCC_E_ARG;
    // (versions 25 / 26 are coded, packed and laid out as 2 / 11, versions 28 / 31 as 7 / 14)
    switch (xc ? attr_version(v2, nl, true) : (k.nbr ? attr_version(true, nl, false) : k.version)) {   //   V2     NL     XC     TR
      case 1: rc = a_code(ACoder<false, false, false>{}); break;
      case 2: rc = a_code(ACoder<true, false, false>{}); break;
      case 4: rc = a_code(ACoder<false, true, false>{}); break;
      case 7: rc = a_code(ACoder<true, true, false>{}); break;
      case 8: rc = a_code(ACoder<false, false, true>{}); break;
      case 11: rc = a_code(ACoder<true, false, true>{}); break;
      case 13: rc = a_code(ACoder<false, true, true>{}); break;
      case 14: rc = a_code(ACoder<true, true, true>{}); break;
      case kAttrTVersion:
      case kAttrCVersion: rc = a_code(ACoder<false, true, false, true>{}); break;   // 21: with its table (d_aux)
      case kAttrSVersion: rc = a_code(ACoder<true, true, false, true>{}); break;    // V2: the 16 counts in the head
    }
    PCC_TRY(rc);
    PCC_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < nf; ++i) PCC_TRY(out.take(who, pl, i, ((volatile long long*)len_dev)[i], tab_b));
  }
  return a_enc_emit(who, k, ctx, h_format, n_frames, key_shift, out, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets, const int32_t* h_format,
                                      const int64_t* h_rows, const int64_t* h_points, int n_frames, const uint32_t* d_perm,
                                      const uint32_t* d_run_starts, int64_t n_unique, uint8_t* h_out, int64_t cap,
                                      int64_t* h_offsets) {
  return a_encode_frames("pcc_attr_encode_frames", a_kind_plain(1, -1, 0, nullptr), ctx, d_values, h_value_offsets, h_format, h_rows,
                         h_points, n_frames, d_perm, d_run_starts, n_unique, nullptr, 0, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_v2(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets, const int32_t* h_format,
                                         const int64_t* h_rows, const int64_t* h_points, int n_frames, const uint32_t* d_perm,
                                         const uint32_t* d_run_starts, int64_t n_unique, const uint64_t* d_keys, int key_shift,
                                         uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  return a_encode_frames("pcc_attr_encode_frames_v2", a_kind_plain(2, -1, 0, nullptr), ctx, d_values, h_value_offsets, h_format, h_rows,
                         h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys, key_shift, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_kept(pcc_ctx* ctx, int version, const void* d_values, const int64_t* h_value_offsets,
                                           const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames,
                                           const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept,
                                           const uint64_t* d_keys, int key_shift, uint8_t* h_out, int64_t cap,
                                           int64_t* h_offsets) {
  PCC_REQUIRE((version == 1 || version == 2) && n_kept >= 0, PCC_E_ARG,
              "pcc_attr_encode_frames_kept: bad argument (version=%d n_kept=%lld)", version, (long long)n_kept);
  return a_encode_frames("pcc_attr_encode_frames_kept", a_kind_plain(version, n_kept, 0, nullptr), ctx, d_values, h_value_offsets, h_format,
                         h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, version == 2 ? d_keys : nullptr,
                         version == 2 ? key_shift : 0, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_nl(pcc_ctx* ctx, int version, const void* d_values, const int64_t* h_value_offsets,
                                         const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames,
                                         const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept,
                                         const uint64_t* d_keys, int key_shift, int max_error, uint8_t* h_out, int64_t cap,
                                         int64_t* h_offsets) {
  PCC_REQUIRE((version == 1 || version == 2) && n_kept >= -1 && max_error >= 0, PCC_E_ARG,
              "pcc_attr_encode_frames_nl: bad argument (version=%d n_kept=%lld max_error=%d)", version, (long long)n_kept, max_error);
  return a_encode_frames("pcc_attr_encode_frames_nl", a_kind_plain(version, n_kept, max_error, nullptr), ctx, d_values, h_value_offsets,
                         h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, version == 2 ? d_keys : nullptr,
                         version == 2 ? key_shift : 0, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_cross(pcc_ctx* ctx, int version, const void* d_values, const int64_t* h_value_offsets,
                                            const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames,
                                            const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept,
                                            const uint64_t* d_keys, int key_shift, int max_error, const int32_t* h_cross,
                                            uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  PCC_REQUIRE((version == 1 || version == 2) && n_kept >= -1 && max_error >= 0 && h_cross, PCC_E_ARG,
              "pcc_attr_encode_frames_cross: bad argument (version=%d n_kept=%lld max_error=%d)", version, (long long)n_kept, max_error);
  return a_encode_frames("pcc_attr_encode_frames_cross", a_kind_plain(version, n_kept, max_error, h_cross), ctx, d_values, h_value_offsets,
                         h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, version == 2 ? d_keys : nullptr,
                         version == 2 ? key_shift : 0, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_nbr(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets, const int32_t* h_format,
                                          const int64_t* h_rows, const int64_t* h_points, int n_frames, const uint32_t* d_perm,
                                          const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept, const uint64_t* d_keys,
                                          int key_shift, const int32_t* h_cross, uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  PCC_REQUIRE(n_kept >= -1, PCC_E_ARG, "pcc_attr_encode_frames_nbr: bad argument (n_kept=%lld)", (long long)n_kept);
  return a_encode_frames("pcc_attr_encode_frames_nbr", a_kind_nbr(n_kept, h_cross), ctx, d_values, h_value_offsets, h_format, h_rows,
                         h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys, key_shift, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_nbr_nl(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets, const int32_t* h_format,
                                             const int64_t* h_rows, const int64_t* h_points, int n_frames, const uint32_t* d_perm,
                                             const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept, const uint64_t* d_keys,
                                             int key_shift, int max_error, const int32_t* h_cross, uint8_t* h_out, int64_t cap,
                                             int64_t* h_offsets) {
  PCC_REQUIRE(n_kept >= -1 && max_error >= 1, PCC_E_ARG, "pcc_attr_encode_frames_nbr_nl: bad argument (n_kept=%lld max_error=%d)",
              (long long)n_kept, max_error);
  return a_encode_frames("pcc_attr_encode_frames_nbr_nl", a_kind_nbr_nl(n_kept, max_error, h_cross), ctx, d_values, h_value_offsets,
                         h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys, key_shift, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_transform(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets,
                                                const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames,
                                                const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept,
                                                const uint64_t* d_keys, int key_shift, int qstep, uint8_t* h_out, int64_t cap,
                                                int64_t* h_offsets) {
  PCC_REQUIRE(n_kept >= -1 && qstep >= 1, PCC_E_ARG, "pcc_attr_encode_frames_transform: bad argument (n_kept=%lld qstep=%d)",
              (long long)n_kept, qstep);
  return a_encode_frames("pcc_attr_encode_frames_transform", a_kind_transform(n_kept, qstep, nullptr, 0), ctx, d_values, h_value_offsets,
                         h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys, key_shift, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_transform2(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets,
                                                 const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames,
                                                 const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept,
                                                 const uint64_t* d_keys, int key_shift, const int32_t h_qstep[4], int colour,
                                                 uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  PCC_REQUIRE(n_kept >= -1 && h_qstep && (colour == 0 || colour == 1), PCC_E_ARG,
              "pcc_attr_encode_frames_transform2: bad argument (n_kept=%lld colour=%d)", (long long)n_kept, colour);
  return a_encode_frames("pcc_attr_encode_frames_transform2", a_kind_transform(n_kept, 0, h_qstep, colour), ctx, d_values, h_value_offsets,
                         h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys, key_shift, h_out, cap, h_offsets);
}

extern "C" int pcc_attr_encode_frames_transform3(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets,
                                                 const int32_t* h_format, const int64_t* h_rows, const int64_t* h_points, int n_frames,
                                                 const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept,
                                                 const uint64_t* d_keys, int key_shift, const int32_t h_qstep[4], int colour,
                                                 int scalable_to, uint8_t* h_out, int64_t cap, int64_t* h_offsets) {
  PCC_REQUIRE(n_kept >= -1 && h_qstep && (colour == 0 || colour == 1) && scalable_to >= 1 && scalable_to <= kAttrMaxLod, PCC_E_ARG,
              "pcc_attr_encode_frames_transform3: bad argument (n_kept=%lld colour=%d scalable_to=%d)", (long long)n_kept, colour, scalable_to);
  return a_encode_frames("pcc_attr_encode_frames_transform3", a_kind_transform(n_kept, 0, h_qstep, colour, scalable_to), ctx, d_values,
                         h_value_offsets, h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys, key_shift, h_out, cap,
                         h_offsets);
}

// ---- versions 19 and 21 under a byte target per frame (include/pcc.h states the ladder and the search) --------------
constexpr int kARMaxRungs = 64;                         // uint16, q = 1: 61
constexpr int64_t kARScratchDefault = (int64_t)1 << 30;   // scratch_limit = 0

// the ladder of base steps q[0 .. c): steps[j][ch] (0 behind c); returns J
static int a_r_ladder(const int32_t* q, int c, int bpv, int32_t (*steps)[4]) {
  static const int64_t mul[4] = {16, 19, 23, 27};
  const int64_t top = ((int64_t)1 << (8 * bpv - 1)) - 1;
  for (int j = 0; j < kARMaxRungs; ++j) {
    bool last = true;
    for (int ch = 0; ch < 4; ++ch) {
      const int64_t s = ch < c ? std::min<int64_t>(top, (((int64_t)q[ch] * mul[j % 4]) << (j / 4)) >> 4) : 0;
      steps[j][ch] = (int32_t)s;
      last &= ch >= c || s == top;
    }
    if (last) return j + 1;
  }
  return kARMaxRungs;   // not reached: q >= 1 is at H - 1 from rung 60 on
}

extern "C" int pcc_attr_rate_ladder(const int32_t h_qstep[4], int c, int bpv, int32_t* h_steps, int32_t* h_rungs) {
  PCC_REQUIRE(h_qstep && h_steps && h_rungs && (bpv == 1 || bpv == 2) && c >= 1 && c <= 4, PCC_E_ARG,
              "pcc_attr_rate_ladder: bad argument (c=%d bpv=%d)", c, bpv);
  for (int ch = 0; ch < c; ++ch)
    PCC_REQUIRE(h_qstep[ch] >= 1 && (uint32_t)h_qstep[ch] <= attr_max_error(bpv), PCC_E_ARG,
                "pcc_attr_rate_ladder: qstep %d of channel %d with %d bytes per value (1 .. %u)", h_qstep[ch], ch, bpv, attr_max_error(bpv));
  *h_rungs = a_r_ladder(h_qstep, c, bpv, reinterpret_cast<int32_t(*)[4]>(h_steps));
  return PCC_OK;
}

// a frame's ladder: the steps of its J rungs
struct ARLadder {
  int32_t steps[kARMaxRungs][4];
  int J;
};

// a candidate row on the host: frame fi (of the frames with points) at rung `rung`
struct ARCand {
  int fi, rung;
  int64_t cb, ctx_off;     // its chunks among the call's candidate chunks, its contexts among the call's
  int64_t idx_off, rec_off, work_off;   // in the scratch block, 16-bit words from its start
  int epoch;               // the scratch block's turn that holds them
  int64_t len;             // bytes of the blob it would give
};

// the scratch block of the candidate rows' indices, records and word regions: groups of rows take it in turn; a group
// that does not fit behind the ones before it starts the block over, and what those left is gone
struct ARScratch {
  size_t cap = 0, used = 0;
  int epoch = 0;
};
// what a candidate row of frame r takes of it
static size_t a_r_row_need(const AFrame& r) { return pcc_align((size_t)r.n * r.c * 2) + 2 * pcc_align((size_t)r.nc * kLanes * r.T * 2); }

// rows [r0, r1) of a host vector (`per` elements a row) to their place behind `at` of the staging and on to the same
// place of the device's tables
template <typename T>
static int a_send_rows(hipStream_t st, uint8_t* stage, uint8_t* d_tabs, size_t at, const std::vector<T>& v, size_t r0, size_t r1,
                       size_t per = 1) {
  const size_t off = at + r0 * per * sizeof(T), bytes = (r1 - r0) * per * sizeof(T);
  memcpy(stage + off, v.data() + r0 * per, bytes);
  PCC_HIP(hipMemcpyAsync(d_tabs + off, stage + off, bytes, hipMemcpyHostToDevice, st));
  return PCC_OK;
}

// one call under a byte target: what its stages share
struct ARCall {
  const char* who;
  pcc_ctx* ctx;
  hipStream_t st;
  const AEncKind* kind;
  const AEncPlan* pl;            // the frames with points: their rows (the places of a candidate row among the coder's
                                 // arrays are its own, a_r_code_rows), order rows, steps and colour
  std::vector<ARLadder> lad;     // their ladders
  int64_t rows_max = 0, chunks_max = 0, ctxs_max = 0;   // candidate rows the call may code, their chunks and contexts
  size_t row_need_max = 0, need_all = 0;                // scratch of the largest row, of all rows at once
  ARScratch scr;
  // the device's tables: the frames' rows | steps and colour | order rows || per candidate row an AFrame and an ARRow ||
  // the winners' rows, their steps and colour, their picks.  The staging: the tables on their way to the device | the
  // blobs | their lengths | the sublevels' bins | the chunks' words
  uint8_t *d_tabs = nullptr, *stage = nullptr;
  size_t aux_at = 0, ord_at = 0, base_end = 0, crow_at = 0, qrow_at = 0, wrow_at = 0, waux_at = 0, pick_at = 0, tab_b = 0, tcnt_at = 0;
  long long* len_dev = nullptr;
  const uint32_t* h_words = nullptr;
  // the arena
  uint16_t *merged = nullptr, *p0 = nullptr, *scratch = nullptr;
  int32_t* hh = nullptr;
  uint2* wts = nullptr;
  uint32_t* cnt = nullptr;
  ASmall small, wsmall;          // of the candidate rows' chunks, of the winners'
  size_t lds = 0;                // k_a_enc's
  // the candidate rows, in the order they were coded
  std::vector<ARCand> cand;
  std::vector<AFrame> crow;      // cand[i]'s row of the coder's table
  std::vector<ARRow> qrow;       // and of the quantiser's
  int64_t chunks_used = 0, ctxs_used = 0;
  // the winners' rows of the pack tables
  std::vector<AFrame> wrow;
  std::vector<ARPick> picks;
  std::vector<int32_t> waux;
  std::vector<int> win_row_of;   // the frame (with points) behind every one of them
  int64_t wchunks = 0;
};

// tables, arena and staging of the call; the frames' tables lie in the staging, ready to go
static int a_r_setup(ARCall& c, int64_t scratch_limit) {
  const AEncPlan& pl = *c.pl;
  const int nf = pl.nf();
  c.scr.cap = std::max(c.row_need_max, std::min(c.need_all, (size_t)(scratch_limit ? scratch_limit : kARScratchDefault)));
  ATables lay;
  lay.add((size_t)nf * sizeof(AFrame));
  c.aux_at = lay.add((size_t)nf * 20), c.ord_at = lay.add((size_t)nf * sizeof(A2Order));
  c.base_end = lay.end;
  c.crow_at = lay.add((size_t)c.rows_max * sizeof(AFrame)), c.qrow_at = lay.add((size_t)c.rows_max * sizeof(ARRow));
  c.wrow_at = lay.add((size_t)nf * sizeof(AFrame)), c.waux_at = lay.add((size_t)nf * 20);
  c.pick_at = lay.add((size_t)nf * sizeof(ARPick)), c.tab_b = lay.bytes;
  int64_t win_chunks = 0;
  for (const AFrame& r : pl.tab) win_chunks += r.nc;
  const size_t merged_b = merged_b_of(pl.vals), hh_b = pcc_align((size_t)pl.vals * 4), wts_b = pcc_align((size_t)pl.u * 8);
  const size_t cnt_b = pcc_align((size_t)c.ctxs_max * 8), p0_b = pcc_align((size_t)c.ctxs_max * 2);
  PCC_TRY(pcc_arena_reserve(c.ctx, c.tab_b + merged_b + hh_b + wts_b + cnt_b + p0_b + ASmall::bytes(c.chunks_max) + ASmall::bytes(win_chunks) +
                                       a_t_order_bytes(pl.u, pl.merge_blocks, nf) + c.scr.cap + 8192));
  c.d_tabs = (uint8_t*)pcc_arena_alloc(c.ctx, c.tab_b);
  c.merged = (uint16_t*)pcc_arena_alloc(c.ctx, merged_b);
  c.hh = (int32_t*)pcc_arena_alloc(c.ctx, hh_b);
  c.wts = (uint2*)pcc_arena_alloc(c.ctx, wts_b);
  c.cnt = (uint32_t*)pcc_arena_alloc(c.ctx, cnt_b);
  c.p0 = (uint16_t*)pcc_arena_alloc(c.ctx, p0_b);
  char* small = (char*)pcc_arena_alloc(c.ctx, ASmall::bytes(c.chunks_max));
  char* wsmall = (char*)pcc_arena_alloc(c.ctx, ASmall::bytes(win_chunks));
  c.scratch = (uint16_t*)pcc_arena_alloc(c.ctx, c.scr.cap);
  if (!c.d_tabs || !c.merged || !c.hh || !c.wts || !c.cnt || !c.p0 || !small || !wsmall || !c.scratch) return PCC_E_NOMEM;
  c.small = ASmall(small, c.chunks_max);
  c.wsmall = ASmall(wsmall, win_chunks);
  const size_t lens_at = c.tab_b + (size_t)pl.out_bytes;
  c.tcnt_at = lens_at + (size_t)nf * 8 + 64;
  const size_t hwords_at = c.tcnt_at + pcc_align((size_t)nf * 2 * kATBins * 4);
  PCC_TRY(o2_stage_reserve(c.ctx, hwords_at + (size_t)c.chunks_max * 4 + 64));
  c.stage = (uint8_t*)c.ctx->stage;
  memcpy(c.stage, pl.tab.data(), (size_t)nf * sizeof(AFrame));
  memcpy(c.stage + c.aux_at, pl.aux.data(), (size_t)nf * 20);
  memcpy(c.stage + c.ord_at, pl.order.data(), (size_t)nf * sizeof(A2Order));
  c.len_dev = (long long*)(c.stage + lens_at);
  c.h_words = (const uint32_t*)(c.stage + hwords_at);
  c.lds = 4096 * 4 + (size_t)(pl.nctx_max + 1) * kLanes * 2;
  return PCC_OK;
}

// what does not depend on the step, once for every rung: the tables up, merge, colour transform, the order stage, the
// lift without its quantiser and the mean
static int a_r_lift(ARCall& c, const void* d_values, const uint32_t* d_perm, const uint32_t* d_run_starts, int64_t n_unique,
                    const uint64_t* d_keys) {
  const AEncPlan& pl = *c.pl;
  const int nf = pl.nf();
  hipStream_t st = c.st;
  const AFrame* d_tab = (const AFrame*)c.d_tabs;
  const int32_t* d_aux = (const int32_t*)(c.d_tabs + c.aux_at);
  const A2Order* d_ord = (const A2Order*)(c.d_tabs + c.ord_at);
  PCC_HIP(hipMemcpyAsync(c.d_tabs, c.stage, c.base_end, hipMemcpyHostToDevice, st));
  PCC_HIP(hipMemsetAsync(c.cnt, 0, (size_t)c.ctxs_max * 8, st));
  hipLaunchKernelGGL(k_a_merge, dim3((unsigned)pl.merge_blocks), dim3(256), 0, st, (const uint8_t*)d_values, d_tab, nf, d_perm, d_run_starts,
                     n_unique, pl.n_keys, c.merged);
  PCC_CHECK_LAUNCH();
  if (c.kind->colour) {
    hipLaunchKernelGGL(k_ac_fwd, dim3(nblk(pl.n_max, 256), (unsigned)nf), dim3(256), 0, st, d_tab, d_aux, c.merged);
    PCC_CHECK_LAUNCH();
  }
  ATOrder o;
  PCC_TRY(a_t_order_enc(c.ctx, st, d_keys, d_ord, nf, pl.merge_blocks, pl.u, (uint32_t*)(c.stage + c.tcnt_at), &o));
  for (int t = 0; t < kATBins - 1; ++t) {
    if (!o.grid[t]) continue;
    hipLaunchKernelGGL(k_ar_lift, dim3(o.grid[t], (unsigned)nf), dim3(256), 0, st, d_keys, d_ord, (const uint32_t*)o.bins, (const uint32_t*)o.inv,
                       t, d_tab, c.merged, c.hh, c.wts);
    PCC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_ar_mean, dim3(nblk(4 * (int64_t)nf, 256)), dim3(256), 0, st, d_tab, nf, (const uint16_t*)c.merged, c.hh);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// lays out the rows `want` (frame, rung) in groups that fit the scratch block, appends them to cand, sends their table
// rows and codes them group by group: k_ar_quant, k_a_stats, k_a_enc
static int a_r_code_rows(ARCall& c, const std::vector<std::pair<int, int>>& want) {
  const std::vector<AFrame>& tab = c.pl->tab;
  ARScratch& scr = c.scr;
  const size_t first = c.cand.size();
  PCC_REQUIRE(first + want.size() <= (size_t)c.rows_max, PCC_E_NOMEM, "%s: %zu candidate rows, room for %lld", c.who, first + want.size(),
              (long long)c.rows_max);
  struct Group {
    size_t r0, r1, base;   // rows, where the group starts in the scratch block (bytes)
    int64_t rec_words, quant_blocks, stats_blocks, chunks, cb;
  };
  std::vector<Group> groups;
  for (size_t w = 0; w < want.size();) {
    size_t w1 = w, bytes = 0;
    while (w1 < want.size() && scr.used + bytes + a_r_row_need(tab[(size_t)want[w1].first]) <= scr.cap)
      bytes += a_r_row_need(tab[(size_t)want[w1++].first]);
    if (w1 == w) {   // the block starts over: one row always fits
      scr.used = 0;
      ++scr.epoch;
      continue;
    }
    Group g{first + w, first + w1, scr.used, 0, 0, 0, 0, c.chunks_used};
    size_t idx_b = 0;
    for (size_t i = w; i < w1; ++i) {
      const AFrame& b = tab[(size_t)want[i].first];
      idx_b += pcc_align((size_t)b.n * b.c * 2);
      g.rec_words += (int64_t)(pcc_align((size_t)b.nc * kLanes * b.T * 2) / 2);
    }
    size_t idx_at = g.base / 2, rec_at = (g.base + idx_b) / 2;   // 16-bit words from the block's start
    for (size_t i = w; i < w1; ++i) {
      const int fi = want[i].first, rung = want[i].second;
      const AFrame& b = tab[(size_t)fi];
      ARCand cd{fi, rung, c.chunks_used, c.ctxs_used, (int64_t)idx_at, (int64_t)rec_at, (int64_t)rec_at + g.rec_words, scr.epoch, 0};
      AFrame r = b;
      r.val_off = cd.idx_off;
      r.rec_off = cd.rec_off;
      r.ctx_off = (int32_t)cd.ctx_off;
      r.cb = (int32_t)g.chunks;
      r.sb = (int32_t)g.stats_blocks;
      ARRow q{b.val_off, c.pl->order[(size_t)fi].pt0, cd.idx_off, b.n * b.c, (int32_t)g.quant_blocks, b.c, b.bpv, 0, {0, 0, 0, 0}};
      for (int ch = 0; ch < 4; ++ch) q.q[ch] = c.lad[(size_t)fi].steps[rung][ch];
      c.cand.push_back(cd);
      c.crow.push_back(r);
      c.qrow.push_back(q);
      g.chunks += b.nc;
      g.stats_blocks += b.sn;
      g.quant_blocks += nblk(b.n * b.c, 256);
      c.chunks_used += b.nc;
      c.ctxs_used += b.nctx;
      idx_at += pcc_align((size_t)b.n * b.c * 2) / 2;
      rec_at += pcc_align((size_t)b.nc * kLanes * b.T * 2) / 2;
    }
    scr.used += bytes;
    groups.push_back(g);
    w = w1;
  }
  PCC_TRY(a_send_rows(c.st, c.stage, c.d_tabs, c.crow_at, c.crow, first, c.crow.size()));
  PCC_TRY(a_send_rows(c.st, c.stage, c.d_tabs, c.qrow_at, c.qrow, first, c.qrow.size()));
  const AFrame* d_crow = (const AFrame*)(c.d_tabs + c.crow_at);
  const ARRow* d_qrow = (const ARRow*)(c.d_tabs + c.qrow_at);
  for (const Group& g : groups) {
    const int n_r = (int)(g.r1 - g.r0);
    const ASmall sm = c.small.from(g.cb);
    hipLaunchKernelGGL(k_ar_quant, dim3((unsigned)g.quant_blocks), dim3(256), 0, c.st, d_qrow + g.r0, n_r, (const int32_t*)c.hh,
                       (const uint2*)c.wts, c.scratch);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_a_stats<false>, dim3((unsigned)g.stats_blocks), dim3(256), 0, c.st, (const uint16_t*)c.scratch, d_crow + g.r0, n_r,
                       c.cnt);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_a_enc<false>, dim3((unsigned)g.chunks), dim3(64), c.lds, c.st, (const uint16_t*)c.scratch, d_crow + g.r0, n_r,
                       (const uint32_t*)c.cnt, c.scratch, c.scratch + g.rec_words, sm.states, sm.lens, sm.words, c.p0);
    PCC_CHECK_LAUNCH();
  }
  return PCC_OK;
}

// the lengths of the rows cand[first ..): one read-back of their chunks' words, one synchronisation
static int a_r_read_lens(ARCall& c, size_t first) {
  if (first == c.cand.size()) return PCC_OK;
  const int64_t c0 = c.cand[first].cb;
  PCC_HIP(hipMemcpyAsync((void*)(c.h_words + c0), c.small.words + c0, (size_t)(c.chunks_used - c0) * 4, hipMemcpyDeviceToHost, c.st));
  PCC_HIP(hipStreamSynchronize(c.st));
  for (size_t i = first; i < c.cand.size(); ++i) {
    const AFrame& b = c.pl->tab[(size_t)c.cand[i].fi];
    int64_t w = 0;
    for (int64_t k = 0; k < b.nc; ++k) w += ((volatile const uint32_t*)c.h_words)[c.cand[i].cb + k];
    c.cand[i].len = a_head_bytes(*c.kind, b.c, b.nctx, b.nc) + 2 * w;
  }
  return PCC_OK;
}

// host only, stage 1 of the search (tests/attr_rate_ref.py): a frame's rows cand[a0, a1) at the rungs of A, rising, under
// the target B.  The row that wins; or -1 and *fall, the first row that fits, which wins unless stage 2 finds a rung that
// fits among those between the rung of the row in front of it and its own
static int64_t a_r_stage1(const std::vector<ARCand>& cand, size_t a0, size_t a1, int64_t B, int64_t* fall) {
  size_t a = a0;
  while (a < a1 && cand[a].len > B) ++a;
  if (a == a1) return (int64_t)a - 1;   // nothing fits: rung J - 1, over its target
  if (a == a0 || cand[a].rung - cand[a - 1].rung == 1) return (int64_t)a;
  *fall = (int64_t)a;
  return -1;
}

// the two-stage search: win[i] = the row of cand that frame i (with points) gets
static int a_r_search(ARCall& c, const int64_t* h_target, std::vector<int64_t>* win_out) {
  const int nf = c.pl->nf();
  const std::vector<int>& frame_of = c.pl->frame_of;
  PCC_HIP(hipFuncSetAttribute((const void*)k_a_enc<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
  // stage 1: the rungs of A = { j : j % 4 == 0 } and J - 1
  std::vector<std::pair<int, int>> want;
  std::vector<size_t> s1_at((size_t)nf + 1);
  for (int i = 0; i < nf; ++i) {
    s1_at[(size_t)i] = want.size();
    const int J = c.lad[(size_t)i].J;
    for (int j = 0; j < J; j += 4) want.emplace_back(i, j);
    if ((J - 1) % 4) want.emplace_back(i, J - 1);
  }
  s1_at[(size_t)nf] = want.size();
  PCC_TRY(a_r_code_rows(c, want));
  PCC_TRY(a_r_read_lens(c, 0));
  // stage 2 codes the rungs inside (a', a) of the frames that stage 1 leaves open; the first of them that fits wins
  std::vector<int64_t>& win = *win_out;
  std::vector<int64_t> s2_fall((size_t)nf, -1);
  win.assign((size_t)nf, -1);
  want.clear();
  for (int i = 0; i < nf; ++i) {
    int64_t& a = s2_fall[(size_t)i];
    win[(size_t)i] = a_r_stage1(c.cand, s1_at[(size_t)i], s1_at[(size_t)i + 1], h_target[frame_of[(size_t)i]], &a);
    if (win[(size_t)i] >= 0) continue;
    for (int j = c.cand[(size_t)a - 1].rung + 1; j < c.cand[(size_t)a].rung; ++j) want.emplace_back(i, j);
  }
  if (want.empty()) return PCC_OK;
  const size_t s2 = c.cand.size();
  PCC_TRY(a_r_code_rows(c, want));
  PCC_TRY(a_r_read_lens(c, s2));
  for (size_t r = s2; r < c.cand.size(); ++r) {
    const int i = c.cand[r].fi;
    if (win[(size_t)i] < 0 && c.cand[r].len <= h_target[frame_of[(size_t)i]]) win[(size_t)i] = (int64_t)r;
  }
  for (int i = 0; i < nf; ++i)
    if (win[(size_t)i] < 0) win[(size_t)i] = s2_fall[(size_t)i];
  return PCC_OK;
}

// one batch of winners: frames[k] (with points) at its row rows[k] of cand, whose word regions the scratch block holds.
// Their rows of the pack tables, sent; k_ar_gather and k_a_pack over them; rung_of[the call's frame] = the rung
static int a_r_pack_batch(ARCall& c, const std::vector<int>& frames, const std::vector<int64_t>& rows, int key_shift, std::vector<int>* rung_of) {
  const size_t r0 = c.wrow.size();
  const int n_r = (int)frames.size();
  const int64_t cb = c.wchunks;   // the batch's chunks in the winners' small arrays
  int64_t chunks = 0, nc_max = 0;
  for (size_t k = 0; k < frames.size(); ++k) {
    const ARCand& cd = c.cand[(size_t)rows[k]];
    const int32_t* steps = c.lad[(size_t)cd.fi].steps[cd.rung];
    AFrame r = c.pl->tab[(size_t)frames[k]];
    r.e = c.kind->tc ? c.kind->e : steps[0];
    r.rec_off = cd.work_off;
    r.ctx_off = (int32_t)cd.ctx_off;
    r.cb = (int32_t)chunks;
    c.picks.push_back(ARPick{(int32_t)cd.cb, (int32_t)(cb + chunks), r.nc, 0});
    for (int ch = 0; ch < 4; ++ch) c.waux.push_back(steps[ch]);
    c.waux.push_back(c.kind->colour);
    c.wrow.push_back(r);
    chunks += r.nc;
    nc_max = std::max<int64_t>(nc_max, r.nc);
    (*rung_of)[(size_t)c.pl->frame_of[(size_t)frames[k]]] = cd.rung;
  }
  c.wchunks += chunks;
  c.win_row_of.insert(c.win_row_of.end(), frames.begin(), frames.end());
  PCC_TRY(a_send_rows(c.st, c.stage, c.d_tabs, c.wrow_at, c.wrow, r0, c.wrow.size()));
  PCC_TRY(a_send_rows(c.st, c.stage, c.d_tabs, c.waux_at, c.waux, r0, c.wrow.size(), 5));
  PCC_TRY(a_send_rows(c.st, c.stage, c.d_tabs, c.pick_at, c.picks, r0, c.picks.size()));
  hipLaunchKernelGGL(k_ar_gather, dim3(nblk(nc_max * 2 * kLanes, 256), (unsigned)n_r), dim3(256), 0, c.st,
                     (const ARPick*)(c.d_tabs + c.pick_at) + r0, (const uint32_t*)c.small.words, (const uint16_t*)c.small.states,
                     (const uint16_t*)c.small.lens, c.wsmall.words, c.wsmall.states, c.wsmall.lens);
  PCC_CHECK_LAUNCH();
  return a_launch_pack<false, true, false, true>(c.st, (unsigned)(chunks + n_r), c.scratch, (const AFrame*)(c.d_tabs + c.wrow_at) + r0, n_r,
                                                 c.wsmall.from(cb), c.p0, c.stage + c.tab_b, c.len_dev + r0, nullptr, key_shift / 3, nullptr,
                                                 c.kind->tc ? (const int32_t*)(c.d_tabs + c.waux_at) + 5 * r0 : nullptr, 0);
}

// the winners to blobs: those whose word regions the scratch block still holds in one batch; the others coded once
// more, as many at a time as one turn of the block holds, every batch packed before the next one may take the block
static int a_r_pack_winners(ARCall& c, const std::vector<int64_t>& win, int key_shift, std::vector<int>* rung_of) {
  const std::vector<AFrame>& tab = c.pl->tab;
  std::vector<int> held, lost;
  for (int i = 0; i < c.pl->nf(); ++i) (c.cand[(size_t)win[(size_t)i]].epoch == c.scr.epoch ? held : lost).push_back(i);
  if (!held.empty()) {
    std::vector<int64_t> rows;
    for (int i : held) rows.push_back(win[(size_t)i]);
    PCC_TRY(a_r_pack_batch(c, held, rows, key_shift, rung_of));
  }
  std::vector<std::pair<int, int>> want;
  for (size_t k = 0; k < lost.size();) {
    size_t k1 = k, bytes = 0;
    while (k1 < lost.size() && bytes + a_r_row_need(tab[(size_t)lost[k1]]) <= c.scr.cap) bytes += a_r_row_need(tab[(size_t)lost[k1++]]);
    c.scr.used = c.scr.cap;   // this group starts the block over
    want.clear();
    const std::vector<int> frames(lost.begin() + (long)k, lost.begin() + (long)k1);
    for (int i : frames) want.emplace_back(i, c.cand[(size_t)win[(size_t)i]].rung);
    const size_t first = c.cand.size();
    PCC_TRY(a_r_code_rows(c, want));
    std::vector<int64_t> rows;
    for (size_t r = first; r < c.cand.size(); ++r) rows.push_back((int64_t)r);
    PCC_TRY(a_r_pack_batch(c, frames, rows, key_shift, rung_of));
    k = k1;
  }
  return PCC_OK;
}

extern "C" int pcc_attr_encode_frames_rate(pcc_ctx* ctx, const void* d_values, const int64_t* h_value_offsets, const int32_t* h_format,
                                           const int64_t* h_rows, const int64_t* h_points, int n_frames, const uint32_t* d_perm,
                                           const uint32_t* d_run_starts, int64_t n_unique, int64_t n_kept, const uint64_t* d_keys,
                                           int key_shift, const int32_t h_qstep[4], int per_channel, int colour,
                                           const int64_t* h_target, int64_t scratch_limit, uint8_t* h_out, int64_t cap,
                                           int64_t* h_offsets, int32_t* h_rung) {
  const char* who = "pcc_attr_encode_frames_rate";
  PCC_REQUIRE(n_kept >= -1 && h_qstep && h_target && (colour == 0 || colour == 1) && (per_channel == 0 || per_channel == 1) &&
                  (per_channel || (!colour && h_qstep[0] >= 1)) && scratch_limit >= 0,
              PCC_E_ARG, "%s: bad argument (n_kept=%lld per_channel=%d colour=%d scratch_limit=%lld)", who, (long long)n_kept, per_channel,
              colour, (long long)scratch_limit);
  const AEncKind kind = a_kind_transform(n_kept, h_qstep[0], per_channel ? h_qstep : nullptr, colour);
  AEncPlan pl;
  ARCall c;
  c.who = who, c.ctx = ctx, c.kind = &kind, c.pl = &pl;
  // per frame its target, checked; per frame with points its ladder and what its candidate rows may take
  PCC_TRY(a_enc_front(who, kind, ctx, d_values, h_value_offsets, h_format, h_rows, h_points, n_frames, d_perm, d_run_starts, n_unique, d_keys,
                      key_shift, h_out, cap, h_offsets, &pl, [&](int f, AFrame* r) -> int {
                        PCC_REQUIRE(h_target[f] >= 1, PCC_E_ARG, "%s: frame %d: a target of %lld bytes (at least 1)", who, f,
                                    (long long)h_target[f]);
                        if (!r) return PCC_OK;
                        c.lad.emplace_back();
                        c.lad.back().J = a_r_ladder(&pl.aux[pl.aux.size() - 5], r->c, r->bpv, c.lad.back().steps);
                        const int64_t rows_f = (c.lad.back().J + 3) / 4 + 1 + 3 + 1;   // stage 1 | stage 2 | once more at the end
                        c.rows_max += rows_f;
                        c.chunks_max += rows_f * r->nc;
                        c.ctxs_max += rows_f * r->nctx;
                        c.row_need_max = std::max(c.row_need_max, a_r_row_need(*r));
                        c.need_all += (size_t)(rows_f - 1) * a_r_row_need(*r);
                        return PCC_OK;
                      }));
  const int nf = pl.nf();
  AEncOut out(n_frames);
  std::vector<int> rung_of((size_t)n_frames, -1);
  if (nf > 0) {
    c.st = ctx->stream;
    PCC_TRY(a_r_setup(c, scratch_limit));
    PccProfScope prof(ctx, "attr_encode_rate", pl.u, nf, c.rows_max, 0);
    PCC_TRY(a_r_lift(c, d_values, d_perm, d_run_starts, n_unique, d_keys));
    std::vector<int64_t> win;
    PCC_TRY(a_r_search(c, h_target, &win));
    PCC_TRY(a_r_pack_winners(c, win, key_shift, &rung_of));
    PCC_HIP(hipStreamSynchronize(c.st));
    for (size_t r = 0; r < c.win_row_of.size(); ++r)
      PCC_TRY(out.take(who, pl, c.win_row_of[r], ((volatile long long*)c.len_dev)[r], c.tab_b));
  }
  PCC_TRY(a_enc_emit(who, kind, ctx, h_format, n_frames, key_shift, out, h_out, cap, h_offsets));
  for (int f = 0; h_rung && f < n_frames; ++f) h_rung[f] = rung_of[(size_t)f];
  return PCC_OK;
}

// a parser's error, named by the entry point
static int a_wrap_error(const char* who, int rc) {
  const std::string m = pcc_last_error();
  pcc_set_error("%s: %s", who, m.c_str());
  return rc;
}

// host only: the version byte and byte 3 of a head, checked: its kind, channels and mask
static int a_head_kind(const char* who, const uint8_t* h_in, int64_t len, bool* scal, bool* nl, bool* xc, int* c, int* m) {
  PCC_REQUIRE(h_in && len >= kAttrHead && h_in[0] == 'A', PCC_E_STREAM, "%s: not an attribute blob (len=%lld)", who, (long long)len);
  bool nbr;   // versions 25 / 26 stand beside 2 / 11 here (scalable, lossless, 26 with a mask), 28 / 31 beside 7 / 14
  PCC_REQUIRE(attr_kind12(h_in[1], scal, nl, xc, &nbr), PCC_E_STREAM, "%s: attribute blob version %d", who, (int)h_in[1]);
  const int bpv = *scal ? h_in[2] & 15 : h_in[2];
  PCC_REQUIRE((bpv == 1 || bpv == 2) && attr_channels(h_in[3], *xc, c, m), PCC_E_STREAM, "%s: %d bytes per value, %d channels%s", who,
              bpv, *c, *xc ? ", or their mask" : "");
  return PCC_OK;
}

// host only: the cross-channel mask of a head, 0 for the plain kinds
extern "C" int pcc_attr_cross_mask(const uint8_t* h_in, int64_t len, int32_t* h_mask) {
  bool scal, nl, xc;
  int c, m;
  PCC_TRY(a_head_kind("pcc_attr_cross_mask", h_in, len, &scal, &nl, &xc, &c, &m));
  if (h_mask) *h_mask = m;
  return PCC_OK;
}

// host only: q of a version-19 head, 0 for every other kind and for a blob without points
extern "C" int pcc_attr_qstep(const uint8_t* h_in, int64_t len, int32_t* h_qstep) {
  int32_t ver = 0;
  PCC_TRY(pcc_attr_info(h_in, len, &ver, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  int32_t q = 0;
  if (attr_t_kind(ver)) {
    AttrTInfo o;
    PCC_TRY(attr_t_parse(h_in, len, &o, true));
    q = (int32_t)o.qstep;
  }
  if (h_qstep) *h_qstep = q;
  return PCC_OK;
}

// host only: the colour word and the steps of a version-21 head (h_in may be a prefix that reaches q[c - 1]), 0s for
// every other kind and for a blob without points
extern "C" int pcc_attr_transform_info(const uint8_t* h_in, int64_t len, int32_t* h_colour, int32_t h_qstep[4]) {
  int32_t ver = 0;
  PCC_TRY(pcc_attr_info(h_in, len, &ver, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  AttrCInfo o;
  o.colour = 0;
  for (int ch = 0; ch < 4; ++ch) o.q[ch] = 0;
  if (attr_c_kind(ver)) PCC_TRY(attr_c_parse(h_in, len, &o, true));
  if (attr_s_kind(ver)) {   // version 22 keeps them where version 21 does
    AttrSInfo s;
    PCC_TRY(attr_s_parse(h_in, len, 0, kAttrSHead, &s, nullptr));
    o.colour = s.colour;
    for (int ch = 0; ch < 4; ++ch) o.q[ch] = s.q[ch];
  }
  if (h_colour) *h_colour = (int32_t)o.colour;
  for (int ch = 0; h_qstep && ch < 4; ++ch) h_qstep[ch] = (int32_t)o.q[ch];
  return PCC_OK;
}

// host only: K of a version-22 head (h_in may be a prefix that reaches K: 20 + 4 c bytes), 0 for every other kind and
// for a blob without points
extern "C" int pcc_attr_scalable_to(const uint8_t* h_in, int64_t len, int32_t* h_scalable_to) {
  int32_t ver = 0;
  PCC_TRY(pcc_attr_info(h_in, len, &ver, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  AttrSInfo s;
  s.K = 0;
  if (attr_s_kind(ver)) PCC_TRY(attr_s_parse(h_in, len, 0, kAttrSHead, &s, nullptr));
  if (h_scalable_to) *h_scalable_to = s.K;
  return PCC_OK;
}

// host only: what the head of an attribute blob of any kind says (h_in may be a prefix that holds the head)
extern "C" int pcc_attr_info(const uint8_t* h_in, int64_t len, int32_t* h_version, int32_t* h_bpv, int32_t* h_channels,
                             int64_t* h_points, int32_t* h_max_error, int32_t* h_scalable, int32_t* h_lod) {
  bool scal = false, nl, xc;
  int ver, bpv, c, m, slod;
  int64_t n;
  uint32_t e = 0;
  if (h_in && len >= kAttrHead && h_in[0] == 'A' && attr_s_kind(h_in[1])) {
    // version 22: its own parser; K through pcc_attr_scalable_to, steps and colour through pcc_attr_transform_info
    AttrSInfo o;
    const int rc = attr_s_parse(h_in, len, 0, kAttrSHead, &o, nullptr);
    if (rc != PCC_OK) return a_wrap_error("pcc_attr_info", rc);
    ver = o.version, bpv = o.bpv, c = o.c, n = o.n, slod = o.slod, scal = true;
  } else if (h_in && len >= kAttrHead && h_in[0] == 'A' && (attr_t_kind(h_in[1]) || attr_c_kind(h_in[1]))) {
    // versions 19 and 21: their own parser; q through pcc_attr_qstep, steps and colour through pcc_attr_transform_info
    AttrCInfo o;
    const int rc = attr_tc_parse(h_in, len, &o, attr_c_kind(h_in[1]) ? &o : nullptr, true);
    if (rc != PCC_OK) return a_wrap_error("pcc_attr_info", rc);
    ver = o.version, bpv = o.bpv, c = o.c, n = o.n, slod = o.slod;
  } else {
    PCC_TRY(a_head_kind("pcc_attr_info", h_in, len, &scal, &nl, &xc, &c, &m));
    ver = h_in[1], bpv = scal ? h_in[2] & 15 : h_in[2], slod = scal ? h_in[2] >> 4 : 0;
    n = (int64_t)attr_u32(h_in + 4);
    PCC_REQUIRE(n < ((int64_t)1 << 27), PCC_E_STREAM, "pcc_attr_info: %lld points", (long long)n);
    if (nl && n > 0) {
      PCC_REQUIRE(len >= kAttrHead + 4, PCC_E_STREAM, "pcc_attr_info: truncated in front of max_error (len=%lld)", (long long)len);
      e = attr_u32(h_in + kAttrHead);
      PCC_REQUIRE(e >= 1 && e <= attr_max_error(bpv), PCC_E_STREAM, "pcc_attr_info: max_error %u with %d bytes per value", e, bpv);
    }
  }
  if (h_version) *h_version = ver;
  if (h_bpv) *h_bpv = bpv;
  if (h_channels) *h_channels = c;
  if (h_points) *h_points = n;
  if (h_max_error) *h_max_error = (int32_t)e;
  if (h_scalable) *h_scalable = scal ? 1 : 0;
  if (h_lod) *h_lod = slod;
  return PCC_OK;
}

// ---- what the three decoders share -----------------------------------------------------------------------------------
static bool a_is_version(const uint8_t* b, int64_t len, int version) { return b && len >= 2 && b[0] == 'A' && b[1] == version; }

// the version of a call's blobs: the first blob's when it is one of the entry point's kinds, else the first of them
template <int N>
static int a_call_version(const uint8_t* b, int64_t len, const int (&kinds)[N]) {
  for (int k : kinds)
    if (a_is_version(b, len, k)) return k;
  return kinds[0];
}

// the blobs of a call are of one version, `mine`: the entry point's other versions are refused by name
template <int N>
static int a_mixed_version(const char* who, int f, const uint8_t* b, int64_t len, const int (&kinds)[N], int mine) {
  for (int other : kinds)
    PCC_REQUIRE(other == mine || !a_is_version(b, len, other), PCC_E_ARG,
                "%s: frame %d: attribute blob version %d in a call of version %d blobs (one version per call)", who, f, other, mine);
  return PCC_OK;
}

// the parser's error, named by entry point and frame
static int a_wrap_error(const char* who, int f, int rc) {
  const std::string m = pcc_last_error();
  pcc_set_error("%s: frame %d: %s", who, f, m.c_str());
  return rc;
}

// a caller's array in pinned host memory receives the values straight from the device; any other one through the
// staging (a failed query of an ordinary pointer leaves its error behind: cleared here)
static bool a_host_is_pinned(const void* h_out) {
  hipPointerAttribute_t attr;
  if (!h_out) return false;
  if (hipPointerGetAttributes(&attr, h_out) == hipSuccess) return attr.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  return false;
}

// k_a_dec's dynamic LDS: a chunk's payload beside the models when it fits in 128 KB in all, else read where it lies
static size_t a_dec_lds(int64_t nctx_max, int64_t cw_max, int* model_rows, int* lds_words) {
  *model_rows = (int)nctx_max + 1;
  const int64_t room = ((int64_t)128 * 1024 - (int64_t)*model_rows * kLanes * 2) / 2;
  *lds_words = (int)std::max<int64_t>(0, std::min<int64_t>(cw_max, room));
  return (size_t)*model_rows * kLanes * 2 + (size_t)*lds_words * 2;
}

// One decode call, the skeleton of pcc_attr_decode_frames, pcc_attr_decode_frames_lod and the transform decoder.  An
// entry point parses and checks frame by frame and hands every frame to a_dec_count; builds its side tables; then
// a_dec_plan (rows, layout, arena), its own arena arrays, a_dec_send (staging, upload), its kernels, a_dec_finish
// (values and status back behind the call's last synchronisation, the status of every frame, the copy out).
struct ADecIn {             // a frame as its parser left it
  const AttrInfo* o;        // the parsed head; the entry point keeps it
  int64_t n_dec;            // values to decode: the frame's points, or its cells at a level of detail
  int64_t nc, last_words;   // the chunks that takes, and the words of the last of them that are there to read
  int64_t body_b;           // the bytes of the blob from off_p0 on that go to the device
  uint32_t e;               // the row's max_error: e of the near-lossless kinds, q of version 19
  int shift;                // decoders against cells: the level of the frame's cells, the sender's and the call's
};
struct ADecCall {
  const char* who;
  pcc_ctx* ctx;
  const uint8_t* const* h_blobs;
  int n_frames;
  uint8_t *d_out, *h_out;
  int64_t cap_bytes;
  int64_t* h_out_offsets;
  int32_t* h_format;
  std::vector<ADecIn> in;
  int nf = 0;                                                // frames with values: the rows of every table
  int64_t bytes = 0, bodies = 0, points = 0;                 // the accounting pass
  const int32_t* masks = nullptr;                            // side tables, one entry per row (nullptr: not in this call):
  const A2Order* order = nullptr;                            //   cross-channel masks | order rows | steps and colour word
  const int32_t* aux = nullptr;
  std::vector<ADFrame> tab;                                  // the rows pass
  int64_t chunks = 0, nctx_max = 0, cw_max = 0, n_max = 0;
  ATables lay;                                               // the upload: rows, masks directly behind | order | aux | bodies
  size_t ord_at = 0, aux_at = 0;
  uint8_t *d_in = nullptr, *out = nullptr;                   // the upload in the arena; the values in HBM
  uint8_t *down = nullptr, *back = nullptr;                  // staging: where the values come down to; what is read back
  size_t masks_at() const { return (size_t)nf * sizeof(ADFrame); }
};

static ADecCall a_dec_call(const char* who, pcc_ctx* ctx, const uint8_t* const* h_blobs, int n_frames, uint8_t* d_out, uint8_t* h_out,
                           int64_t cap_bytes, int64_t* h_out_offsets, int32_t* h_format) {
  h_out_offsets[0] = 0;
  return ADecCall{who, ctx, h_blobs, n_frames, d_out, h_out, cap_bytes, h_out_offsets, h_format, std::vector<ADecIn>((size_t)n_frames)};
}

// accounting, frame f, once it has passed its entry point's checks: format and offsets out, every frame's values on 16 bytes
static void a_dec_count(ADecCall& d, int f, const ADecIn& in) {
  const AttrInfo& o = *in.o;
  d.in[(size_t)f] = in;
  if (d.h_format) d.h_format[f] = o.bpv | (o.c << 8);
  d.bytes = a_round(d.bytes + in.n_dec * o.c * o.bpv, 16);
  d.points += in.n_dec;
  d.h_out_offsets[f + 1] = d.bytes;
  if (in.n_dec) {
    d.bodies += a_round(in.body_b, 16);
    ++d.nf;
  }
}

// behind the parse loop.  *idle: nothing to decode, or nowhere to put it (a call that asks for sizes)
static int a_dec_counted(const ADecCall& d, const char* noun, bool* idle) {
  PCC_REQUIRE(d.points < ((int64_t)1 << 31), PCC_E_ARG, "%s: the blobs announce %lld %s in all", d.who, (long long)d.points, noun);
  *idle = d.bytes == 0 || (!d.d_out && !d.h_out);
  return PCC_OK;
}

// decoders against the cells of the geometry (levels of detail, the transform kinds): the cells are needed; one order
// row per frame with values, its cells [at, at + n_dec) of the call's, its blocks of 256 from *blocks on
static int a_dec_order(const ADecCall& d, const int32_t* d_cells, const int64_t* h_cell_offsets, std::vector<A2Order>* order,
                       int64_t* blocks, int64_t* cells_all, const int32_t** cells) {
  PCC_REQUIRE(d_cells && h_cell_offsets && h_cell_offsets[0] >= 0, PCC_E_ARG, "%s: the cells of the frames are needed", d.who);
  const int64_t cell0 = h_cell_offsets[0];
  *blocks = 0;
  for (int f = 0; f < d.n_frames; ++f) {
    const ADecIn& in = d.in[(size_t)f];
    if (in.n_dec == 0) continue;
    order->push_back(A2Order{h_cell_offsets[f] - cell0, in.n_dec, (int32_t)*blocks, in.shift});
    *blocks += nblk(in.n_dec, 256);
  }
  *cells_all = h_cell_offsets[d.n_frames] - cell0;
  *cells = d_cells + 3 * cell0;
  return PCC_OK;
}

// the row of a frame with points: its body at body_off of the upload, its values at out_off of the output, its chunks
// [cb, cb + nc) of the call's, the last of them with last_words words there to read, n_dec values to decode
static ADFrame a_dec_row(const ADecIn& in, int64_t body_off, int64_t out_off, int64_t cb) {
  const AttrInfo& o = *in.o;
  ADFrame r;
  r.body_off = body_off;
  r.table_off = o.off_table - o.off_p0;
  r.payload_off = o.off_payload - o.off_p0;
  r.n = o.n;
  r.out_off = out_off;
  r.S = (int32_t)o.S;
  r.nc = (int32_t)in.nc;
  r.cb = (int32_t)cb;
  r.c = o.c;
  r.bpv = o.bpv;
  r.nctx = o.nctx;
  r.n_dec = in.n_dec;
  r.last_words = (int32_t)in.last_words;
  r.max_error = (int32_t)in.e;
  return r;
}

// capacity, the rows pass, the layout of the upload, and the arena: own_b bytes for the entry point's arrays besides
// the upload and value_arrays arrays of the call's bytes (the values unless d_out takes them, indices, residuals)
static int a_dec_plan(ADecCall& d, int value_arrays, size_t own_b) {
  PCC_REQUIRE(d.cap_bytes >= d.bytes, PCC_E_NOMEM, "%s: %lld bytes, capacity %lld", d.who, (long long)d.bytes, (long long)d.cap_bytes);
  int64_t body_off = 0;
  for (int f = 0; f < d.n_frames; ++f) {
    const ADecIn& in = d.in[(size_t)f];
    if (in.n_dec == 0) continue;
    const uint8_t* table = d.h_blobs[f] + in.o->off_table;
    d.tab.push_back(a_dec_row(in, body_off, d.h_out_offsets[f], d.chunks));
    for (int64_t k = 0; k + 1 < in.nc; ++k) d.cw_max = std::max<int64_t>(d.cw_max, attr_u32(table + 4 * k));
    d.cw_max = std::max<int64_t>(d.cw_max, in.last_words);
    d.n_max = std::max(d.n_max, in.n_dec);
    body_off += a_round(in.body_b, 16);
    d.chunks += in.nc;
    d.nctx_max = std::max<int64_t>(d.nctx_max, in.o->nctx);
  }
  d.lay.add((size_t)d.nf * (sizeof(ADFrame) + (d.masks ? 4 : 0)));
  d.ord_at = d.lay.add(d.order ? (size_t)d.nf * sizeof(A2Order) : 0);
  d.aux_at = d.lay.add(d.aux ? (size_t)d.nf * 20 : 0);
  PCC_TRY(pcc_arena_reserve(d.ctx, d.lay.bytes + pcc_align((size_t)d.bodies + 16) + (size_t)value_arrays * pcc_align((size_t)d.bytes) + own_b));
  d.d_in = (uint8_t*)pcc_arena_alloc(d.ctx, d.lay.bytes + (size_t)d.bodies + 16);
  d.out = d.d_out ? d.d_out : (uint8_t*)pcc_arena_alloc(d.ctx, (size_t)d.bytes);
  return d.d_in && d.out ? PCC_OK : PCC_E_NOMEM;
}

// staging: rows, side tables and bodies on their way up | the values on their way down, unless they go straight to the
// caller's pinned array | back_b bytes of counts and status read back; then the upload
static int a_dec_send(ADecCall& d, size_t back_b) {
  const size_t in_b = d.lay.bytes + (size_t)d.bodies, nf = (size_t)d.nf;
  const bool direct = a_host_is_pinned(d.h_out);
  const size_t out_b = d.h_out && !direct ? (size_t)d.bytes : 0;
  PCC_TRY(o2_stage_reserve(d.ctx, pcc_align(in_b) + pcc_align(out_b) + back_b + 64));
  uint8_t* stage = (uint8_t*)d.ctx->stage;
  d.down = !d.h_out ? nullptr : (direct ? d.h_out : stage + pcc_align(in_b));
  d.back = stage + pcc_align(in_b) + pcc_align(out_b);
  memcpy(stage, d.tab.data(), nf * sizeof(ADFrame));
  if (d.masks) memcpy(stage + d.masks_at(), d.masks, nf * 4);
  if (d.order) memcpy(stage + d.ord_at, d.order, nf * sizeof(A2Order));
  if (d.aux) memcpy(stage + d.aux_at, d.aux, nf * 20);
  for (int f = 0, k = 0; f < d.n_frames; ++f) {
    const ADecIn& in = d.in[(size_t)f];
    if (in.n_dec == 0) continue;
    memcpy(stage + d.lay.bytes + d.tab[(size_t)k++].body_off, d.h_blobs[f] + in.o->off_p0, (size_t)in.body_b);
  }
  PCC_HIP(hipMemcpyAsync(d.d_in, stage, in_b, hipMemcpyHostToDevice, d.ctx->stream));
  return PCC_OK;
}

// the lane decoder over the call's chunks: values, residuals or indices to dst
template <bool V2>
static int a_launch_dec(const ADecCall& d, uint8_t* dst, int32_t* status) {
  int model_rows, lds_words;
  const size_t lds = a_dec_lds(d.nctx_max, d.cw_max, &model_rows, &lds_words);
  PCC_HIP(hipFuncSetAttribute((const void*)k_a_dec<V2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_a_dec<V2>, dim3((unsigned)d.chunks), dim3(64), lds, d.ctx->stream, d.d_in + d.lay.bytes, (const ADFrame*)d.d_in, d.nf,
                     model_rows, lds_words, dst, status);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// the end of a call: the values down, back_b bytes of back_dev to back_at of what is read back, one synchronisation;
// then per frame with values (row k) the entry point's own check and the frame's status, an int32 per row at status_at
// of what was read back; and the values out of the staging where they came down there
template <typename Check>
static int a_dec_finish(ADecCall& d, const void* back_dev, size_t back_b, size_t back_at, size_t status_at, const char* legend,
                        Check&& frame_check) {
  hipStream_t st = d.ctx->stream;
  if (d.down) PCC_HIP(hipMemcpyAsync(d.down, d.out, (size_t)d.bytes, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipMemcpyAsync(d.back + back_at, back_dev, back_b, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipStreamSynchronize(st));
  const int32_t* h_status = (const int32_t*)(d.back + status_at);
  for (int f = 0, k = 0; f < d.n_frames; ++f) {
    if (d.in[(size_t)f].n_dec == 0) continue;
    PCC_TRY(frame_check(f, k));
    const int32_t bad = h_status[k++];
    PCC_REQUIRE(bad == 0, PCC_E_STREAM, "%s: frame %d: attribute blob: corrupt stream (status %d: 1 = words, 4 = final state%s)", d.who, f, bad,
                legend);
  }
  if (d.down && d.down != d.h_out) memcpy(d.h_out, d.down, (size_t)d.bytes);
  return PCC_OK;
}
static int a_dec_finish(ADecCall& d, const void* back_dev, size_t back_b, size_t back_at, size_t status_at, const char* legend) {
  return a_dec_finish(d, back_dev, back_b, back_at, status_at, legend, [](int, int) { return PCC_OK; });
}

extern "C" int pcc_attr_decode_frames(pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                                      const int64_t* h_points, uint8_t* d_out, uint8_t* h_out, int64_t cap_bytes,
                                      int64_t* h_out_offsets, int32_t* h_format) {
  const char* who = "pcc_attr_decode_frames";
  PCC_REQUIRE(ctx && h_blobs && h_lens && h_out_offsets && n_frames >= 1 && n_frames <= 65535, PCC_E_ARG,
              "%s: bad argument (n_frames=%d)", who, n_frames);
  // the blobs of a call are of one version, the first blob's: 1, or 4 (its indices through the decoder of version 2 at
  // lod 0, then k_a4_recon), or their cross-channel forms 8 and 13 (k_ax_inv behind that decoder, then k_a8_recon /
  // k_a4_recon)
  const int kinds[4] = {1, 4, 8, 13};
  const int mine = a_call_version(h_blobs[0], h_lens[0], kinds);
  const bool nl = mine == 4 || mine == 13, xc = mine == 8 || mine == 13;
  ADecCall d = a_dec_call(who, ctx, h_blobs, n_frames, d_out, h_out, cap_bytes, h_out_offsets, h_format);
  std::vector<AttrInfo> info((size_t)n_frames);
  for (int f = 0; f < n_frames; ++f) {
    AttrInfo& o = info[(size_t)f];
    PCC_TRY(a_mixed_version(who, f, h_blobs[f], h_lens[f], kinds, mine));
    const int rc = attr_parse_kind(h_blobs[f], h_lens[f], nl, &o, xc);
    if (rc != PCC_OK) return a_wrap_error(who, f, rc);
    PCC_REQUIRE(!h_points || h_points[f] == o.n, PCC_E_STREAM, "%s: frame %d: the attribute blob has %lld points, its geometry %lld",
                who, f, (long long)o.n, (long long)(h_points ? h_points[f] : 0));
    const int64_t last_words = o.n ? attr_u32(h_blobs[f] + o.off_table + 4 * (o.nc - 1)) : 0;
    a_dec_count(d, f, ADecIn{&o, o.n, o.nc, last_words, h_lens[f] - o.off_p0, o.max_error, 0});
  }
  bool idle;
  PCC_TRY(a_dec_counted(d, "points", &idle));
  if (idle) return PCC_OK;
  std::vector<int32_t> cross;   // the masks of versions 8 and 13
  int64_t run_threads = 0;
  for (const AttrInfo& o : info) {
    if (o.n == 0) continue;
    cross.push_back(o.cross);
    run_threads = std::max<int64_t>(run_threads, o.nc * kLanes * o.c);
  }
  if (xc) d.masks = cross.data();
  const size_t status_b = (size_t)d.nf * 4 + 64;
  PCC_TRY(a_dec_plan(d, (d_out ? 0 : 1) + (nl ? 1 : 0), pcc_align(status_b) + 4096));
  const int nf = d.nf;
  hipStream_t st = ctx->stream;
  uint8_t* out = d.out;
  uint8_t* idx = nl ? (uint8_t*)pcc_arena_alloc(ctx, (size_t)d.bytes) : out;   // version 4: the indices, as version 2's residuals
  int32_t* status = (int32_t*)pcc_arena_alloc(ctx, status_b);
  if (!idx || !status) return PCC_E_NOMEM;
  PccProfScope prof(ctx, "attr_decode", d.points, nf, d.chunks, 0);
  PCC_TRY(a_dec_send(d, (size_t)nf * 4));
  PCC_HIP(hipMemsetAsync(status, 0, status_b, st));
  const ADFrame* d_tab = (const ADFrame*)d.d_in;
  if (!nl && !xc) {
    PCC_TRY(a_launch_dec<false>(d, out, status));
  } else {
    PCC_TRY(a_launch_dec<true>(d, idx, status));
    if (xc) {
      hipLaunchKernelGGL(k_ax_inv, dim3(nblk(d.n_max, 256), (unsigned)nf), dim3(256), 0, st, d_tab, (const int32_t*)(d.d_in + d.masks_at()), idx);
      PCC_CHECK_LAUNCH();
    }
  }
  if (xc && !nl) {   // version 8: idx is out
    hipLaunchKernelGGL(k_a8_recon, dim3(nblk(run_threads, 256), (unsigned)nf), dim3(256), 0, st, d_tab, out);
    PCC_CHECK_LAUNCH();
  } else if (nl) {
    hipLaunchKernelGGL(k_a4_recon, dim3(nblk(run_threads, 256), (unsigned)nf), dim3(256), 0, st, d_tab, (const uint8_t*)idx, out, status);
    PCC_CHECK_LAUNCH();
  }
  return a_dec_finish(d, status, (size_t)nf * 4, 0, 0, nl ? ", 16 = reconstruction out of range" : "");
}

// ---- versions 19 and 21: the decoder ---------------------------------------------------------------------------------
// Against the cells its geometry decode left in HBM, as version 2's at lod 0: the order stage over the cells' keys, the
// lane decoder (x in coding order), the root, one k_at_lift<false> per occupied sublevel top-down, clamp and store.
// tc: a call of version-21 blobs — their steps and colour words in a table behind the order rows (aux: 5 words per
// frame), the lift with a step per channel, and k_ac_store in place of k_at_store where a frame has the colour transform.
// Version 22, at level of detail lod (0 for the other two): the cells are those of the geometry at lod, biased by
// 32768 >> (slod + lod); the lane decoder reads the level's prefix as version 2's does; k_as_flag and the scan behind
// the order stage, whose counts must be the head's; k_as_lift over the sublevels of the cells' keys (47 - 3 lod .. 0),
// each frame under its own K (the row's max_error); k_ac_store over the cells
static int a_t_decode_frames(const char* who, pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                             const int32_t* d_cells, const int64_t* h_cell_offsets, uint8_t* d_out, uint8_t* h_out, int64_t cap_bytes,
                             int64_t* h_out_offsets, int32_t* h_format, int version, int lod) {
  const bool sc = attr_s_kind(version), tc = sc || attr_c_kind(version);
  ADecCall d = a_dec_call(who, ctx, h_blobs, n_frames, d_out, h_out, cap_bytes, h_out_offsets, h_format);
  std::vector<AttrSInfo> info((size_t)n_frames);
  for (int f = 0; f < n_frames; ++f) {
    AttrSInfo& o = info[(size_t)f];
    if (sc) {
      Attr2Plan pl;
      const int rc = attr_s_parse(h_blobs[f], h_lens[f], lod, kAttrSDecode, &o, &pl);
      if (rc != PCC_OK) return a_wrap_error(who, f, rc);
      if (h_cell_offsets) {
        const int64_t m = h_cell_offsets[f + 1] - h_cell_offsets[f];
        PCC_REQUIRE(m == pl.m, PCC_E_STREAM, "%s: frame %d: the attribute blob has %lld values at level of detail %d, its geometry %lld cells",
                    who, f, (long long)pl.m, lod, (long long)m);
      }
      a_dec_count(d, f, ADecIn{&o, pl.m, pl.chunks, pl.last_words, pl.bytes - o.off_p0, (uint32_t)o.K, lod + o.slod});   // K where e is kept
      continue;
    }
    const int rc = attr_tc_parse(h_blobs[f], h_lens[f], &o, tc ? &o : nullptr, false);
    if (rc != PCC_OK) return a_wrap_error(who, f, rc);
    if (h_cell_offsets) {
      const int64_t m = h_cell_offsets[f + 1] - h_cell_offsets[f];
      PCC_REQUIRE(m == o.n, PCC_E_STREAM, "%s: frame %d: the attribute blob has %lld values, its geometry %lld points", who, f,
                  (long long)o.n, (long long)m);
    }
    const int64_t last_words = o.n ? attr_u32(h_blobs[f] + o.off_table + 4 * (o.nc - 1)) : 0;
    a_dec_count(d, f, ADecIn{&o, o.n, o.nc, last_words, h_lens[f] - o.off_p0, o.qstep, o.slod});   // q where the near-lossless kinds keep e
  }
  bool idle;
  PCC_TRY(a_dec_counted(d, "values", &idle));
  if (idle) return PCC_OK;
  std::vector<A2Order> order;
  std::vector<int32_t> aux;
  int64_t blocks, cells_all, vals_max = 0;
  const int32_t* cells;
  PCC_TRY(a_dec_order(d, d_cells, h_cell_offsets, &order, &blocks, &cells_all, &cells));
  bool any_colour = false;
  for (const AttrSInfo& o : info) {
    if (o.n == 0) continue;
    vals_max = std::max(vals_max, o.n * o.c);
    if (!tc) continue;
    for (int ch = 0; ch < 4; ++ch) aux.push_back((int32_t)o.q[ch]);
    aux.push_back((int32_t)o.colour);
    any_colour |= o.colour != 0;
  }
  d.order = order.data();
  if (tc) d.aux = aux.data();
  const int nf = d.nf;
  const size_t keys_b = pcc_align((size_t)cells_all * 8), u32_b = pcc_align((size_t)cells_all * 4), pk_b = pcc_align((size_t)cells_all * 2);
  const size_t hist_b = pcc_align((size_t)blocks * kATBins * 4), bins_b = pcc_align((size_t)nf * 2 * kATBins * 4);
  const size_t val_b = pcc_align((size_t)d.bytes * 8), status_b = pcc_align((size_t)nf * 4 + 64);
  PCC_TRY(a_dec_plan(d, d_out ? 1 : 2, val_b + keys_b + u32_b + pk_b + hist_b + bins_b + status_b + (sc ? a_s_cells_bytes(cells_all) : 0) + 8192));
  hipStream_t st = ctx->stream;
  uint8_t* x = (uint8_t*)pcc_arena_alloc(ctx, (size_t)d.bytes);
  int64_t* val = (int64_t*)pcc_arena_alloc(ctx, val_b);
  uint64_t* keys = (uint64_t*)pcc_arena_alloc(ctx, keys_b);
  uint32_t* inv = (uint32_t*)pcc_arena_alloc(ctx, u32_b);
  uint16_t* packed = (uint16_t*)pcc_arena_alloc(ctx, pk_b);
  uint32_t* hist = (uint32_t*)pcc_arena_alloc(ctx, hist_b);
  uint32_t* bins = (uint32_t*)pcc_arena_alloc(ctx, bins_b);
  int32_t* status = (int32_t*)pcc_arena_alloc(ctx, status_b);
  if (!x || !val || !keys || !inv || !packed || !hist || !bins || !status) return PCC_E_NOMEM;
  PccProfScope prof(ctx, "attr_decode_transform", d.points, nf, d.chunks, 0);
  const size_t bins_back = (size_t)nf * 2 * kATBins * 4;   // read back: the sublevels' starts and counts | status
  PCC_TRY(a_dec_send(d, bins_back + (size_t)nf * 4));
  PCC_HIP(hipMemsetAsync(status, 0, (size_t)nf * 4, st));
  const ADFrame* d_tab = (const ADFrame*)d.d_in;
  const A2Order* d_ord = (const A2Order*)(d.d_in + d.ord_at);
  const int32_t* d_aux = tc ? (const int32_t*)(d.d_in + d.aux_at) : nullptr;
  PCC_TRY(a_launch_dec<true>(d, x, status));
  unsigned grid[kATBins];
  PCC_TRY(a_t_order(st, true, (const void*)cells, keys, d_ord, nf, blocks, packed, hist, bins, inv, (uint32_t*)d.back, grid));
  const uint32_t* g = nullptr;
  if (sc) {
    // the counts of the cells themselves (read back behind the order stage's synchronisation) against the head's, level by
    // level from lod up: count[K] among them, which M is formed from
    for (int f = 0, k = 0; f < n_frames; ++f) {
      if (d.in[(size_t)f].n_dec == 0) continue;
      const uint32_t* hb = (const uint32_t*)d.back + (size_t)k++ * 2 * kATBins;
      for (int j = lod; j <= kAttrMaxLod; ++j) {
        const int64_t own = (int64_t)hb[3 * (j - lod)] + hb[kATBins + 3 * (j - lod)];
        PCC_REQUIRE(own == info[(size_t)f].cells[j], PCC_E_STREAM,
                    "%s: frame %d: attribute blob: level of detail %d announces %lld values, the cells give %lld", who, f, j,
                    (long long)info[(size_t)f].cells[j], (long long)own);
      }
    }
    PCC_TRY(a_s_cells(ctx, st, d_ord, nf, blocks, packed, nullptr, d_tab, 3 * lod, cells_all, &g));
  }
  hipLaunchKernelGGL(k_at_root, dim3(nblk(4 * (int64_t)nf, 256)), dim3(256), 0, st, d_tab, nf, (const uint8_t*)x, val);
  PCC_CHECK_LAUNCH();
  for (int t = kATBins - 2; t >= 0; --t) {
    if (!grid[t]) continue;
    PCC_TRY(a_launch_lift<false>(st, grid[t], nf, keys, d_ord, bins, inv, t, nullptr, nullptr, nullptr, d_tab, x, val, status, d_aux, g, 3 * lod));
  }
  if (sc || any_colour)
    hipLaunchKernelGGL(k_ac_store, dim3(nblk(d.n_max, 256), (unsigned)nf), dim3(256), 0, st, d_tab, d_aux, (const int64_t*)val, d.out);
  else
    hipLaunchKernelGGL(k_at_store, dim3(nblk(vals_max, 256), (unsigned)nf), dim3(256), 0, st, d_tab, (const int64_t*)val, d.out);
  PCC_CHECK_LAUNCH();
  return a_dec_finish(d, status, (size_t)nf * 4, bins_back, bins_back, ", 8 = keys");
}

// ---- version 2: levels of detail ----------------------------------------------------------------------------------
extern "C" int pcc_attr_lod_info(const uint8_t* h_in, int64_t len, int lod, int64_t* h_bytes, int64_t* h_values) {
  PCC_REQUIRE(lod >= 0 && lod <= kAttrMaxLod, PCC_E_ARG, "pcc_attr_lod_info: level of detail %d outside 0 .. %d", lod, kAttrMaxLod);
  PCC_REQUIRE(h_in && len >= 2 && h_in[0] == 'A', PCC_E_STREAM, "pcc_attr_lod_info: not an attribute blob (len=%lld)", (long long)len);
  Attr2Plan pl;
  int rc;
  if (attr_s_kind(h_in[1])) {   // version 22: its own parser, version 2's plan; a level above its K is PCC_E_ARG
    AttrSInfo o;
    rc = attr_s_parse(h_in, len, lod, kAttrSPlan, &o, &pl);
  } else {
    bool scal = false, nl = false, xc = false, nbr = false;
    PCC_REQUIRE(!attr_t_kind(h_in[1]) && !attr_c_kind(h_in[1]), PCC_E_ARG,
                "pcc_attr_lod_info: attribute blob version %d (a transform-coded blob has no level-of-detail prefixes: the weights of its "
                "transform need every point)", (int)h_in[1]);
    PCC_REQUIRE(attr_kind12(h_in[1], &scal, &nl, &xc, &nbr) && scal, PCC_E_ARG,
                "pcc_attr_lod_info: attribute blob version %d (levels of detail are a property of version 2)", (int)h_in[1]);
    Attr2Info o;
    rc = attr2_parse_kind(h_in, len, lod, false, nl, &o, &pl, xc, nbr);
  }
  if (rc != PCC_OK) return a_wrap_error("pcc_attr_lod_info", rc);
  if (h_bytes) *h_bytes = pl.bytes;
  if (h_values) *h_values = pl.m;
  return PCC_OK;
}

extern "C" int pcc_attr_decode_frames_lod(pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames, int lod,
                                          const int32_t* d_cells, const int64_t* h_cell_offsets, uint8_t* d_out, uint8_t* h_out,
                                          int64_t cap_bytes, int64_t* h_out_offsets, int32_t* h_format) {
  const char* who = "pcc_attr_decode_frames_lod";
  PCC_REQUIRE(ctx && h_blobs && h_lens && h_out_offsets && n_frames >= 1 && n_frames <= 65535, PCC_E_ARG,
              "%s: bad argument (n_frames=%d)", who, n_frames);
  PCC_REQUIRE(lod >= 0 && lod <= kAttrMaxLod, PCC_E_ARG, "%s: level of detail %d outside 0 .. %d", who, lod, kAttrMaxLod);
  // versions 19, 21 and 22 (one version per call): their own decoder, the first two at lod 0, 22 up to every blob's K
  for (const int tv : {kAttrTVersion, kAttrCVersion, kAttrSVersion}) {
    bool any = false;
    for (int f = 0; f < n_frames; ++f) any |= a_is_version(h_blobs[f], h_lens[f], tv);
    if (!any) continue;
    for (int f = 0; f < n_frames; ++f)
      PCC_REQUIRE(a_is_version(h_blobs[f], h_lens[f], tv), PCC_E_ARG,
                  "%s: frame %d: attribute blobs of version %d and of another version in one call (one version per call)", who, f, tv);
    PCC_REQUIRE(lod == 0 || attr_s_kind(tv), PCC_E_ARG, "%s: attribute blob version %d at level of detail %d (it decodes at 0 only)", who,
                tv, lod);
    return a_t_decode_frames(who, ctx, h_blobs, h_lens, n_frames, d_cells, h_cell_offsets, d_out, h_out, cap_bytes, h_out_offsets, h_format, tv,
                             lod);
  }
  // the blobs of a call are of one version, the first blob's: 2, or 7 (k_a2_walk<true> scales and clamps), or their
  // cross-channel forms 11 and 14 (k_ax_inv between the decoder and the walk), or 25 or its cross form 26 (k_an_plan for
  // k_a2_place, and k_an_recon size by size for the walk)
  // (28 / 31: the launches of 25 / 26 with k_anl_recon, which scales and clamps as the walk of version 7 does)
  const int kinds[8] = {2, 7, 11, 14, kAttrNVersion, kAttrNXVersion, kAttrNLVersion, kAttrNLXVersion};
  const int mine = a_call_version(h_blobs[0], h_lens[0], kinds);
  bool scal, nl, xc, nbr;
  attr_kind12(mine, &scal, &nl, &xc, &nbr);
  ADecCall d = a_dec_call(who, ctx, h_blobs, n_frames, d_out, h_out, cap_bytes, h_out_offsets, h_format);
  std::vector<Attr2Info> info((size_t)n_frames);
  for (int f = 0; f < n_frames; ++f) {
    Attr2Info& o = info[(size_t)f];
    Attr2Plan pl;
    PCC_TRY(a_mixed_version(who, f, h_blobs[f], h_lens[f], kinds, mine));
    const int rc = attr2_parse_kind(h_blobs[f], h_lens[f], lod, true, nl, &o, &pl, xc, nbr);
    if (rc != PCC_OK) return a_wrap_error(who, f, rc);
    if (h_cell_offsets) {
      const int64_t m = h_cell_offsets[f + 1] - h_cell_offsets[f];
      PCC_REQUIRE(m == pl.m, PCC_E_STREAM, "%s: frame %d: the attribute blob has %lld values at level of detail %d, its geometry %lld cells",
                  who, f, (long long)pl.m, lod, (long long)m);
    }
    PCC_REQUIRE(o.slod + lod <= kAttrMaxLod, PCC_E_ARG,
                "%s: frame %d: level of detail %d of cells the sender coded at its level %d: beyond %d", who, f, lod, o.slod, kAttrMaxLod);
    a_dec_count(d, f, ADecIn{&o, pl.m, pl.chunks, pl.last_words, pl.bytes - o.off_p0, o.max_error, lod + o.slod});   // the level's bytes only
  }
  bool idle;
  PCC_TRY(a_dec_counted(d, "values", &idle));
  if (idle) return PCC_OK;
  std::vector<A2Order> order;
  std::vector<int32_t> cross;   // the masks of versions 11 and 14
  int64_t blocks, cells_all;
  const int32_t* cells;
  PCC_TRY(a_dec_order(d, d_cells, h_cell_offsets, &order, &blocks, &cells_all, &cells));
  for (int f = 0; f < n_frames; ++f)
    if (d.in[(size_t)f].n_dec) cross.push_back(info[(size_t)f].cross);
  d.order = order.data();
  if (xc) d.masks = cross.data();
  const int nf = d.nf;
  const size_t keys_b = pcc_align((size_t)cells_all * 8), u32_b = pcc_align((size_t)cells_all * 4), pk_b = pcc_align((size_t)cells_all * 2);
  // 17 bin bases per frame | 16 counts per frame | status per frame: the last two come back in one copy
  const size_t hist_b = pcc_align((size_t)blocks * kA2Bins * 4), bins_b = pcc_align((size_t)nf * 34 * 4 + 64);
  // versions 25 / 26: `rank` holds the inverse of the places and `first` every cell's choice, 3 words
  const size_t first_b = nbr ? pcc_align((size_t)cells_all * 12) : u32_b;
  PCC_TRY(a_dec_plan(d, d_out ? 1 : 2, keys_b + u32_b + first_b + pk_b + hist_b + bins_b + 8192));
  hipStream_t st = ctx->stream;
  uint8_t* resid = (uint8_t*)pcc_arena_alloc(ctx, (size_t)d.bytes);
  uint64_t* keys = (uint64_t*)pcc_arena_alloc(ctx, keys_b);
  uint32_t* rank = (uint32_t*)pcc_arena_alloc(ctx, u32_b);
  uint32_t* first = (uint32_t*)pcc_arena_alloc(ctx, first_b);
  uint16_t* packed = (uint16_t*)pcc_arena_alloc(ctx, pk_b);
  uint32_t* hist = (uint32_t*)pcc_arena_alloc(ctx, hist_b);
  uint32_t* bins = (uint32_t*)pcc_arena_alloc(ctx, bins_b);
  if (!resid || !keys || !rank || !first || !packed || !hist || !bins) return PCC_E_NOMEM;
  uint32_t* counts = bins + (size_t)nf * kA2Bins;
  int32_t* status = (int32_t*)(counts + (size_t)nf * 16);
  PccProfScope prof(ctx, "attr_decode_lod", d.points, nf, d.chunks, 0);
  PCC_TRY(a_dec_send(d, (size_t)nf * 17 * 4));
  PCC_HIP(hipMemsetAsync(status, 0, (size_t)nf * 4, st));
  const ADFrame* d_tab = (const ADFrame*)d.d_in;
  const A2Order* d_ord = (const A2Order*)(d.d_in + d.ord_at);
  // the introduction order of the cells: nothing of it depends on the attribute stream
  hipLaunchKernelGGL(k_a2_size<true>, dim3((unsigned)blocks), dim3(256), 0, st, (const void*)cells, d_ord, nf, keys, packed, hist);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_a2_scan, dim3((unsigned)nf), dim3(256), 0, st, d_ord, hist, bins, counts);
  PCC_CHECK_LAUNCH();
  if (nbr) {
    hipLaunchKernelGGL(k_an_plan, dim3((unsigned)blocks), dim3(256), 0, st, (const uint64_t*)keys, d_ord, nf, (const uint16_t*)packed,
                       (const uint32_t*)hist, (const uint32_t*)bins, rank, first);
  } else {
    hipLaunchKernelGGL(k_a2_place<false>, dim3((unsigned)blocks), dim3(256), 0, st, (const uint64_t*)keys, d_ord, nf, (const uint16_t*)packed,
                       (const uint32_t*)hist, (const uint32_t*)bins, (const AFrame*)nullptr, (const uint16_t*)nullptr, (uint16_t*)nullptr,
                       rank, first);
  }
  PCC_CHECK_LAUNCH();
  PCC_TRY(a_launch_dec<true>(d, resid, status));
  if (xc) {
    hipLaunchKernelGGL(k_ax_inv, dim3(nblk(d.n_max, 256), (unsigned)nf), dim3(256), 0, st, d_tab, (const int32_t*)(d.d_in + d.masks_at()), resid);
    PCC_CHECK_LAUNCH();
  }
  if (nbr) {
    // sizes 16 .. 0 of the cells, each over its range of the introduction order, all frames in one grid.  The grid of a
    // size comes from the heads' counts (size j of the cells: cells[lod + j] - cells[lod + j + 1], point 0 alone at 16),
    // which the parser bounded and counts_match holds against the cells below; the ranges themselves are the order
    // stage's, on the device.  A size without a point in any frame is not launched
    for (int s = kA2Bins - 1; s >= 0; --s) {
      int64_t most = 0;
      for (int f = 0; f < n_frames; ++f) {
        if (d.in[(size_t)f].n_dec == 0) continue;
        const int64_t* c = info[(size_t)f].cells;
        const int j = lod + s;
        most = std::max<int64_t>(most, s == 16 ? 1 : (j > kAttrMaxLod ? 0 : c[j] - (j < kAttrMaxLod ? c[j + 1] : 1)));
      }
      if (most == 0) continue;
      hipLaunchKernelGGL((nl ? k_anl_recon : k_an_recon), dim3(nblk(most, 256), (unsigned)nf), dim3(256), 0, st, d_ord, d_tab, (const uint32_t*)bins, s,
                         (const uint32_t*)rank, (const uint32_t*)first, (const uint8_t*)resid, d.out, status);
      PCC_CHECK_LAUNCH();
    }
  } else {
    hipLaunchKernelGGL((nl ? k_a2_walk<true> : k_a2_walk<false>), dim3((unsigned)blocks), dim3(256), 0, st, d_ord, nf, d_tab,
                       (const uint32_t*)rank, (const uint32_t*)first, (const uint8_t*)resid, d.out, status);
    PCC_CHECK_LAUNCH();
  }
  // counts and status come back in one copy; per frame, the coarser levels' counts of the header against those of the
  // cells themselves, then its status
  const auto counts_match = [&](int f, int k) -> int {
    const uint32_t* h_counts = (const uint32_t*)d.back + 16 * k;
    for (int j = 0; lod + j <= kAttrMaxLod; ++j)
      PCC_REQUIRE((int64_t)h_counts[j] == info[(size_t)f].cells[lod + j], PCC_E_STREAM,
                  "%s: frame %d: attribute blob: level of detail %d announces %lld values, the cells give %u", who, f, lod + j,
                  (long long)info[(size_t)f].cells[lod + j], h_counts[j]);
    return PCC_OK;
  };
  return a_dec_finish(d, counts, (size_t)nf * 17 * 4, 0, (size_t)nf * 16 * 4,
                      nbr ? (nl ? ", 8 = index outside the frame, 16 = reconstruction out of range" : ", 8 = index outside the frame")
                          : (nl ? ", 8 = predictor chain, 16 = reconstruction out of range" : ", 8 = predictor chain"),
                      counts_match);
}
