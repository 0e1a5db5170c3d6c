// transfer.hip — attribute transfer onto another geometry (recolouring): what consumes the two pairings of pcc_nn_frames
// (nn.hip) when a frame's attributes have to follow its points onto a different point set.  include/pcc.h has the
// rule; tests/transfer_ref.py restates it in numpy.  No search runs here: both row arrays come from the caller.
//
//   accumulate  one thread per source row, in the order of the sorted source keys.  Its target row t = row_st[i].
//               Morton-sorted sources mostly share a target with their neighbour, so the wave first sums every run of
//               equal adjacent target rows among its 64 lanes (a segmented suffix sum over shuffles, 32-bit: 64 values
//               of at most 65535) and the first lane of each run issues the run's atomics: one 64-bit integer add per
//               channel and one for the count, into acc[n_t][channels + 1], zeroed by the call.  A target that shows in
//               two separate runs of a wave (A, B, A) gets two sets of atomics; integer addition does not mind.
//   finish      one thread per target.  count > 0: the rounded mean (sum + count / 2) / count.  count == 0: the merged
//               value of the distinct source point row_ts[t] — the same rounded mean over its run of duplicate rows,
//               read from the sorted values (the loop of k_a_merge).  Neither: 0.
//
// Every index read from an array is checked before it is used: a target row outside [0, n_t), a distinct source row
// outside [0, n_su), a run start behind n_s and a source key whose frame index is not below n_frames contribute
// nothing.  Sums are integers, so the result does not depend on the order in which the atomics land.
#include "common.h"
#include "nn_cells.h"

template <typename T>
__global__ __launch_bounds__(256) void k_transfer_accumulate(const uint64_t* __restrict__ skeys, const int32_t* __restrict__ row_st,
                                                             int64_t n_s, const T* __restrict__ values, int64_t n_t, int channels,
                                                             int n_frames, unsigned long long* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t t = -1;      // -1: this lane adds nothing
  uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0, cnt = 0;
  if (i < n_s) {
    const int64_t r = row_st[i];
    if (r >= 0 && r < n_t && (skeys[i] >> 48) < (uint64_t)n_frames) {
      t = (int32_t)r;      // n_t <= 2^27
      cnt = 1;
      const T* p = values + i * channels;
      e0 = p[0];
      if (channels > 1) e1 = p[1];
      if (channels > 2) e2 = p[2];
      if (channels > 3) e3 = p[3];
    }
  }
  // every lane of the wave is here.  A run: adjacent lanes of equal t; `end` is the lane behind this lane's run
  const int32_t before = __shfl_up(t, 1);
  const bool head = lane == 0 || before != t;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int end = above ? lane + __ffsll((long long)above) : 64;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {      // after the step of `off`, a lane holds the sum of 2 off lanes of its run
    const uint32_t o0 = __shfl_down(e0, off), o1 = __shfl_down(e1, off), o2 = __shfl_down(e2, off), o3 = __shfl_down(e3, off),
                   oc = __shfl_down(cnt, off);
    if (lane + off < end) {
      e0 += o0;
      e1 += o1;
      e2 += o2;
      e3 += o3;
      cnt += oc;
    }
  }
  if (!head || t < 0) return;
  // a sum of 0 needs no atomic: the channels a caller padded its rows with (GeometryCodec.transfer) cost nothing
  unsigned long long* a = acc + (size_t)t * (channels + 1);
  if (e0) atomicAdd(&a[0], (unsigned long long)e0);
  if (e1) atomicAdd(&a[1], (unsigned long long)e1);
  if (e2) atomicAdd(&a[2], (unsigned long long)e2);
  if (e3) atomicAdd(&a[3], (unsigned long long)e3);
  atomicAdd(&a[channels], (unsigned long long)cnt);
}

// (s + c / 2) / c, c > 0: in 32 bits where the dividend fits them (every run of duplicates, every target of fewer than
// 65536 sources), else in 64
__device__ static inline uint32_t transfer_mean(unsigned long long s, unsigned long long c) {
  const unsigned long long d = s + c / 2;
  return (d >> 32) == 0 ? (uint32_t)d / (uint32_t)c : (uint32_t)(d / c);
}

template <typename T>
__global__ __launch_bounds__(256) void k_transfer_finish(const unsigned long long* __restrict__ acc, const int32_t* __restrict__ row_ts,
                                                         int64_t n_t, const uint64_t* __restrict__ skeys,
                                                         const uint32_t* __restrict__ sruns, int64_t n_su,
                                                         const T* __restrict__ values, int64_t n_s, int channels, int n_frames,
                                                         T* __restrict__ out, uint32_t* __restrict__ count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_t) return;
  const unsigned long long* a = acc + (size_t)t * (channels + 1);
  unsigned long long s0 = a[0], s1 = channels > 1 ? a[1] : 0ull, s2 = channels > 2 ? a[2] : 0ull, s3 = channels > 3 ? a[3] : 0ull;
  unsigned long long cnt = a[channels];
  if (count) count[t] = (uint32_t)cnt;      // at most n_s <= 2^27
  if (cnt == 0) {      // no source row chose this target: its nearest distinct source point, merged
    const int64_t u = row_ts[t];
    if (u >= 0 && u < n_su) {
      int64_t r0 = sruns[u], r1 = u + 1 < n_su ? (int64_t)sruns[u + 1] : n_s;
      if (r1 > n_s) r1 = n_s;
      s0 = s1 = s2 = s3 = 0;
      for (int64_t r = r0; r < r1; ++r) {
        if ((skeys[r] >> 48) >= (uint64_t)n_frames) continue;
        const T* p = values + r * channels;
        s0 += p[0];
        if (channels > 1) s1 += p[1];
        if (channels > 2) s2 += p[2];
        if (channels > 3) s3 += p[3];
        ++cnt;
      }
    }
  }
  T* o = out + t * channels;
  o[0] = cnt ? (T)transfer_mean(s0, cnt) : (T)0;
  if (channels > 1) o[1] = cnt ? (T)transfer_mean(s1, cnt) : (T)0;
  if (channels > 2) o[2] = cnt ? (T)transfer_mean(s2, cnt) : (T)0;
  if (channels > 3) o[3] = cnt ? (T)transfer_mean(s3, cnt) : (T)0;
}

template <typename T>
static int transfer_launch(pcc_ctx* ctx, const uint64_t* d_skeys, int64_t n_s, const uint32_t* d_sruns, int64_t n_su, const void* d_svalues,
                           const int32_t* d_row_st, const int32_t* d_row_ts, int64_t n_t, int channels, int n_frames,
                           unsigned long long* acc, void* d_out, uint32_t* d_count) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_transfer_accumulate<T>, dim3(nblk(n_s, 256)), dim3(256), 0, st, d_skeys, d_row_st, n_s, (const T*)d_svalues, n_t,
                     channels, n_frames, acc);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_transfer_finish<T>, dim3(nblk(n_t, 256)), dim3(256), 0, st, (const unsigned long long*)acc, d_row_ts, n_t, d_skeys,
                     d_sruns, n_su, (const T*)d_svalues, n_s, channels, n_frames, (T*)d_out, d_count);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
extern "C" int pcc_attr_transfer_frames(pcc_ctx* ctx, const uint64_t* d_skeys, int64_t n_s, const uint32_t* d_sruns, int64_t n_su,
                                        const void* d_svalues, const int32_t* d_row_st, const int32_t* d_row_ts, int64_t n_t, int bpv,
                                        int channels, int n_frames, void* d_out, uint32_t* d_count) {
  PCC_REQUIRE(ctx && n_frames >= 1 && n_frames <= 65535 && n_s >= 0 && n_s <= NN_MAX_KEYS && n_t >= 0 && n_t <= NN_MAX_KEYS && n_su >= 0 &&
                  n_su <= n_s && (n_su > 0) == (n_s > 0) && (bpv == 1 || bpv == 2) && channels >= 1 && channels <= 4,
              PCC_E_ARG, "pcc_attr_transfer_frames: bad argument (n_s=%lld n_su=%lld n_t=%lld n_frames=%d bpv=%d channels=%d)",
              (long long)n_s, (long long)n_su, (long long)n_t, n_frames, bpv, channels);
  PCC_REQUIRE(n_s == 0 || (d_skeys && d_sruns && d_svalues && d_row_st), PCC_E_ARG, "pcc_attr_transfer_frames: null source arrays");
  PCC_REQUIRE(n_t == 0 || (d_row_ts && d_out), PCC_E_ARG, "pcc_attr_transfer_frames: null target arrays");
  if (n_t == 0) return PCC_OK;
  hipStream_t st = ctx->stream;
  if (n_s == 0) {      // no source anywhere: value 0, count 0; no kernel
    PCC_HIP(hipMemsetAsync(d_out, 0, (size_t)n_t * channels * bpv, st));
    if (d_count) PCC_HIP(hipMemsetAsync(d_count, 0, (size_t)n_t * 4, st));
    return PCC_OK;
  }
  const size_t acc_b = (size_t)n_t * (channels + 1) * 8;
  PCC_TRY(pcc_arena_reserve(ctx, pcc_align(acc_b) + 256));
  unsigned long long* acc = (unsigned long long*)pcc_arena_alloc(ctx, acc_b);
  if (!acc) return PCC_E_NOMEM;
  PCC_HIP(hipMemsetAsync(acc, 0, acc_b, st));
  PccProfScope prof(ctx, "attr_transfer", n_s, n_t, channels, bpv);
  return bpv == 1 ? transfer_launch<uint8_t>(ctx, d_skeys, n_s, d_sruns, n_su, d_svalues, d_row_st, d_row_ts, n_t, channels, n_frames, acc,
                                             d_out, d_count)
                  : transfer_launch<uint16_t>(ctx, d_skeys, n_s, d_sruns, n_su, d_svalues, d_row_st, d_row_ts, n_t, channels, n_frames, acc,
                                              d_out, d_count);
}
