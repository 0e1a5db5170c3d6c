// metric.hip — the metric front and back end of the frame codec (GeometryCodec): float32 points in metres onto the
// int16 lattice and into Morton keys in one pass, the row index of a compress call, lattice points back to metres.
//
// The quantisation rule (include/pcc.h has the contract): per coordinate, in float32, q = rint((x - o) / v) — one IEEE
// subtraction, one correctly rounded division, round-half-to-even; back: x = o + t * v, one multiplication, then one
// addition.  Every step is spelled with its _rn intrinsic, so neither a reciprocal nor a contraction can take its
// place whatever the build's flags say.
//
// Three plain data-parallel passes: no LDS, every global access guarded by the row count.
#include "common.h"

// one coordinate: *q = rint((x - o) / v) as a float; 0 = on the grid, 1 = finite but off the grid, 2 = not finite
__device__ __forceinline__ int quantise(float x, float o, float v, float* q) {
  if (!(fabsf(x) <= 3.402823466e+38f)) return 2;   // NaN, +Inf, -Inf
  *q = rintf(__fdiv_rn(__fsub_rn(x, o), v));
  return !(*q >= -32768.f && *q <= 32767.f) ? 1 : 0;   // on the float, NaN-safe, before any conversion to int
}

// keys of a sequence of float32 frames: xyz [n, 3], frames concatenated, frame f = rows [offs[f], offs[f + 1]) (the
// search of k_morton_keys_frames).  status[0] |= 1 for a finite coordinate off the grid, |= 2 for a non-finite one
// (drop == 0).  drop != 0: a row with a non-finite coordinate gets the key n_frames << 48 instead, which sorts behind
// every frame's keys, and is counted in status[1] (one atomic per wave).  12 B in, 8 B out per row.
__global__ __launch_bounds__(256) void k_morton_keys_frames_f32(const float* __restrict__ xyz, int64_t n,
                                                                const int64_t* __restrict__ offs, int n_frames, float v,
                                                                float ox, float oy, float oz, int drop,
                                                                uint64_t* __restrict__ keys, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool dropped = false;
  if (i < n) {
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (offs[mid] <= i) lo = mid; else hi = mid - 1;
    }
    float qx = 0.f, qy = 0.f, qz = 0.f;
    const int sx = quantise(xyz[3 * i], ox, v, &qx), sy = quantise(xyz[3 * i + 1], oy, v, &qy),
              sz = quantise(xyz[3 * i + 2], oz, v, &qz);
    const int s = sx | sy | sz;
    uint64_t key = (uint64_t)(uint32_t)n_frames << 48;
    if (s & 2) {
      dropped = drop != 0;
      if (!dropped) atomicOr(&status[0], 2);
    } else if (s & 1) {
      atomicOr(&status[0], 1);
    } else {
      key = pcc_morton(lo, (int)qx, (int)qy, (int)qz);
    }
    keys[i] = key;
  }
  const unsigned long long m = __ballot(dropped);      // every lane of the wave is still here
  if (dropped && (m & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0ull) atomicAdd(&status[1], (int32_t)__popcll(m));
}

// index[r] for every input row r of a compress call: sorted position t holds row perm[t]; the kept rows are positions
// [0, n_keep), run u starts at position runs[u] (n_runs of them, ascending, runs[0] = 0); row r lies in frame f with
// offs[f] <= r < offs[f + 1], whose first run is first_run[f].  index[r] = its run counted from its frame's first, or
// -1 behind n_keep.  The run is found by a binary search (n_runs < 2^27: at most 27 steps); the scatter through perm
// is the only uncoalesced access.
__global__ __launch_bounds__(256) void k_rows_index(const uint32_t* __restrict__ perm, int64_t n, int64_t n_keep,
                                                    const uint32_t* __restrict__ runs, int64_t n_runs,
                                                    const int64_t* __restrict__ offs, const int64_t* __restrict__ first_run,
                                                    int n_frames, int32_t* __restrict__ index) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t r = perm[t];
  if (r >= n) return;      // not a permutation of the call's rows: nothing is written out of bounds
  if (t >= n_keep || n_runs <= 0) {
    index[r] = -1;
    return;
  }
  int64_t lo = 0, hi = n_runs - 1;      // the last run that starts at or before t
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if ((int64_t)runs[mid] <= t) lo = mid; else hi = mid - 1;
  }
  int f = 0, fh = n_frames - 1;
  while (f < fh) {
    const int mid = (f + fh + 1) >> 1;
    if (offs[mid] <= r) f = mid; else fh = mid - 1;
  }
  index[r] = (int32_t)(lo - first_run[f]);
}

// lattice points or cells of a decode back to metres, one thread per coordinate: t = c at lod 0, the centre of the
// cell's lattice points (c << k) + (2^k - 1) / 2 at lod k — a half-integer below 2^16 in size, exact in float32 — and
// x = o + t * v.  12 B in, 12 B out per point.
__global__ __launch_bounds__(256) void k_points_to_metric(const int32_t* __restrict__ cells, int64_t n3, int lod, float v,
                                                          float ox, float oy, float oz, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  const int axis = (int)(i % 3);
  const float o = axis == 0 ? ox : (axis == 1 ? oy : oz);
  const int32_t c = cells[i];
  const float t = 0.5f * (float)((int32_t)((uint32_t)c * (2u << lod)) + ((1 << lod) - 1));      // an integer below 2^17: exact
  out[i] = __fadd_rn(o, __fmul_rn(t, v));
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
extern "C" int pcc_morton_keys_frames_f32(pcc_ctx* ctx, const float* d_xyz, int64_t n, const int64_t* d_frame_offsets,
                                          int n_frames, float voxel, const float* h_origin, int drop, uint64_t* d_keys,
                                          int32_t* d_status) {
  PCC_REQUIRE(ctx && h_origin && n_frames >= 1 && n_frames <= 65535 && n >= 0 &&
                  (n == 0 || (d_xyz && d_frame_offsets && d_keys && d_status)),
              PCC_E_ARG, "pcc_morton_keys_frames_f32: bad argument (n_frames=%d)", n_frames);
  PCC_REQUIRE(voxel > 0.f && voxel <= 3.402823466e+38f && fabsf(h_origin[0]) <= 3.402823466e+38f &&
                  fabsf(h_origin[1]) <= 3.402823466e+38f && fabsf(h_origin[2]) <= 3.402823466e+38f,
              PCC_E_ARG, "pcc_morton_keys_frames_f32: voxel %g must be positive and finite, the origin finite", (double)voxel);
  PCC_REQUIRE(n < ((int64_t)1 << 31), PCC_E_ARG, "pcc_morton_keys_frames_f32: n too large");
  if (n <= 0) return PCC_OK;
  hipLaunchKernelGGL(k_morton_keys_frames_f32, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, d_xyz, n, d_frame_offsets,
                     n_frames, voxel, h_origin[0], h_origin[1], h_origin[2], drop, d_keys, d_status);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_rows_index(pcc_ctx* ctx, const uint32_t* d_perm, int64_t n, int64_t n_keep, const uint32_t* d_run_starts,
                              int64_t n_unique, const int64_t* d_frame_offsets, const int64_t* d_first_run, int n_frames,
                              int32_t* d_index) {
  PCC_REQUIRE(ctx && n_frames >= 1 && n_frames <= 65535 && n >= 0 && n < ((int64_t)1 << 31) && n_keep >= 0 &&
                  n_keep <= n && n_unique >= 0 && n_unique <= n_keep && n_unique < ((int64_t)1 << 27) &&
                  (n_unique > 0) == (n_keep > 0),
              PCC_E_ARG, "pcc_rows_index: bad argument (n=%lld kept=%lld runs=%lld n_frames=%d)", (long long)n,
              (long long)n_keep, (long long)n_unique, n_frames);
  PCC_REQUIRE(n == 0 || (d_perm && d_frame_offsets && d_first_run && d_index && (n_unique == 0 || d_run_starts)), PCC_E_ARG,
              "pcc_rows_index: null arg");
  if (n <= 0) return PCC_OK;
  hipLaunchKernelGGL(k_rows_index, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, d_perm, n, n_keep, d_run_starts, n_unique,
                     d_frame_offsets, d_first_run, n_frames, d_index);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_points_to_metric(pcc_ctx* ctx, const int32_t* d_points, int64_t n, int lod, float voxel,
                                    const float* h_origin, float* d_out) {
  PCC_REQUIRE(ctx && h_origin && n >= 0 && n < ((int64_t)1 << 40) && lod >= 0 && lod <= 15 && (n == 0 || (d_points && d_out)),
              PCC_E_ARG, "pcc_points_to_metric: bad argument (lod=%d)", lod);
  PCC_REQUIRE(voxel > 0.f && voxel <= 3.402823466e+38f && fabsf(h_origin[0]) <= 3.402823466e+38f &&
                  fabsf(h_origin[1]) <= 3.402823466e+38f && fabsf(h_origin[2]) <= 3.402823466e+38f,
              PCC_E_ARG, "pcc_points_to_metric: voxel %g must be positive and finite, the origin finite", (double)voxel);
  if (n <= 0) return PCC_OK;
  hipLaunchKernelGGL(k_points_to_metric, dim3(nblk(3 * n, 256)), dim3(256), 0, ctx->stream, d_points, 3 * n, lod, voxel,
                     h_origin[0], h_origin[1], h_origin[2], d_out);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}
