// attr_stage.hip — per-point attributes of a call from wherever they lie on the device into the layouts the attribute
// coders, distortion and transfer read: uint8 / uint16 rows as they are, float32 / float64 rows quantised under the
// rule of include/pcc.h (tests/attr_stage_ref.py restates it in numpy).  One memory-bound pass, one thread per row.
//
//   packed   frame f's rows tight as [rows_f][c_f] of its own width at byte out_offset[f] of d_out: what
//            pcc_attr_encode_frames and its siblings take as d_values.  The pad bytes between frames are not written.
//   sorted   d_out [n][channels] of one width, rows of 4 or 8 bytes: row i is source row d_perm[i] of the call,
//            widened, absent channels 0 — in place of a widening on the host, an upload and pcc_gather_rows.
//
// The row's frame is found by a bounded binary search over the row offsets (at most 16 steps for 65535 frames); lanes
// past n leave early; no LDS, no shuffles, no atomics except the status atomicOr.  Sources are read element by element
// at pitch * row + ch, so a [:, 4:7] view of an interleaved tensor needs no copy; with pitch == c adjacent lanes read
// adjacent addresses.  In sorted mode every lane issues one 4- or 8-byte store at out + i * row bytes; in packed mode
// rows of 1, 2, 4 and 8 bytes are one store, rows of 3 and 6 bytes three.
//
// Every index is checked before it is used: a d_perm entry >= n reads nothing, writes a zero row and sets status bit 1;
// a record's channel count is cut to 1 .. 4 and to the row's channels, a row in front of its frame's first reads nothing.
#include "common.h"
#include <math.h>

// one value under the rule: one IEEE multiplication in the source's precision, round-half-to-even, the clamp on the
// float, then the conversion.  *bad is set for NaN and +-Inf, whose result is unspecified (0 here).
__device__ __forceinline__ uint32_t stage_quantise(float x, float s, float peak, bool* bad) {
  if (!(fabsf(x) <= 3.402823466e+38f)) {
    *bad = true;
    return 0u;
  }
  const float q = rintf(__fmul_rn(x, s));      // a finite x may overflow to +-Inf: the clamp takes it
  return (uint32_t)(q > peak ? peak : (q > 0.f ? q : 0.f));      // -0.0 and every q <= 0 give 0
}
__device__ __forceinline__ uint32_t stage_quantise(double x, double s, double peak, bool* bad) {
  if (!(fabs(x) <= 1.7976931348623157e+308)) {
    *bad = true;
    return 0u;
  }
  const double q = rint(__dmul_rn(x, s));
  return (uint32_t)(q > peak ? peak : (q > 0.0 ? q : 0.0));
}

// the c values of source row r of a frame -> v[0 .. c), the others 0
__device__ __forceinline__ void stage_load(const pcc_attr_stage_frame& fr, int64_t r, int c, double scale, float peak, uint32_t v[4],
                                           bool* bad) {
  v[0] = v[1] = v[2] = v[3] = 0u;
  const int64_t at = r * fr.pitch;
  switch (fr.kind) {
    case PCC_ATTR_SRC_U8: {
      const uint8_t* p = (const uint8_t*)fr.d_src + at;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
        if (ch < c) v[ch] = p[ch];
      break;
    }
    case PCC_ATTR_SRC_U16: {
      const uint16_t* p = (const uint16_t*)fr.d_src + at;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
        if (ch < c) v[ch] = p[ch];
      break;
    }
    case PCC_ATTR_SRC_F32: {
      const float* p = (const float*)fr.d_src + at;
      const float s = (float)scale;      // narrowed once
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
        if (ch < c) v[ch] = stage_quantise(p[ch], s, peak, bad);
      break;
    }
    case PCC_ATTR_SRC_F64: {
      const double* p = (const double*)fr.d_src + at;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
        if (ch < c) v[ch] = stage_quantise(p[ch], scale, (double)peak, bad);
      break;
    }
    default:
      break;
  }
}

// the frame of row r of the call: the last f with offs[f] <= r
__device__ __forceinline__ int stage_frame_of(const int64_t* __restrict__ offs, int n_frames, int64_t r) {
  int lo = 0, hi = n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One kernel, two output modes.  CH == 0: packed, `bpv_float` the width of a float source's values (an integer source
// keeps its own), `perm` not read.  CH > 0: sorted, rows of BPV * CH = 4 or 8 bytes.
template <int BPV, int CH>
__global__ __launch_bounds__(256) void k_attr_stage(const pcc_attr_stage_frame* __restrict__ frames, const int64_t* __restrict__ offs,
                                                    int n_frames, int64_t n, double scale, int bpv_float,
                                                    const uint32_t* __restrict__ perm, void* __restrict__ out,
                                                    int32_t* __restrict__ status) {
  static_assert(CH == 0 || BPV * CH == 4 || BPV * CH == 8, "sorted rows of 4 or 8 bytes");
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t src = CH ? (int64_t)perm[i] : i;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  int c = 0, bpv = BPV;
  int64_t r = -1, out_offset = 0;
  if (src >= n) {
    atomicOr(status, 2);
  } else {
    const int f = stage_frame_of(offs, n_frames, src);
    const pcc_attr_stage_frame fr = frames[f];
    r = src - offs[f];
    const int most = CH ? CH : 4;
    c = fr.channels < 1 ? 1 : (fr.channels > most ? most : fr.channels);
    if (!CH) bpv = fr.kind == PCC_ATTR_SRC_U8 ? 1 : (fr.kind == PCC_ATTR_SRC_U16 ? 2 : bpv_float);
    out_offset = fr.out_offset;
    bool bad = false;
    if (r >= 0) stage_load(fr, r, c, scale, bpv == 1 ? 255.f : 65535.f, v, &bad);
    if (bad) atomicOr(status, 1);
  }
  const uint32_t b4 = (v[0] & 255u) | (v[1] & 255u) << 8 | (v[2] & 255u) << 16 | v[3] << 24;      // four uint8
  const uint32_t lo = (v[0] & 65535u) | v[1] << 16, hi = (v[2] & 65535u) | v[3] << 16;            // four uint16
  if (CH) {      // one store per lane, adjacent across lanes
    if (BPV == 1) ((uint32_t*)out)[i] = b4;
    else if (CH == 2) ((uint32_t*)out)[i] = lo;
    else ((uint64_t*)out)[i] = (uint64_t)lo | (uint64_t)hi << 32;
    return;
  }
  if (r < 0) return;
  // out_offset is 16-aligned, so a row is aligned to its size where that is 2, 4 or 8 bytes
  uint8_t* o = (uint8_t*)out + out_offset + r * (int64_t)(c * bpv);
  if (bpv == 1) {
    if (c == 4) *(uint32_t*)o = b4;
    else if (c == 2) *(uint16_t*)o = (uint16_t)b4;
    else {
      o[0] = (uint8_t)v[0];
      if (c == 3) {
        o[1] = (uint8_t)v[1];
        o[2] = (uint8_t)v[2];
      }
    }
  } else {
    if (c == 4) *(uint64_t*)o = (uint64_t)lo | (uint64_t)hi << 32;
    else if (c == 2) *(uint32_t*)o = lo;
    else {
      uint16_t* o2 = (uint16_t*)o;
      o2[0] = (uint16_t)v[0];
      if (c == 3) {
        o2[1] = (uint16_t)v[1];
        o2[2] = (uint16_t)v[2];
      }
    }
  }
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
extern "C" int pcc_attr_stage_frames(pcc_ctx* ctx, const pcc_attr_stage_frame* h_frames, const pcc_attr_stage_frame* d_frames,
                                     const int64_t* h_row_offsets, const int64_t* d_row_offsets, int n_frames, double scale, int bpv,
                                     int channels, const uint32_t* d_perm, void* d_out, int64_t out_bytes, int32_t* d_status) {
  PCC_REQUIRE(ctx && h_frames && d_frames && h_row_offsets && d_row_offsets && d_status, PCC_E_ARG,
              "pcc_attr_stage_frames: null arrays");
  PCC_REQUIRE(n_frames >= 1 && n_frames <= 65535 && (bpv == 1 || bpv == 2) && out_bytes >= 0 &&
                  (channels == 0 || bpv * channels == 4 || bpv * channels == 8),
              PCC_E_ARG, "pcc_attr_stage_frames: bad argument (n_frames=%d bpv=%d channels=%d out_bytes=%lld)", n_frames, bpv, channels,
              (long long)out_bytes);
  const bool sorted = channels != 0;
  PCC_REQUIRE(h_row_offsets[0] == 0, PCC_E_ARG, "pcc_attr_stage_frames: the row offsets begin at %lld, not 0", (long long)h_row_offsets[0]);
  bool any_float = false;
  int64_t end = 0;      // packed: the byte behind the frames so far
  for (int f = 0; f < n_frames; ++f) {
    const pcc_attr_stage_frame& fr = h_frames[f];
    const int64_t rows = h_row_offsets[f + 1] - h_row_offsets[f];
    PCC_REQUIRE(rows >= 0 && h_row_offsets[f + 1] < ((int64_t)1 << 27), PCC_E_ARG,
                "pcc_attr_stage_frames: frame %d: row offsets %lld .. %lld (ascending, fewer than 2^27 rows)", f,
                (long long)h_row_offsets[f], (long long)h_row_offsets[f + 1]);
    PCC_REQUIRE(fr.kind >= PCC_ATTR_SRC_U8 && fr.kind <= PCC_ATTR_SRC_F64, PCC_E_ARG, "pcc_attr_stage_frames: frame %d: bad source kind %d",
                f, fr.kind);
    PCC_REQUIRE(fr.channels >= 1 && fr.channels <= 4 && (!sorted || fr.channels <= channels), PCC_E_ARG,
                "pcc_attr_stage_frames: frame %d: %d channels (1 .. %d)", f, fr.channels, sorted ? channels : 4);
    PCC_REQUIRE(fr.pitch >= fr.channels, PCC_E_ARG, "pcc_attr_stage_frames: frame %d: pitch %lld below its %d channels", f,
                (long long)fr.pitch, fr.channels);
    const int elem = fr.kind == PCC_ATTR_SRC_U8 ? 1 : (fr.kind == PCC_ATTR_SRC_U16 ? 2 : (fr.kind == PCC_ATTR_SRC_F32 ? 4 : 8));
    PCC_REQUIRE(rows == 0 || (fr.d_src && (uintptr_t)fr.d_src % elem == 0), PCC_E_ARG,
                "pcc_attr_stage_frames: frame %d: null source, or one not aligned to its %d-byte elements", f, elem);
    const bool is_float = fr.kind >= PCC_ATTR_SRC_F32;
    any_float |= is_float;
    const int own = is_float ? bpv : (fr.kind == PCC_ATTR_SRC_U8 ? 1 : 2);
    if (sorted) {
      PCC_REQUIRE(own <= bpv, PCC_E_ARG, "pcc_attr_stage_frames: frame %d: uint16 values into rows of uint8", f);
    } else {
      PCC_REQUIRE(fr.out_offset >= end && fr.out_offset % 16 == 0, PCC_E_ARG,
                  "pcc_attr_stage_frames: frame %d: value offset %lld (16-aligned, behind the frame before it)", f,
                  (long long)fr.out_offset);
      end = fr.out_offset + rows * fr.channels * own;
    }
  }
  const int64_t n = h_row_offsets[n_frames];
  PCC_REQUIRE((sorted ? n * bpv * channels : end) <= out_bytes, PCC_E_ARG, "pcc_attr_stage_frames: %lld bytes of output in a buffer of %lld",
              (long long)(sorted ? n * bpv * channels : end), (long long)out_bytes);
  PCC_REQUIRE(!any_float || (scale > 0.0 && scale <= 1.7976931348623157e+308), PCC_E_ARG,
              "pcc_attr_stage_frames: scale %g must be positive and finite", scale);
  PCC_REQUIRE(n == 0 || (d_out && (uintptr_t)d_out % 16 == 0 && (sorted ? d_perm != nullptr : d_perm == nullptr)), PCC_E_ARG,
              "pcc_attr_stage_frames: null or unaligned output, or a permutation in the wrong mode (sorted takes one, packed none)");
  if (n == 0) return PCC_OK;
  PccProfScope prof(ctx, "attr_stage", n, n_frames, channels, bpv);
  const dim3 grid(nblk(n, 256)), block(256);
  hipStream_t st = ctx->stream;
  if (!sorted)
    hipLaunchKernelGGL((k_attr_stage<0, 0>), grid, block, 0, st, d_frames, d_row_offsets, n_frames, n, scale, bpv, d_perm, d_out, d_status);
  else if (bpv == 1)
    hipLaunchKernelGGL((k_attr_stage<1, 4>), grid, block, 0, st, d_frames, d_row_offsets, n_frames, n, scale, bpv, d_perm, d_out, d_status);
  else if (channels == 2)
    hipLaunchKernelGGL((k_attr_stage<2, 2>), grid, block, 0, st, d_frames, d_row_offsets, n_frames, n, scale, bpv, d_perm, d_out, d_status);
  else
    hipLaunchKernelGGL((k_attr_stage<2, 4>), grid, block, 0, st, d_frames, d_row_offsets, n_frames, n, scale, bpv, d_perm, d_out, d_status);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}
