// entropy.hip — device side of the entropy models: symbol / index formation
// for the factorized bottleneck (z) and the Gaussian conditional (y), and the
// decoder's offset de-quantisation.
//
// Replaces the tensor arithmetic around the CompressAI calls in
//   factorized_model_step_batched  codec_pipeline.py:294-317 / codec_parallel.py:291-318
//   gaussian_model_step_batched    codec_pipeline.py:397-437 / codec_parallel.py:382-419
// Every operation is a single IEEE float32 op (no contraction, no
// transcendental), so encoder, decoder and the CPU oracle derive identical
// integers; the serial rANS itself runs on the host (rans_host.cpp).
// Layouts: features [n,c] row-major; symbols / indexes channel-major [.., c, n]
// (the order CompressAI flattens [B,C,N] in).
#include "common.h"

// thread t -> (ch = t / n, i = t % n): coalesced channel-major writes
__global__ __launch_bounds__(256) void k_factorized_quant(const float* __restrict__ z, int64_t n, int c,
                                                          const float* __restrict__ med,
                                                          int32_t* __restrict__ sym,
                                                          float* __restrict__ zhat) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * c) return;
  const int ch = (int)(t / n);
  const int64_t i = t - (int64_t)ch * n;
  const float m = med[ch];
  const float r = rintf(__fsub_rn(z[i * c + ch], m));
  sym[t] = (int32_t)r;
  zhat[i * c + ch] = __fadd_rn(r, m);
}

__global__ __launch_bounds__(256) void k_factorized_dequant(const int32_t* __restrict__ sym, int64_t n,
                                                            int c, const float* __restrict__ med,
                                                            float* __restrict__ zhat) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * c) return;
  const int ch = (int)(t / n);
  const int64_t i = t - (int64_t)ch * n;
  zhat[i * c + ch] = __fadd_rn((float)sym[t], med[ch]);
}

__device__ __forceinline__ int32_t scale_index(float sc, const float* __restrict__ table, int n_tab) {
  // GaussianConditional.build_indexes: lower-bound at table[0], then
  // idx = (n_tab-1) - #{t in table[:-1] : scale <= t}
  const float s = fmaxf(sc, table[0]);
  int32_t idx = n_tab - 1;
  for (int j = 0; j < n_tab - 1; ++j) idx -= (s <= table[j]) ? 1 : 0;
  return idx;
}

// The Gaussian stage reads row-major tensors (y [N, C], params [N, 2C]: what the layers write) and writes channel-major
// symbol arrays ([C, N]: the order the reference's coder reads, codec_pipeline.py:397-437) — a transposition.  One thread
// per output element read its inputs with a stride of C (128 / 256 B): every lane its own cache line, 48 us for 844k x 3
// symbols (now 17; the de-quantiser 37 -> 9).  Here a workgroup stages GQ_TILE rows through LDS: coalesced reads of the rows, coalesced writes of GQ_TILE
// consecutive positions of every channel (pitch C + 1: conflict-free both ways).  The arithmetic per element is unchanged.
constexpr int GQ_TILE = 16;    // 26k latent rows -> 1650 workgroups (64 rows: 412, 2.1x slower; 8 rows: 6 % slower)
constexpr int GQ_MAX_C = 256;  // three [GQ_TILE][C + 1] float planes within 64 KB of LDS
static inline size_t gq_lds_bytes(int c, int planes) { return (size_t)(64 + planes * GQ_TILE * (c + 1)) * 4; }

// stage `rows` rows of a row-major [*, width] tensor, columns [col0, col0 + c), into dst[r * (c + 1) + ch]: wave w takes
// rows w, w + 4, ..., its lanes the columns (no division by a run-time width)
__device__ __forceinline__ void gq_stage(const float* __restrict__ src, int64_t row0, int rows, int width, int col0, int c,
                                         float* __restrict__ dst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int r = wave; r < rows; r += nw) {
    const float* row = src + (row0 + r) * width + col0;
    for (int j = lane; j < c; j += 64) dst[r * (c + 1) + j] = row[j];
  }
}

// The scale table in LDS and whether it ascends (every table a CompressAI model builds does: exp(linspace)): then the
// count of build_indexes is a lower bound — six probes instead of 63 comparisons.  Block-uniform.
__device__ __forceinline__ bool gq_load_table(const float* __restrict__ table, int n_tab, float* __restrict__ tab) {
  if (threadIdx.x < n_tab) tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const bool ok = !((int)threadIdx.x + 1 < n_tab) || tab[threadIdx.x] <= tab[threadIdx.x + 1];
  return __syncthreads_and(ok) != 0;
}
__device__ __forceinline__ int32_t scale_index_fast(float sc, const float* __restrict__ tab, int n_tab, bool ascending) {
  if (!ascending) return scale_index(sc, tab, n_tab);
  // idx = (n_tab - 1) - #{j < n_tab - 1 : s <= tab[j]} = the first j in [0, n_tab - 1] with tab[j] >= s (n_tab - 1 if none)
  const float s = fmaxf(sc, tab[0]);
  int lo = 0, hi = n_tab - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] >= s) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// SymT / IdxT: int32 / int32 (generic), int16 / uint8 with the int16 overflow flag (what crosses PCIe to the host
// coders), int32 / uint8 (what the GPU coder reads)
template <typename SymT, typename IdxT, bool CHECK16>
__global__ __launch_bounds__(256) void k_gaussian_quant_t(
    const float* __restrict__ y, const float* __restrict__ params, int64_t n, int c,
    const float* __restrict__ scale, int nq, const float* __restrict__ table, int n_tab,
    SymT* __restrict__ sym, IdxT* __restrict__ idx, int32_t* __restrict__ flag) {
  extern __shared__ float gq_lds[];
  float* tab = gq_lds;
  float* yt = gq_lds + 64;
  float* sct = yt + GQ_TILE * (c + 1);
  float* mut = sct + GQ_TILE * (c + 1);
  const bool asc = gq_load_table(table, n_tab, tab);
  const int64_t row0 = (int64_t)blockIdx.x * GQ_TILE;
  const int rows = (int)min((int64_t)GQ_TILE, n - row0);
  gq_stage(y, row0, rows, c, 0, c, yt);
  gq_stage(params, row0, rows, 2 * c, 0, c, sct);
  gq_stage(params, row0, rows, 2 * c, c, c, mut);
  __syncthreads();
  bool over = false;
  for (int e = threadIdx.x; e < GQ_TILE * c; e += blockDim.x) {
    const int ch = e / GQ_TILE, r = e - ch * GQ_TILE;
    if (r >= rows) continue;
    const float yv = yt[r * (c + 1) + ch], sc = sct[r * (c + 1) + ch], mu = mut[r * (c + 1) + ch];
    const int64_t t = (int64_t)ch * n + row0 + r;
    for (int q = 0; q < nq; ++q) {
      const float s = scale[q * c + ch];
      const float v = rintf(__fsub_rn(__fmul_rn(yv, s), __fmul_rn(mu, s)));
      if constexpr (CHECK16) over |= !(v >= -32768.0f && v <= 32767.0f);
      sym[(int64_t)q * n * c + t] = (SymT)(int32_t)v;
      idx[(int64_t)q * n * c + t] = (IdxT)scale_index_fast(__fmul_rn(sc, s), tab, n_tab, asc);
    }
  }
  if constexpr (CHECK16)
    if (over) atomicOr(flag, 1);
}

template <typename IdxT>
__global__ __launch_bounds__(256) void k_gaussian_indexes_t(const float* __restrict__ params, int64_t n, int c,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ table, int n_tab,
                                                            IdxT* __restrict__ idx) {
  extern __shared__ float gq_lds[];
  float* tab = gq_lds;
  float* sct = gq_lds + 64;
  const bool asc = gq_load_table(table, n_tab, tab);
  const int64_t row0 = (int64_t)blockIdx.x * GQ_TILE;
  const int rows = (int)min((int64_t)GQ_TILE, n - row0);
  gq_stage(params, row0, rows, 2 * c, 0, c, sct);
  __syncthreads();
  for (int e = threadIdx.x; e < GQ_TILE * c; e += blockDim.x) {
    const int ch = e / GQ_TILE, r = e - ch * GQ_TILE;
    if (r >= rows) continue;
    idx[(int64_t)ch * n + row0 + r] = (IdxT)scale_index_fast(__fmul_rn(sct[r * (c + 1) + ch], scale[ch]), tab, n_tab, asc);
  }
}

// the way back: channel-major symbols + row-major params -> row-major y_hat
__global__ __launch_bounds__(256) void k_gaussian_dequant(const int32_t* __restrict__ sym,
                                                          const float* __restrict__ params, int64_t n,
                                                          int c, const float* __restrict__ scale,
                                                          float bound, float off_a, float off_b,
                                                          float* __restrict__ yhat) {
  extern __shared__ float gq_lds[];
  float* sct = gq_lds + 64;
  float* mut = sct + GQ_TILE * (c + 1);
  float* out = mut + GQ_TILE * (c + 1);
  const int64_t row0 = (int64_t)blockIdx.x * GQ_TILE;
  const int rows = (int)min((int64_t)GQ_TILE, n - row0);
  gq_stage(params, row0, rows, 2 * c, 0, c, sct);
  gq_stage(params, row0, rows, 2 * c, c, c, mut);
  __syncthreads();
  for (int e = threadIdx.x; e < GQ_TILE * c; e += blockDim.x) {
    const int ch = e / GQ_TILE, r = e - ch * GQ_TILE;
    if (r >= rows) continue;
    const float s = scale[ch];
    const float rescale = __fdiv_rn(1.0f, s);
    const float sigma = fmaxf(__fmul_rn(sct[r * (c + 1) + ch], s), bound);
    const float mu = mut[r * (c + 1) + ch];
    const int32_t q = sym[(int64_t)ch * n + row0 + r];
    const float q_abs = fabsf((float)q);
    const float sign = (q > 0) ? 1.0f : ((q < 0) ? -1.0f : 0.0f);
    // get_offsets(sigma, scale) := off_a / (off_b + sigma); applied negated, zero for the zero bin
    float q_off = -__fdiv_rn(off_a, __fadd_rn(off_b, sigma));
    if (q_abs < 0.0001f) q_off = 0.0f;
    const float v = __fmul_rn(sign, __fadd_rn(q_abs, q_off));
    out[r * (c + 1) + ch] = __fadd_rn(__fmul_rn(v, rescale), mu);
  }
  __syncthreads();
  float* dst = yhat + row0 * c;
  for (int e = threadIdx.x; e < rows * c; e += blockDim.x) {
    const int r = e / c, ch = e - r * c;
    dst[e] = out[r * (c + 1) + ch];
  }
}

// ---- element-wise forms behind the CompressAI-shaped methods (any tensor shape, flat) --------
__global__ __launch_bounds__(256) void k_build_indexes(const float* __restrict__ scales, int64_t n,
                                                       const float* __restrict__ table, int n_tab,
                                                       int32_t* __restrict__ idx) {
  __shared__ float tab[64];
  if (threadIdx.x < n_tab) tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) idx[t] = scale_index(scales[t], tab, n_tab);
}

__global__ __launch_bounds__(256) void k_quantize_symbols(const float* __restrict__ x,
                                                          const float* __restrict__ means /*nullable*/,
                                                          int64_t n, int32_t* __restrict__ sym) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float v = means ? __fsub_rn(x[t], means[t]) : x[t];
  sym[t] = (int32_t)rintf(v);
}

extern "C" int pcc_build_indexes(pcc_ctx* ctx, const float* d_scales, int64_t n, const float* d_table,
                                 int n_tab, int32_t* d_idx) {
  PCC_REQUIRE(ctx && n_tab >= 2 && n_tab <= 64, PCC_E_ARG, "pcc_build_indexes: bad arg");
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_scales && d_table && d_idx, PCC_E_ARG, "pcc_build_indexes: null buffers");
  hipLaunchKernelGGL(k_build_indexes, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, d_scales, n, d_table,
                     n_tab, d_idx);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_quantize_symbols(pcc_ctx* ctx, const float* d_x, const float* d_means, int64_t n,
                                    int32_t* d_sym) {
  PCC_REQUIRE(ctx, PCC_E_ARG, "pcc_quantize_symbols: null ctx");
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_x && d_sym, PCC_E_ARG, "pcc_quantize_symbols: null buffers");
  hipLaunchKernelGGL(k_quantize_symbols, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, d_x, d_means, n, d_sym);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_factorized_quant(pcc_ctx* ctx, const float* d_z, int64_t n, int c,
                                    const float* d_med, int32_t* d_sym, float* d_zhat) {
  PCC_REQUIRE(ctx && c >= 1, PCC_E_ARG, "pcc_factorized_quant: bad arg");
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_z && d_med && d_sym && d_zhat, PCC_E_ARG, "pcc_factorized_quant: null buffers");
  hipLaunchKernelGGL(k_factorized_quant, dim3(nblk(n * c, 256)), dim3(256), 0, ctx->stream, d_z, n, c,
                     d_med, d_sym, d_zhat);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_factorized_dequant(pcc_ctx* ctx, const int32_t* d_sym, int64_t n, int c,
                                      const float* d_med, float* d_zhat) {
  PCC_REQUIRE(ctx && c >= 1, PCC_E_ARG, "pcc_factorized_dequant: bad arg");
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_sym && d_med && d_zhat, PCC_E_ARG, "pcc_factorized_dequant: null buffers");
  hipLaunchKernelGGL(k_factorized_dequant, dim3(nblk(n * c, 256)), dim3(256), 0, ctx->stream, d_sym, n,
                     c, d_med, d_zhat);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_gaussian_quant(pcc_ctx* ctx, const float* d_y, const float* d_params, int64_t n,
                                  int c, const float* d_scale, int q, const float* d_table, int n_tab,
                                  int32_t* d_sym, int32_t* d_idx) {
  PCC_REQUIRE(ctx && c >= 1 && c <= GQ_MAX_C && q >= 1 && n_tab >= 2 && n_tab <= 64, PCC_E_ARG,
              "pcc_gaussian_quant: bad arg (c=%d q=%d n_tab=%d)", c, q, n_tab);
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_y && d_params && d_scale && d_table && d_sym && d_idx, PCC_E_ARG,
              "pcc_gaussian_quant: null buffers");
  hipLaunchKernelGGL((k_gaussian_quant_t<int32_t, int32_t, false>), dim3(nblk(n, GQ_TILE)), dim3(256), gq_lds_bytes(c, 3),
                     ctx->stream, d_y, d_params, n, c, d_scale, q, d_table, n_tab, d_sym, d_idx, (int32_t*)nullptr);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_gaussian_quant16(pcc_ctx* ctx, const float* d_y, const float* d_params, int64_t n,
                                    int c, const float* d_scale, int q, const float* d_table, int n_tab,
                                    int16_t* d_sym, uint8_t* d_idx, int32_t* d_flag) {
  PCC_REQUIRE(ctx && c >= 1 && c <= GQ_MAX_C && q >= 1 && n_tab >= 2 && n_tab <= 64, PCC_E_ARG,
              "pcc_gaussian_quant16: bad arg (c=%d q=%d n_tab=%d)", c, q, n_tab);
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_y && d_params && d_scale && d_table && d_sym && d_idx && d_flag, PCC_E_ARG,
              "pcc_gaussian_quant16: null buffers");
  hipLaunchKernelGGL((k_gaussian_quant_t<int16_t, uint8_t, true>), dim3(nblk(n, GQ_TILE)), dim3(256), gq_lds_bytes(c, 3),
                     ctx->stream, d_y, d_params, n, c, d_scale, q, d_table, n_tab, d_sym, d_idx, d_flag);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_gaussian_quant_dev(pcc_ctx* ctx, const float* d_y, const float* d_params, int64_t n, int c,
                                      const float* d_scale, int q, const float* d_table, int n_tab, int32_t* d_sym,
                                      uint8_t* d_idx) {
  PCC_REQUIRE(ctx && c >= 1 && c <= GQ_MAX_C && q >= 1 && n_tab >= 2 && n_tab <= 64, PCC_E_ARG,
              "pcc_gaussian_quant_dev: bad arg (c=%d q=%d n_tab=%d)", c, q, n_tab);
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_y && d_params && d_scale && d_table && d_sym && d_idx, PCC_E_ARG, "pcc_gaussian_quant_dev: null buffers");
  hipLaunchKernelGGL((k_gaussian_quant_t<int32_t, uint8_t, false>), dim3(nblk(n, GQ_TILE)), dim3(256), gq_lds_bytes(c, 3),
                     ctx->stream, d_y, d_params, n, c, d_scale, q, d_table, n_tab, d_sym, d_idx, (int32_t*)nullptr);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_gaussian_indexes8(pcc_ctx* ctx, const float* d_params, int64_t n, int c,
                                     const float* d_scale, const float* d_table, int n_tab,
                                     uint8_t* d_idx) {
  PCC_REQUIRE(ctx && c >= 1 && c <= GQ_MAX_C && n_tab >= 2 && n_tab <= 64, PCC_E_ARG, "pcc_gaussian_indexes8: bad arg");
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_params && d_scale && d_table && d_idx, PCC_E_ARG, "pcc_gaussian_indexes8: null buffers");
  hipLaunchKernelGGL((k_gaussian_indexes_t<uint8_t>), dim3(nblk(n, GQ_TILE)), dim3(256), gq_lds_bytes(c, 1), ctx->stream,
                     d_params, n, c, d_scale, d_table, n_tab, d_idx);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_gaussian_indexes(pcc_ctx* ctx, const float* d_params, int64_t n, int c,
                                    const float* d_scale, const float* d_table, int n_tab,
                                    int32_t* d_idx) {
  PCC_REQUIRE(ctx && c >= 1 && c <= GQ_MAX_C && n_tab >= 2 && n_tab <= 64, PCC_E_ARG, "pcc_gaussian_indexes: bad arg");
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_params && d_scale && d_table && d_idx, PCC_E_ARG, "pcc_gaussian_indexes: null buffers");
  hipLaunchKernelGGL((k_gaussian_indexes_t<int32_t>), dim3(nblk(n, GQ_TILE)), dim3(256), gq_lds_bytes(c, 1), ctx->stream,
                     d_params, n, c, d_scale, d_table, n_tab, d_idx);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_gaussian_dequant(pcc_ctx* ctx, const int32_t* d_sym, const float* d_params,
                                    int64_t n, int c, const float* d_scale, float bound, float off_a,
                                    float off_b, float* d_yhat) {
  PCC_REQUIRE(ctx && c >= 1 && c <= GQ_MAX_C, PCC_E_ARG, "pcc_gaussian_dequant: bad arg");
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(d_sym && d_params && d_scale && d_yhat, PCC_E_ARG, "pcc_gaussian_dequant: null buffers");
  hipLaunchKernelGGL(k_gaussian_dequant, dim3(nblk(n, GQ_TILE)), dim3(256), gq_lds_bytes(c, 3), ctx->stream, d_sym,
                     d_params, n, c, d_scale, bound, off_a, off_b, d_yhat);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}
