// knn.hip — the k nearest neighbours of every point of a frame among the frame's own points, the scatter matrix of
// that neighbourhood and its surface normal.  include/pcc.h has the rules; tests/normals_ref.py restates them in numpy.
// (The D2 projection onto these normals consumes a 1-NN pairing and lives beside that search, in nn.hip.)
//
// k_knn_frames is the k-best form of nn.hip's search: one thread per query walks the cells of its own frame in row
// order with nn_walk (nn_cells.h has the walk and why it ends).
//
//   list   the k best (d2, row) so far, ascending by (d2, row), in registers: a capacity template (8 / 16 / 32, chosen
//          by the host from k) whose insertion is fully unrolled, so every index is static and nothing lives in
//          scratch (DESIGN.md 6c has the figures).  The list sits at the END of the capacity: the CAP - k slots in
//          front hold (0, -1), below every candidate, so the pruning bound is always the last slot.  Free slots hold
//          (2^64 - 1, INT32_MAX): until the list holds k_eff = min(k, frame rows) entries nothing is pruned.
//   seed   the k_eff rows around the query's place in key order, clamped to the frame's rows, fill the list before the
//          walk starts; the walk passes over them (seeded), so no row enters twice.  The seed loop counts k_eff rows.
//   host   knn_with_cap picks the capacity for every launch and replay of this file, knn_entry is what every entry on
//          one key array does in front of its launches, knn_host_frames the replays' walk over the frames.
//
// Epilogue, same thread: C = m sum d d^T - (sum d)(sum d)^T over the m = k_eff neighbours in int64 (below 2^46), then
// a unit eigenvector of its smallest eigenvalue in float64 — eigenvalues in closed form (trigonometric), the vector
// of the better separated end from the largest cross product of two rows of C - lambda I, the other end inside that
// vector's orthogonal complement (a 2 x 2 problem), so a double eigenvalue at the small end still gives a vector of
// its eigenspace — and the flip towards a viewpoint.
#include "common.h"
#include "nn_cells.h"
#include <algorithm>
#include <math.h>
#include <type_traits>
#include <vector>

#define KNN_NO_DIST (~0ull)
#define KNN_NO_ROW 0x7FFFFFFF

// ---------------------------------------------------------------- the list
template <int CAP>
struct KnnList {
  uint64_t d[CAP];
  int32_t r[CAP];
};

__host__ __device__ static inline bool knn_less(uint64_t d, int32_t r, uint64_t d1, int32_t r1) {
  return d < d1 || (d == d1 && r < r1);
}

template <int CAP>
__host__ __device__ static inline void knn_init(KnnList<CAP>& L, int k) {
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    const bool live = j >= CAP - k;
    L.d[j] = live ? KNN_NO_DIST : 0ull;
    L.r[j] = live ? KNN_NO_ROW : -1;
  }
}

// (d, r) into its place if it is below the last slot; what was last falls out.  Slot j takes slot j - 1's entry where
// the new one belongs in front of j - 1, the new one where it belongs in front of j only: selects on static indexes.
template <int CAP>
__host__ __device__ static inline void knn_insert(KnnList<CAP>& L, uint64_t d, int32_t r) {
  bool before = knn_less(d, r, L.d[CAP - 1], L.r[CAP - 1]);      // in front of slot j
  if (!before) return;
#pragma unroll
  for (int j = CAP - 1; j >= 1; --j) {
    const bool before_prev = knn_less(d, r, L.d[j - 1], L.r[j - 1]);
    L.d[j] = before_prev ? L.d[j - 1] : (before ? d : L.d[j]);
    L.r[j] = before_prev ? L.r[j - 1] : (before ? r : L.r[j]);
    before = before_prev;
  }
  if (before) {
    L.d[0] = d;
    L.r[0] = r;
  }
}

// the k-NN bound of nn_walk: the list's last slot; the seed rows [s0, s1) are in the list already.  CAPPED (the radius
// search): never beyond cap = radius2 + 1, and at the cap no row wins a tie (bound_row -1): a cell at box distance
// radius2 + 1 holds no point within the radius.  Not CAPPED: cap is not read, and a last slot that is still free
// answers (2^64 - 1, KNN_NO_ROW) by itself.
template <int CAP, bool CAPPED>
struct KnnBest {
  KnnList<CAP>& L;
  int64_t s0, s1;
  uint64_t cap;
  __host__ __device__ bool below_cap() const { return !CAPPED || L.d[CAP - 1] < cap; }
  __host__ __device__ uint64_t bound() const { return below_cap() ? L.d[CAP - 1] : cap; }
  __host__ __device__ int64_t bound_row() const { return below_cap() ? (int64_t)L.r[CAP - 1] : -1; }
  __host__ __device__ bool seeded(int64_t r) const { return r >= s0 && r < s1; }
  __host__ __device__ void offer(uint64_t d, int64_t r) { knn_insert(L, d, (int32_t)r); }
};

// the k-best search of one query among the rows [flo, fhi) of its frame, flo < fhi, 1 <= k <= CAP; L comes from
// knn_init.  Returns the nodes tried (cells tested and points measured, the seeds included).
template <int CAP>
__host__ __device__ static inline uint32_t knn_search(const uint64_t* __restrict__ keys, int64_t flo, int64_t fhi, uint64_t qk,
                                                      int k, KnnList<CAP>& L) {
  const uint32_t qx = pcc_compact3(qk >> 2), qy = pcc_compact3(qk >> 1), qz = pcc_compact3(qk);
  const int64_t n_f = fhi - flo;
  const int64_t k_eff = n_f < k ? n_f : k;
  const int64_t lo = nn_lower_bound(keys, flo, fhi, qk);      // the first row of the frame whose key is not below the query's
  int64_t s0 = lo - k_eff / 2;      // the seed rows [s0, s1) inside [flo, fhi)
  if (s0 > fhi - k_eff) s0 = fhi - k_eff;
  if (s0 < flo) s0 = flo;
  KnnBest<CAP, false> b = {L, s0, s0 + k_eff, 0};
  for (int64_t r = b.s0; r < b.s1; ++r) knn_insert(L, nn_d2(qx, qy, qz, keys[r]), (int32_t)r);
  if (k_eff == n_f) return (uint32_t)k_eff;      // the seed was the whole frame
  return (uint32_t)k_eff + nn_walk(keys, flo, fhi, qx, qy, qz, b);
}

// ---------------------------------------------------------------- scatter matrix and normal
// C = m sum d d^T - (sum d)(sum d)^T over the list's m entries, d = neighbour - query: xx, xy, xz, yy, yz, zz
template <int CAP>
__host__ __device__ static inline void knn_cov(const uint64_t* __restrict__ keys, const KnnList<CAP>& L, int k, uint64_t qk,
                                               int64_t c[6]) {
  const int64_t qx = pcc_compact3(qk >> 2), qy = pcc_compact3(qk >> 1), qz = pcc_compact3(qk);
  int64_t m = 0, sx = 0, sy = 0, sz = 0, xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    if (j >= CAP - k && L.d[j] != KNN_NO_DIST) {
      const uint64_t key = keys[L.r[j]];
      const int64_t dx = (int64_t)pcc_compact3(key >> 2) - qx, dy = (int64_t)pcc_compact3(key >> 1) - qy,
                    dz = (int64_t)pcc_compact3(key) - qz;
      ++m;
      sx += dx; sy += dy; sz += dz;
      xx += dx * dx; xy += dx * dy; xz += dx * dz;
      yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
  }
  c[0] = m * xx - sx * sx; c[1] = m * xy - sx * sy; c[2] = m * xz - sx * sz;
  c[3] = m * yy - sy * sy; c[4] = m * yz - sy * sz; c[5] = m * zz - sz * sz;
}

struct KnnV3 {
  double x, y, z;
};
__host__ __device__ static inline KnnV3 knn_cross(KnnV3 a, KnnV3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__host__ __device__ static inline double knn_dot(KnnV3 a, KnnV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

struct KnnSym3 {
  double a00, a01, a02, a11, a12, a22;
};
__host__ __device__ static inline KnnV3 knn_mul(const KnnSym3& a, KnnV3 v) {
  return {(a.a00 * v.x + a.a01 * v.y) + a.a02 * v.z, (a.a01 * v.x + a.a11 * v.y) + a.a12 * v.z,
          (a.a02 * v.x + a.a12 * v.y) + a.a22 * v.z};
}

// a unit vector of the null space of A - lambda I where that matrix has rank 2 (lambda the better separated end of
// the spectrum): the largest cross product of two of its rows
__host__ __device__ static inline KnnV3 knn_evec_rank2(const KnnSym3& a, double lambda) {
  const KnnV3 r0 = {a.a00 - lambda, a.a01, a.a02}, r1 = {a.a01, a.a11 - lambda, a.a12}, r2 = {a.a02, a.a12, a.a22 - lambda};
  const KnnV3 c01 = knn_cross(r0, r1), c02 = knn_cross(r0, r2), c12 = knn_cross(r1, r2);
  const double d01 = knn_dot(c01, c01), d02 = knn_dot(c02, c02), d12 = knn_dot(c12, c12);
  KnnV3 v = c01;
  double d = d01;
  if (d02 > d) { v = c02; d = d02; }
  if (d12 > d) { v = c12; d = d12; }
  if (!(d > 0.0)) return {1.0, 0.0, 0.0};      // rank <= 1 after all: the caller's complement step still works on it
  const double s = 1.0 / sqrt(d);
  return {v.x * s, v.y * s, v.z * s};
}

// a unit eigenvector of A for lambda inside the orthogonal complement of the unit eigenvector e: the null vector of
// the 2 x 2 matrix (U V)^T (A - lambda I) (U V), taken from its larger row
__host__ __device__ static inline KnnV3 knn_evec_in_complement(const KnnSym3& a, KnnV3 e, double lambda) {
  KnnV3 u;
  if (fabs(e.x) > fabs(e.y)) {
    const double s = 1.0 / sqrt(e.x * e.x + e.z * e.z);
    u = {-e.z * s, 0.0, e.x * s};
  } else {
    const double s = 1.0 / sqrt(e.y * e.y + e.z * e.z);
    u = {0.0, e.z * s, -e.y * s};
  }
  const KnnV3 v = knn_cross(e, u);
  const KnnV3 au = knn_mul(a, u), av = knn_mul(a, v);
  double m00 = knn_dot(u, au) - lambda, m01 = knn_dot(u, av), m11 = knn_dot(v, av) - lambda;
  const double b00 = fabs(m00), b01 = fabs(m01), b11 = fabs(m11);
  double cu, cv;      // the result is cu U + cv V
  if (b00 >= b11) {
    if (!((b00 > b01 ? b00 : b01) > 0.0)) return u;
    if (b00 >= b01) {
      m01 /= m00; m00 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m00;
    } else {
      m00 /= m01; m01 = 1.0 / sqrt(1.0 + m00 * m00); m00 *= m01;
    }
    cu = m01; cv = -m00;
  } else {
    if (!((b11 > b01 ? b11 : b01) > 0.0)) return u;
    if (b11 >= b01) {
      m01 /= m11; m11 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m11;
    } else {
      m11 /= m01; m01 = 1.0 / sqrt(1.0 + m11 * m11); m11 *= m01;
    }
    cu = m11; cv = -m01;
  }
  return {cu * u.x + cv * v.x, cu * u.y + cv * v.y, cu * u.z + cv * v.z};
}

// a unit eigenvector of the symmetric matrix c (xx, xy, xz, yy, yz, zz; integers below 2^46, exact in float64) for
// its smallest eigenvalue; always finite, (0, 0, 1) for c = 0
__host__ __device__ static inline KnnV3 knn_normal(const int64_t c[6]) {
  KnnSym3 a = {(double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4], (double)c[5]};
  double top = fabs(a.a00);
  top = fabs(a.a01) > top ? fabs(a.a01) : top;
  top = fabs(a.a02) > top ? fabs(a.a02) : top;
  top = fabs(a.a11) > top ? fabs(a.a11) : top;
  top = fabs(a.a12) > top ? fabs(a.a12) : top;
  top = fabs(a.a22) > top ? fabs(a.a22) : top;
  if (!(top > 0.0)) return {0.0, 0.0, 1.0};
  const double inv = 1.0 / top;
  a.a00 *= inv; a.a01 *= inv; a.a02 *= inv; a.a11 *= inv; a.a12 *= inv; a.a22 *= inv;
  const double off = (a.a01 * a.a01 + a.a02 * a.a02) + a.a12 * a.a12;
  KnnV3 n;
  if (!(off > 0.0)) {      // diagonal: the axis of the smallest entry
    if (a.a00 <= a.a11 && a.a00 <= a.a22) n = {1.0, 0.0, 0.0};
    else if (a.a11 <= a.a22) n = {0.0, 1.0, 0.0};
    else n = {0.0, 0.0, 1.0};
    return n;
  }
  const double q = ((a.a00 + a.a11) + a.a22) / 3.0;
  const double b00 = a.a00 - q, b11 = a.a11 - q, b22 = a.a22 - q;
  const double p = sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + 2.0 * off) / 6.0);
  const double c00 = b11 * b22 - a.a12 * a.a12, c01 = a.a01 * b22 - a.a12 * a.a02, c02 = a.a01 * a.a12 - b11 * a.a02;
  double half_det = ((b00 * c00 - a.a01 * c01) + a.a02 * c02) / (p * p * p) * 0.5;
  half_det = half_det < -1.0 ? -1.0 : (half_det > 1.0 ? 1.0 : half_det);
  const double angle = acos(half_det) / 3.0;
  const double beta2 = 2.0 * cos(angle), beta0 = 2.0 * cos(angle + 2.0943951023931954923), beta1 = -(beta0 + beta2);
  const double ev0 = q + p * beta0, ev1 = q + p * beta1, ev2 = q + p * beta2;      // ascending
  if (half_det >= 0.0) {      // the largest eigenvalue is the better separated one
    const KnnV3 e2 = knn_evec_rank2(a, ev2);
    const KnnV3 e1 = knn_evec_in_complement(a, e2, ev1);
    n = knn_cross(e1, e2);
  } else {
    n = knn_evec_rank2(a, ev0);
  }
  const double len2 = knn_dot(n, n);
  if (!(len2 > 0.0) || !(len2 < 4.0)) return {0.0, 0.0, 1.0};      // never taken by a finite matrix; keeps the promise
  const double s = 1.0 / sqrt(len2);
  return {n.x * s, n.y * s, n.z * s};
}

// everything of one query: search, then the outputs asked for (each pointer nullable, indexed by the query's row i)
template <int CAP>
__host__ __device__ static inline uint32_t knn_point(const uint64_t* __restrict__ keys, int64_t flo, int64_t fhi, int64_t i, int k,
                                                     int32_t* __restrict__ rows, uint64_t* __restrict__ sqdist,
                                                     int64_t* __restrict__ cov, float* __restrict__ normals, bool has_vp, int vx,
                                                     int vy, int vz) {
  const uint64_t qk = keys[i];
  KnnList<CAP> L;
  knn_init(L, k);
  const uint32_t nodes = knn_search(keys, flo, fhi, qk, k, L);
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    if (j >= CAP - k) {
      const int64_t at = i * k + (j - (CAP - k));
      if (rows) rows[at] = L.d[j] == KNN_NO_DIST ? -1 : L.r[j];
      if (sqdist) sqdist[at] = L.d[j];
    }
  }
  if (!cov && !normals) return nodes;
  int64_t c[6] = {0, 0, 0, 0, 0, 0};
  const bool has_normal = fhi - flo >= 3;      // fewer than 3 distinct points: no normal, C = 0
  if (has_normal) knn_cov(keys, L, k, qk, c);
  if (cov) {
#pragma unroll
    for (int j = 0; j < 6; ++j) cov[i * 6 + j] = c[j];
  }
  if (normals) {
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (has_normal) {
      const KnnV3 n = knn_normal(c);
      nx = (float)n.x; ny = (float)n.y; nz = (float)n.z;
      if (has_vp) {      // towards the viewpoint: flipped where n . (viewpoint - p) < 0, on the float32 values returned
        const double ex = (double)(vx - ((int)pcc_compact3(qk >> 2) - 32768)), ey = (double)(vy - ((int)pcc_compact3(qk >> 1) - 32768)),
                     ez = (double)(vz - ((int)pcc_compact3(qk) - 32768));
        if ((ex * (double)nx + ey * (double)ny) + ez * (double)nz < 0.0) {
          nx = -nx; ny = -ny; nz = -nz;
        }
      }
    }
    normals[i * 3] = nx;
    normals[i * 3 + 1] = ny;
    normals[i * 3 + 2] = nz;
  }
  return nodes;
}

template <int CAP>
__global__ __launch_bounds__(256) void k_knn_frames(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ offs,
                                                    int k, int32_t* __restrict__ rows, uint64_t* __restrict__ sqdist,
                                                    int64_t* __restrict__ cov, float* __restrict__ normals, int has_vp, int vx,
                                                    int vy, int vz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(keys[i] >> 48);      // below n_frames: k_nn_check
  const int64_t flo = offs[f], fhi = offs[f + 1];      // flo <= i < fhi: row i is a row of its own frame
  (void)knn_point<CAP>(keys, flo, fhi, i, k, rows, sqdist, cov, normals, has_vp != 0, vx, vy, vz);
}

// ---------------------------------------------------------------- what the entries and the replays share
// the capacity of a list of `len` entries (k, or m + 1 under the radius rule): fn(std::integral_constant<int, CAP>),
// CAP the smallest of 8 / 16 / 32 that holds it
template <typename Fn>
static inline void knn_with_cap(int len, Fn fn) {
  if (len <= 8) fn(std::integral_constant<int, 8>());
  else if (len <= 16) fn(std::integral_constant<int, 16>());
  else fn(std::integral_constant<int, 32>());
}

// What an entry on one key array does in front of its launches, in the order of its refusals (nn_cells.h declares it
// and its two records for cluster.hip): the ranges of the call and of the rule's integer k, the null pointers (the
// keys, then the entry's own), the per-frame output d_frame (nullable) zeroed, frame_bytes a frame, and for n > 0 the
// arena (reserve: the bytes of the whole call, 0: what the checks take) and the key checks.  *offs: the first row of
// every frame; nullptr for n == 0, nothing to do.
int knn_entry(pcc_ctx* ctx, const char* who, KnnRange k, const uint64_t* d_keys, int64_t n, int n_frames, KnnNulls nulls,
              void* d_frame, size_t frame_bytes, size_t reserve, const int64_t** offs) {
  const bool call_ok = ctx && n >= 0 && n <= NN_MAX_KEYS && n_frames >= 1 && n_frames <= 65535;
  if (k.name)
    PCC_REQUIRE(call_ok && k.v >= k.lo && k.v <= k.hi, PCC_E_ARG,
                "%s: bad argument (n=%lld n_frames=%d %s=%d; %s in %d .. %d, at most 2^27 keys, 1 .. 65535 frames)", who, (long long)n,
                n_frames, k.name, k.v, k.name, k.lo, k.hi);
  else
    PCC_REQUIRE(call_ok, PCC_E_ARG, "%s: bad argument (n=%lld n_frames=%d; at most 2^27 keys, 1 .. 65535 frames)", who, (long long)n,
                n_frames);
  PCC_REQUIRE(n == 0 || d_keys, PCC_E_ARG, "%s: %s", who, nulls.keys);
  PCC_REQUIRE(nulls.others_ok, PCC_E_ARG, "%s: %s", who, nulls.others);
  *offs = nullptr;
  if (n > 0) {
    if (reserve) PCC_TRY(pcc_arena_reserve(ctx, reserve));
    PCC_TRY(nn_check_and_offsets(ctx, who, "a key's", "keys", d_keys, n, nullptr, 0, n_frames, offs));
  }
  if (d_frame) PCC_HIP(hipMemsetAsync(d_frame, 0, (size_t)n_frames * frame_bytes, ctx->stream));
  return PCC_OK;
}

// host: the refusal of a frame index that is not below n_frames (65536: every index is); behind it ready(), where a
// replay zeroes and sizes what it fills; then the frames of the sorted keys one after the other, body(f, flo, fhi) for
// the rows [flo, fhi) of frame f
template <typename Ready, typename Body>
static int knn_host_frames(const char* who, const uint64_t* h_keys, int64_t n, int n_frames, Ready ready, Body body) {
  PCC_REQUIRE(n == 0 || (int)(h_keys[n - 1] >> 48) < n_frames, PCC_E_RANGE, "%s: a key's frame index is not below n_frames=%d", who,
              n_frames);
  ready();
  int64_t flo = 0;
  while (flo < n) {
    const uint64_t frame = h_keys[flo] & ~NN_KEY48;
    const int64_t fhi = std::upper_bound(h_keys + flo, h_keys + n, frame | NN_KEY48) - h_keys;
    body((int)(frame >> 48), flo, fhi);
    flo = fhi;
  }
  return PCC_OK;
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
extern "C" int pcc_knn_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int k, int32_t* d_rows,
                              uint64_t* d_sqdist, int64_t* d_cov, float* d_normals, const int32_t* h_viewpoint) {
  const int64_t* offs;
  PCC_TRY(knn_entry(ctx, "pcc_knn_frames", {"k", k, 3, 32}, d_keys, n, n_frames, {"null keys", true, ""}, nullptr, 0, 0, &offs));
  if (!offs || (!d_rows && !d_sqdist && !d_cov && !d_normals)) return PCC_OK;
  PccProfScope prof(ctx, "knn_frames", n, k, n_frames, 0);
  const int32_t* vp = h_viewpoint;
  knn_with_cap(k, [&](auto cap) {
    hipLaunchKernelGGL(k_knn_frames<decltype(cap)::value>, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, d_keys, n, offs, k, d_rows,
                       d_sqdist, d_cov, d_normals, vp ? 1 : 0, vp ? vp[0] : 0, vp ? vp[1] : 0, vp ? vp[2] : 0);
  });
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// host only, no ctx: knn_point for every row on the calling thread — the kernel's traversal and epilogue, for counting
// the nodes it tries and for checks where there is no device.  Not a product path.
extern "C" int pcc_knn_replay_host(const uint64_t* h_keys, int64_t n, int k, int32_t* h_rows, uint64_t* h_sqdist, int64_t* h_cov,
                                   float* h_normals, uint32_t* h_nodes) {
  PCC_REQUIRE(k >= 3 && k <= 32 && n >= 0 && n <= NN_MAX_KEYS && (n == 0 || h_keys), PCC_E_ARG,
              "pcc_knn_replay_host: bad argument (n=%lld k=%d; k in 3 .. 32, at most 2^27 keys)", (long long)n, k);
  PCC_TRY(nn_host_sorted_distinct("pcc_knn_replay_host", "keys", h_keys, n));
  return knn_host_frames("pcc_knn_replay_host", h_keys, n, 65536, [] {}, [&](int, int64_t flo, int64_t fhi) {
    knn_with_cap(k, [&](auto cap) {
      for (int64_t i = flo; i < fhi; ++i) {
        const uint32_t nodes = knn_point<decltype(cap)::value>(h_keys, flo, fhi, i, k, h_rows, h_sqdist, h_cov, h_normals, false, 0, 0, 0);
        if (h_nodes) h_nodes[i] = nodes;
      }
    });
  });
}

// ---------------------------------------------------------------- outlier removal behind the same search
#include "outlier.h"

// ---------------------------------------------------------------- DBSCAN clusters: the radius rule's core points, united
#include "cluster.h"
