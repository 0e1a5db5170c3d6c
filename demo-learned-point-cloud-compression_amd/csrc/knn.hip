// knn.hip — the k nearest neighbours of every point of a frame among the frame's own points, the scatter matrix of
// that neighbourhood and its surface normal; and the D2 (point-to-plane) projection of a 1-NN pairing (nn.hip) onto
// such normals.  include/pcc.h has the rules; tests/normals_ref.py restates them in numpy.
//
// k_knn_frames is the k-best form of nn.hip's walk: sorted distinct Morton keys are an implicit octree, one thread per
// query walks the cells of its own frame in row order with scalar state and no stack.
//
//   list   the k best (d2, row) so far, ascending by (d2, row), in registers: a capacity template (8 / 16 / 32, chosen
//          by the host from k) whose insertion is fully unrolled, so every index is static and nothing lives in
//          scratch (DESIGN.md 6c has the figures).  The list sits at the END of the capacity: the CAP - k slots in
//          front hold (0, -1), below every candidate, so the pruning bound is always the last slot.  Free slots hold
//          (2^64 - 1, INT32_MAX): until the list holds k_eff = min(k, frame rows) entries nothing is pruned.
//   seed   the k_eff rows around the query's place in key order, clamped to the frame's rows, fill the list before the
//          walk starts; the walk measures every other row at most once, so no row enters twice.
//   walk   nn_search's: at row r the cells that begin at r are tried from the largest down; a cell whose box distance
//          exceeds the bound's d2, or equals it while r > the bound's row, is left out whole.
//
// Termination: every iteration of the walk moves r forward — a skip lands on a row of [r + 1, fhi], a measured point
// on r + 1 — and every binary search runs inside the frame's rows [flo, fhi): at most 47 halvings.  The seed loop
// counts k_eff rows.  No step waits for another thread.  Keep both properties: a walk that can stand still is a hang.
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

static inline unsigned nblk(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

#define KNN_NO_DIST (~0ull)
#define KNN_NO_ROW 0x7FFFFFFF

// bit 0: equal neighbours, bit 1: descending neighbours, bit 2: a key's frame index >= n_frames
__global__ __launch_bounds__(256) void k_knn_check(const uint64_t* __restrict__ keys, int64_t n, int n_frames,
                                                   int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int bits = 0;
  const uint64_t k = keys[i];
  if ((k >> 48) >= (uint64_t)n_frames) bits |= 4;
  if (i > 0) {
    const uint64_t p = keys[i - 1];
    if (p == k) bits |= 1;
    if (p > k) bits |= 2;
  }
  if (bits) atomicOr(flag, bits);
}

// offs[f] = the first row of frame f, offs[n_frames] = n
__global__ __launch_bounds__(64) void k_knn_offsets(const uint64_t* __restrict__ keys, int64_t n, int n_frames,
                                                    int64_t* __restrict__ offs) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_frames) return;
  int64_t lo = 0, hi = n;
  if (f == n_frames) lo = n;
  const uint64_t want = (uint64_t)f << 48;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  offs[f] = lo;
}

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

// the k-best search of one query among the rows [flo, fhi) of its frame, flo < fhi, 1 <= k <= CAP; L comes from
// knn_init.  Returns the nodes tried (cells tested and points measured, the seeds included).  One function for the
// device and the host, so pcc_knn_replay_host is the kernel's traversal.
template <int CAP>
__host__ __device__ static inline uint32_t knn_search(const uint64_t* __restrict__ keys, int64_t flo, int64_t fhi, uint64_t qk,
                                                      int k, KnnList<CAP>& L) {
  const uint32_t qx = pcc_compact3(qk >> 2), qy = pcc_compact3(qk >> 1), qz = pcc_compact3(qk);
  const int64_t n_f = fhi - flo;
  const int64_t k_eff = n_f < k ? n_f : k;
  uint32_t nodes = 0;
  int64_t lo = flo, hi = fhi;      // the first row of the frame whose key is not below the query's
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < qk) lo = mid + 1; else hi = mid;
  }
  int64_t s0 = lo - k_eff / 2;      // the seed rows [s0, s1) inside [flo, fhi)
  if (s0 > fhi - k_eff) s0 = fhi - k_eff;
  if (s0 < flo) s0 = flo;
  const int64_t s1 = s0 + k_eff;
  for (int64_t r = s0; r < s1; ++r) {
    knn_insert(L, nn_d2(qx, qy, qz, keys[r]), (int32_t)r);
    ++nodes;
  }
  if (k_eff == n_f) return nodes;      // the seed was the whole frame
  int64_t r = flo;
  uint64_t prev = 0;
  while (r < fhi) {
    const uint64_t key = keys[r];
    int Lv = r == flo ? 15 : (63 - __builtin_clzll(((prev ^ key) & NN_KEY48) | 1ull)) / 3;      // keys are distinct
    const uint32_t cx = pcc_compact3(key >> 2), cy = pcc_compact3(key >> 1), cz = pcc_compact3(key);
    // the cells of levels 0 .. l1 hold row r alone (key r + 1 leaves them): measuring the point is their test
    const int l1 = r + 1 < fhi ? (63 - __builtin_clzll(((key ^ keys[r + 1]) & NN_KEY48) | 1ull)) / 3 : 15;
    const uint64_t bound = L.d[CAP - 1];
    const int64_t bound_row = L.r[CAP - 1];
    bool skipped = false;
    for (; Lv > l1; --Lv) {
      const uint64_t bd = (uint64_t)nn_gap_sq(qx, cx, Lv) + nn_gap_sq(qy, cy, Lv) + nn_gap_sq(qz, cz, Lv);
      ++nodes;
      if (bd > bound || (bd == bound && r > bound_row)) {
        // the first row behind the cell, whose keys are [p << 3L, (p + 1) << 3L)
        const uint64_t end = (((key & NN_KEY48) >> (3 * Lv)) + 1ull) << (3 * Lv);
        int64_t a = r + 1, b = fhi;
        if (end <= NN_KEY48) {
          const uint64_t want = (key & ~NN_KEY48) | end;
          while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (keys[mid] < want) a = mid + 1; else b = mid;
          }
        } else {
          a = fhi;      // the cell reaches the end of the key range
        }
        r = a;
        skipped = true;
        break;
      }
    }
    if (skipped) {
      if (r < fhi) prev = keys[r - 1];
      continue;
    }
    if (r < s0 || r >= s1) {      // a seed row is in the list already
      knn_insert(L, (uint64_t)nn_sq(qx, cx) + nn_sq(qy, cy) + nn_sq(qz, cz), (int32_t)r);
      ++nodes;
    }
    prev = key;
    ++r;
  }
  return nodes;
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
  const int f = (int)(keys[i] >> 48);      // below n_frames: k_knn_check
  const int64_t flo = offs[f], fhi = offs[f + 1];      // flo <= i < fhi: row i is a row of its own frame
  (void)knn_point<CAP>(keys, flo, fhi, i, k, rows, sqdist, cov, normals, has_vp != 0, vx, vy, vz);
}

// proj[i] = ((q_i - r_row[i]) . n)^2 in float64, n = row normal_row[i] (row i without normal_row) of normals, the dot
// product as (ex nx + ey ny) + ez nz; sum[f] += proj over the queries i of frame f.  A query without a row (-1), a
// row outside the reference, a negative normal row or a frame index outside the call adds nothing (proj 0).  The
// reduction is k_nn_frames': per frame present in the wave shuffles, then one atomic from one lane.
__global__ __launch_bounds__(256) void k_nn_d2(const uint64_t* __restrict__ qkeys, const int32_t* __restrict__ row, int64_t n_q,
                                               const uint64_t* __restrict__ rkeys, int64_t n_r, const float* __restrict__ normals,
                                               const int32_t* __restrict__ normal_row, int n_frames, double* __restrict__ proj,
                                               double* __restrict__ sum) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  int f = 0;
  double p = 0.0;
  if (i < n_q) {
    const int64_t r = row[i];
    const uint64_t qk = qkeys[i];
    const int64_t nr = normal_row ? (int64_t)normal_row[i] : i;
    f = (int)(qk >> 48);
    if (r >= 0 && r < n_r && nr >= 0 && f < n_frames) {
      valid = true;
      const uint64_t rk = rkeys[r];
      const double ex = (double)((int)pcc_compact3(qk >> 2) - (int)pcc_compact3(rk >> 2)),
                   ey = (double)((int)pcc_compact3(qk >> 1) - (int)pcc_compact3(rk >> 1)),
                   ez = (double)((int)pcc_compact3(qk) - (int)pcc_compact3(rk));
      const float* n = normals + nr * 3;
      const double d = (ex * (double)n[0] + ey * (double)n[1]) + ez * (double)n[2];
      p = d * d;
    }
    if (proj) proj[i] = p;
  }
  if (!sum) return;      // the same in every lane
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int f0 = __shfl(f, leader);
    const bool mine = valid && f == f0;
    double s = mine ? p : 0.0;
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if (lane == leader) atomicAdd(&sum[f0], s);
    todo &= ~__ballot(mine);
  }
}

// ---------------------------------------------------------------- C-ABI (include/pcc.h)
template <int CAP>
static void knn_launch(hipStream_t st, const uint64_t* d_keys, int64_t n, const int64_t* offs, int k, int32_t* d_rows,
                       uint64_t* d_sqdist, int64_t* d_cov, float* d_normals, const int32_t* vp) {
  hipLaunchKernelGGL(k_knn_frames<CAP>, dim3(nblk(n, 256)), dim3(256), 0, st, d_keys, n, offs, k, d_rows, d_sqdist, d_cov,
                     d_normals, vp ? 1 : 0, vp ? vp[0] : 0, vp ? vp[1] : 0, vp ? vp[2] : 0);
}

extern "C" int pcc_knn_frames(pcc_ctx* ctx, const uint64_t* d_keys, int64_t n, int n_frames, int k, int32_t* d_rows,
                              uint64_t* d_sqdist, int64_t* d_cov, float* d_normals, const int32_t* h_viewpoint) {
  const int64_t kMax = (int64_t)1 << 27;
  PCC_REQUIRE(ctx && k >= 3 && k <= 32 && n >= 0 && n <= kMax && n_frames >= 1 && n_frames <= 65535, PCC_E_ARG,
              "pcc_knn_frames: bad argument (n=%lld n_frames=%d k=%d; k in 3 .. 32, at most 2^27 keys, 1 .. 65535 frames)",
              (long long)n, n_frames, k);
  PCC_REQUIRE(n == 0 || d_keys, PCC_E_ARG, "pcc_knn_frames: null keys");
  if (n == 0) return PCC_OK;
  hipStream_t st = ctx->stream;
  const size_t offs_b = (size_t)(n_frames + 1) * 8;
  PCC_TRY(pcc_arena_reserve(ctx, pcc_align(offs_b) + 512));
  int64_t* offs = (int64_t*)pcc_arena_alloc(ctx, offs_b);
  int32_t* flag = (int32_t*)pcc_arena_alloc(ctx, 4);
  if (!offs || !flag) return PCC_E_NOMEM;
  PCC_HIP(hipMemsetAsync(flag, 0, 4, st));
  hipLaunchKernelGGL(k_knn_check, dim3(nblk(n, 256)), dim3(256), 0, st, d_keys, n, n_frames, flag);
  PCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_knn_offsets, dim3(nblk(n_frames + 1, 64)), dim3(64), 0, st, d_keys, n, n_frames, offs);
  PCC_CHECK_LAUNCH();
  int32_t* h = (int32_t*)ctx->pinned;
  PCC_HIP(hipMemcpyAsync(h, flag, 4, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipStreamSynchronize(st));
  const int32_t bits = h[0];
  PCC_REQUIRE(!(bits & 4), PCC_E_RANGE, "pcc_knn_frames: a key's frame index is not below n_frames=%d", n_frames);
  PCC_REQUIRE(!(bits & 2), PCC_E_ARG, "pcc_knn_frames: keys not sorted (pcc_sort_pairs)");
  PCC_REQUIRE(!(bits & 1), PCC_E_DUP, "pcc_knn_frames: duplicate keys");
  if (!d_rows && !d_sqdist && !d_cov && !d_normals) return PCC_OK;
  PccProfScope prof(ctx, "knn_frames", n, k, n_frames, 0);
  if (k <= 8) knn_launch<8>(st, d_keys, n, offs, k, d_rows, d_sqdist, d_cov, d_normals, h_viewpoint);
  else if (k <= 16) knn_launch<16>(st, d_keys, n, offs, k, d_rows, d_sqdist, d_cov, d_normals, h_viewpoint);
  else knn_launch<32>(st, d_keys, n, offs, k, d_rows, d_sqdist, d_cov, d_normals, h_viewpoint);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

extern "C" int pcc_nn_d2_frames(pcc_ctx* ctx, const uint64_t* d_qkeys, const int32_t* d_row, int64_t n_q, const uint64_t* d_rkeys,
                                int64_t n_r, const float* d_normals, const int32_t* d_normal_row, int n_frames, double* d_proj,
                                double* d_sum) {
  const int64_t kMax = (int64_t)1 << 27;
  PCC_REQUIRE(ctx && n_frames >= 1 && n_frames <= 65535 && n_q >= 0 && n_q <= kMax && n_r >= 0 && n_r <= kMax, PCC_E_ARG,
              "pcc_nn_d2_frames: bad argument (n_q=%lld n_r=%lld n_frames=%d)", (long long)n_q, (long long)n_r, n_frames);
  PCC_REQUIRE(n_q == 0 || (d_qkeys && d_row), PCC_E_ARG, "pcc_nn_d2_frames: null query arrays");
  PCC_REQUIRE(n_q == 0 || n_r == 0 || (d_rkeys && d_normals), PCC_E_ARG, "pcc_nn_d2_frames: null reference keys or normals");
  hipStream_t st = ctx->stream;
  if (d_sum) PCC_HIP(hipMemsetAsync(d_sum, 0, (size_t)n_frames * 8, st));
  if (n_q == 0 || (!d_proj && !d_sum)) return PCC_OK;
  if (n_r == 0) {      // no row can be valid
    if (d_proj) PCC_HIP(hipMemsetAsync(d_proj, 0, (size_t)n_q * 8, st));
    return PCC_OK;
  }
  PccProfScope prof(ctx, "nn_d2", n_q, n_r, n_frames, 0);
  hipLaunchKernelGGL(k_nn_d2, dim3(nblk(n_q, 256)), dim3(256), 0, st, d_qkeys, d_row, n_q, d_rkeys, n_r, d_normals, d_normal_row,
                     n_frames, d_proj, d_sum);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

// host only, no ctx: knn_point for every row on the calling thread — the kernel's traversal and epilogue, for counting
// the nodes it tries and for checks where there is no device.  Not a product path.
template <int CAP>
static void knn_replay(const uint64_t* h_keys, int64_t n, int k, int32_t* h_rows, uint64_t* h_sqdist, int64_t* h_cov,
                       float* h_normals, uint32_t* h_nodes) {
  int64_t flo = 0;
  while (flo < n) {
    const uint64_t frame = h_keys[flo] & ~NN_KEY48;
    const int64_t fhi = std::upper_bound(h_keys + flo, h_keys + n, frame | NN_KEY48) - h_keys;
    for (int64_t i = flo; i < fhi; ++i) {
      const uint32_t nodes = knn_point<CAP>(h_keys, flo, fhi, i, k, h_rows, h_sqdist, h_cov, h_normals, false, 0, 0, 0);
      if (h_nodes) h_nodes[i] = nodes;
    }
    flo = fhi;
  }
}

extern "C" int pcc_knn_replay_host(const uint64_t* h_keys, int64_t n, int k, int32_t* h_rows, uint64_t* h_sqdist, int64_t* h_cov,
                                   float* h_normals, uint32_t* h_nodes) {
  const int64_t kMax = (int64_t)1 << 27;
  PCC_REQUIRE(k >= 3 && k <= 32 && n >= 0 && n <= kMax && (n == 0 || h_keys), PCC_E_ARG,
              "pcc_knn_replay_host: bad argument (n=%lld k=%d; k in 3 .. 32, at most 2^27 keys)", (long long)n, k);
  for (int64_t i = 1; i < n; ++i) {
    PCC_REQUIRE(h_keys[i - 1] <= h_keys[i], PCC_E_ARG, "pcc_knn_replay_host: keys not sorted (pcc_sort_pairs)");
    PCC_REQUIRE(h_keys[i - 1] != h_keys[i], PCC_E_DUP, "pcc_knn_replay_host: duplicate keys");
  }
  if (k <= 8) knn_replay<8>(h_keys, n, k, h_rows, h_sqdist, h_cov, h_normals, h_nodes);
  else if (k <= 16) knn_replay<16>(h_keys, n, k, h_rows, h_sqdist, h_cov, h_normals, h_nodes);
  else knn_replay<32>(h_keys, n, k, h_rows, h_sqdist, h_cov, h_normals, h_nodes);
  return PCC_OK;
}
