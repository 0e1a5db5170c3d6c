// The host replay of the outlier rules (csrc/outlier.h behind csrc/knn.hip: pcc_outlier_replay_host, the kernels'
// __host__ __device__ functions compiled for the host) over random and degenerate key sets, every buffer sized exactly:
// scores and frame sums against a brute force over all pairs, the radius rule under the bounded search against the
// unbounded one and against a count over all pairs, nodes tried bounded <= unbounded.  Degenerate sets: points on a
// line with two coordinates equal, one point, n just below, at and above k, the two far corners of the lattice.
// Built with -fsanitize=address,undefined for the host by tests/test_geometry_filter.py; nothing here touches a device.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "knn.hip"

// what knn.hip takes from the rest of the library: only the host checks are ever reached
void pcc_set_error(const char* fmt, ...) {}
int nn_check_and_offsets(pcc_ctx*, const char*, const char*, const char*, const uint64_t*, int64_t, const uint64_t*, int64_t, int,
                         const int64_t**) { abort(); }
int nn_host_sorted_distinct(const char*, const char*, const uint64_t* h_keys, int64_t n) {
  for (int64_t i = 1; i < n; ++i) {
    if (h_keys[i - 1] > h_keys[i]) return PCC_E_ARG;
    if (h_keys[i - 1] == h_keys[i]) return PCC_E_DUP;
  }
  return PCC_OK;
}
PccProfScope::PccProfScope(pcc_ctx*, const char*, int64_t, int64_t, int64_t, int64_t) : c(nullptr), slot(-1) {}
PccProfScope::~PccProfScope() {}
int pcc_arena_reserve(pcc_ctx*, size_t) { abort(); }
void* pcc_arena_alloc(pcc_ctx*, size_t) { abort(); }
int pcc_scan_exclusive_u32(pcc_ctx*, const uint32_t*, uint32_t*, int64_t, uint32_t*) { abort(); }
size_t pcc_scan_scratch_bytes(int64_t) { abort(); }

static uint64_t seed = 4243;
static uint32_t rnd() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); }

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); exit(1); }  \
  } while (0)

struct P { int x, y, z; };

static uint64_t isqrt_ref(uint64_t x) {      // bisection on integers alone
  uint64_t lo = 0, hi = (uint64_t)1 << 32;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (mid * mid <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// frames: the points of every frame, any order, duplicates allowed -> checks of one replay call
static void run(const std::vector<std::vector<P>>& frames, int k, int m, uint64_t radius2) {
  const int nf = (int)frames.size();
  std::vector<uint64_t> keys;
  for (int f = 0; f < nf; ++f)
    for (const P& p : frames[f]) keys.push_back(pcc_morton(f, p.x, p.y, p.z));
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const int64_t n = (int64_t)keys.size();
  // exactly sized heap buffers: a write past the end is a report
  std::vector<uint64_t> scores(n), sums(4 * (size_t)nf), th(nf, 0);
  std::vector<uint32_t> nodes(n), nodes_b(n), nodes_u(n);
  std::vector<uint8_t> keep(n), keep_b(n), keep_u(n);
  int rc = pcc_outlier_replay_host(keys.data(), n, nf, k, m, radius2, nullptr, scores.data(), sums.data(), nullptr, nodes.data(),
                                   keep_b.data(), nodes_b.data(), keep_u.data(), nodes_u.data());
  CHECK(rc == PCC_OK);
  std::vector<int64_t> lo(nf + 1, n);
  for (int64_t i = n - 1; i >= 0; --i) lo[keys[i] >> 48] = i;
  for (int f = nf - 1; f >= 0; --f) lo[f] = std::min(lo[f], lo[f + 1]);
  for (int f = 0; f < nf; ++f) {
    const int64_t a = lo[f], b = lo[f + 1];
    uint64_t s1 = 0, s2 = 0;
    for (int64_t i = a; i < b; ++i) {
      std::vector<uint64_t> d;
      int within = 0;
      for (int64_t j = a; j < b; ++j) {
        int fi, x0, y0, z0, x1, y1, z1;
        pcc_unmorton(keys[i], &fi, &x0, &y0, &z0);
        pcc_unmorton(keys[j], &fi, &x1, &y1, &z1);
        const int64_t dx = x0 - x1, dy = y0 - y1, dz = z0 - z1;
        d.push_back((uint64_t)(dx * dx + dy * dy + dz * dz));
        if (j != i && d.back() <= radius2) ++within;
      }
      std::sort(d.begin(), d.end());
      uint64_t q = 0;
      for (size_t j = 0; j < d.size() && j < (size_t)k; ++j) q += isqrt_ref(d[j] << 8);
      CHECK(scores[i] == q);
      CHECK(keep_u[i] == (within >= m ? 1 : 0));
      CHECK(keep_b[i] == keep_u[i]);
      CHECK(nodes_b[i] <= nodes_u[i]);
      CHECK(nodes[i] >= 1 && nodes_b[i] >= 1);
      s1 += q;
      s2 += q * q;      // n <= a few hundred: no overflow here
    }
    CHECK(sums[4 * f] == s1 && sums[4 * f + 1] + (sums[4 * f + 2] << 32) == s2 && sums[4 * f + 3] == (uint64_t)(b - a));
    th[f] = b > a ? s1 / (uint64_t)(b - a) : 0;      // the mean as a threshold: both verdicts occur
  }
  rc = pcc_outlier_replay_host(keys.data(), n, nf, k, m, radius2, th.data(), scores.data(), nullptr, keep.data(), nullptr, nullptr,
                               nullptr, nullptr, nullptr);
  CHECK(rc == PCC_OK);
  for (int64_t i = 0; i < n; ++i) CHECK(keep[i] == (scores[i] <= th[keys[i] >> 48] ? 1 : 0));
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 300;
  const uint64_t far2 = 3ull * 65535ull * 65535ull;
  const uint64_t radii[] = {0, 1, 3, 25, 400, far2, ~0ull};
  // the root itself
  for (uint64_t r = 1; r < (1ull << 21); r = r * 3 + 1)
    for (int64_t e = -1; e <= 1; ++e) CHECK(pcc_outlier_isqrt_host(r * r + e) == isqrt_ref(r * r + e));
  CHECK(pcc_outlier_isqrt_host(far2 << 8) == isqrt_ref(far2 << 8));
  // degenerate sets
  for (int k : {3, 8, 9, 16, 17, 32}) {
    for (int n : {1, 2, k - 1, k, k + 1}) {
      std::vector<P> line, cube;
      for (int i = 0; i < n; ++i) line.push_back({7 * i - 20, 5, 5});      // two coordinates equal on the whole line
      for (int i = 0; i < n; ++i) cube.push_back({i & 3, (i >> 2) & 3, i >> 4});
      for (uint64_t r2 : radii) {
        run({line}, k, std::min(31, k - 1), r2);
        run({cube, line, {}}, k, 1 + (int)(rnd() % 31), r2);
      }
    }
    run({{{-32768, -32768, -32768}, {32767, 32767, 32767}}}, k, 1, far2);
    run({{{-32768, -32768, -32768}, {32767, 32767, 32767}}}, k, 1, far2 - 1);
    run({{}, {}}, k, 1, 0);
  }
  // random sets: tight clusters with far points, up to three frames
  for (int it = 0; it < iters; ++it) {
    const int nf = 1 + (int)(rnd() % 3);
    std::vector<std::vector<P>> frames(nf);
    for (auto& fr : frames) {
      const int n = (int)(rnd() % 120), span = 1 + (int)(rnd() % (rnd() % 2 ? 12 : 3000));
      const int cx = (int)(rnd() % 60000) - 30000, cy = (int)(rnd() % 60000) - 30000, cz = (int)(rnd() % 60000) - 30000;
      for (int i = 0; i < n; ++i) {
        auto c = [&](int c0) { return std::max(-32768, std::min(32767, c0 + (int)(rnd() % span))); };
        if (rnd() % 16 == 0) fr.push_back({(int)(rnd() % 65536) - 32768, (int)(rnd() % 65536) - 32768, (int)(rnd() % 65536) - 32768});
        else fr.push_back({c(cx), c(cy), c(cz)});
      }
    }
    run(frames, 3 + (int)(rnd() % 30), 1 + (int)(rnd() % 31), radii[rnd() % 7]);
  }
  // refusals
  uint64_t two[2] = {5, 5};
  CHECK(pcc_outlier_replay_host(two, 2, 1, 3, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_DUP);
  two[1] = 4;
  CHECK(pcc_outlier_replay_host(two, 2, 1, 3, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  two[1] = 1ull << 48;
  CHECK(pcc_outlier_replay_host(two, 2, 1, 3, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_RANGE);
  printf("fuzz: %d random sets ok\n", iters);
  return 0;
}
