// The host replay of the clustering rule (csrc/cluster.h behind csrc/knn.hip: pcc_cluster_replay_host and its reversed
// twin, the kernels' __host__ __device__ functions compiled for the host) over random and degenerate key sets, every
// buffer sized exactly: labels, sizes, counts, core flags and roots against a brute force over all pairs with a
// sequential union-find of its own, in both orders of the unions.  Degenerate sets: points on a line with two
// coordinates equal, a dense cube, one point, empty frames, the far corners of the lattice; then the refusals.
// Built with -fsanitize=address,undefined for the host by tests/test_geometry_cluster.py; nothing here touches a device.
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

static uint64_t seed = 90210;
static uint32_t rnd() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); }

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); exit(1); }  \
  } while (0)

struct P { int x, y, z; };

static int64_t find_ref(std::vector<int64_t>& parent, int64_t x) {
  while (parent[x] != x) x = parent[x] = parent[parent[x]];
  return x;
}

// frames: the points of every frame, any order, duplicates allowed -> checks of the replay in both orders
static void run(const std::vector<std::vector<P>>& frames, int m, uint64_t radius2, int64_t min_points) {
  const int nf = (int)frames.size();
  std::vector<uint64_t> keys;
  for (int f = 0; f < nf; ++f)
    for (const P& p : frames[f]) keys.push_back(pcc_morton(f, p.x, p.y, p.z));
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const int64_t n = (int64_t)keys.size();
  // the brute force, frame by frame
  std::vector<int32_t> want_label(n, -1), want_root(n, -1);
  std::vector<uint8_t> want_core(n, 0);
  std::vector<uint32_t> want_sizes(n, 0);
  std::vector<uint64_t> want_counts(4 * (size_t)nf, 0);
  std::vector<int64_t> lo(nf + 1, n);
  for (int64_t i = n - 1; i >= 0; --i) lo[keys[i] >> 48] = i;
  for (int f = nf - 1; f >= 0; --f) lo[f] = std::min(lo[f], lo[f + 1]);
  for (int f = 0; f < nf; ++f) {
    const int64_t a = lo[f], b = lo[f + 1], nfr = b - a;
    std::vector<uint64_t> d((size_t)(nfr * nfr));
    for (int64_t i = a; i < b; ++i)
      for (int64_t j = a; j < b; ++j) {
        int fi, x0, y0, z0, x1, y1, z1;
        pcc_unmorton(keys[i], &fi, &x0, &y0, &z0);
        pcc_unmorton(keys[j], &fi, &x1, &y1, &z1);
        const int64_t dx = x0 - x1, dy = y0 - y1, dz = z0 - z1;
        d[(size_t)((i - a) * nfr + (j - a))] = (uint64_t)(dx * dx + dy * dy + dz * dz);
      }
    std::vector<int64_t> parent((size_t)nfr), size((size_t)nfr, 0), root((size_t)nfr, -1);
    uint64_t n_core = 0, n_noise = 0;
    for (int64_t i = 0; i < nfr; ++i) {
      int within = 0;
      for (int64_t j = 0; j < nfr; ++j) within += j != i && d[(size_t)(i * nfr + j)] <= radius2;
      want_core[a + i] = within >= m ? 1 : 0;
      n_core += want_core[a + i];
      parent[i] = i;
    }
    for (int64_t i = 0; i < nfr; ++i)
      for (int64_t j = 0; j < i; ++j)
        if (want_core[a + i] && want_core[a + j] && d[(size_t)(i * nfr + j)] <= radius2) {
          const int64_t ri = find_ref(parent, i), rj = find_ref(parent, j);
          if (ri != rj) parent[std::max(ri, rj)] = std::min(ri, rj);
        }
    for (int64_t i = 0; i < nfr; ++i) {
      if (want_core[a + i]) {
        root[i] = find_ref(parent, i);
      } else {
        int64_t best = -1;
        for (int64_t j = 0; j < nfr; ++j)      // ascending rows: the first of the nearest stays
          if (want_core[a + j] && d[(size_t)(i * nfr + j)] <= radius2 && (best < 0 || d[(size_t)(i * nfr + j)] < d[(size_t)(i * nfr + best)]))
            best = j;
        if (best >= 0) root[i] = find_ref(parent, best);
      }
      if (root[i] >= 0) ++size[root[i]];
    }
    std::vector<int64_t> alive;
    for (int64_t i = 0; i < nfr; ++i)
      if (root[i] == i && size[i] >= min_points) alive.push_back(i);
    std::stable_sort(alive.begin(), alive.end(), [&](int64_t p, int64_t q) { return size[p] > size[q]; });
    std::vector<int32_t> label_of((size_t)nfr, -1);
    for (size_t k = 0; k < alive.size(); ++k) {
      label_of[alive[k]] = (int32_t)k;
      want_sizes[a + (int64_t)k] = (uint32_t)size[alive[k]];
    }
    for (int64_t i = 0; i < nfr; ++i) {
      want_root[a + i] = root[i] < 0 ? -1 : (int32_t)(a + root[i]);
      want_label[a + i] = root[i] < 0 ? -1 : label_of[root[i]];
      n_noise += want_label[a + i] < 0;
    }
    want_counts[4 * f] = (uint64_t)nfr; want_counts[4 * f + 1] = n_core; want_counts[4 * f + 2] = alive.size(); want_counts[4 * f + 3] = n_noise;
  }
  for (int rev = 0; rev < 2; ++rev) {
    // exactly sized heap buffers: a write past the end is a report
    std::vector<int32_t> labels(n), root(n);
    std::vector<uint32_t> sizes(n), nodes(n);
    std::vector<uint64_t> counts(4 * (size_t)nf);
    std::vector<uint8_t> core(n);
    const int rc = (rev ? pcc_cluster_replay_host_reversed : pcc_cluster_replay_host)(
        keys.data(), n, nf, m, radius2, min_points, labels.data(), sizes.data(), counts.data(), core.data(), root.data(), nodes.data());
    CHECK(rc == PCC_OK);
    CHECK(labels == want_label);
    CHECK(sizes == want_sizes);
    CHECK(counts == want_counts);
    CHECK(core == want_core);
    CHECK(root == want_root);
    // every output is nullable
    CHECK((rev ? pcc_cluster_replay_host_reversed : pcc_cluster_replay_host)(keys.data(), n, nf, m, radius2, min_points, labels.data(),
                                                                             nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_OK);
    CHECK(labels == want_label);
  }
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 200;
  const uint64_t radii[] = {0, 1, 2, 3, 12, 100, 4096};
  const int64_t min_pts[] = {1, 2, 5, 50, (int64_t)1 << 27};
  // degenerate sets
  for (int m : {0, 1, 3, 7, 8, 15, 16, 31}) {
    for (int n : {1, 2, 9, 33, 64}) {
      std::vector<P> line, cube;
      for (int i = 0; i < n; ++i) line.push_back({3 * i - 20, 5, 5});      // two coordinates equal on the whole line
      for (int i = 0; i < n; ++i) cube.push_back({i & 3, (i >> 2) & 3, i >> 4});
      for (uint64_t r2 : radii) {
        run({line}, m, r2, 1);
        run({cube, line, {}}, m, r2, min_pts[rnd() % 5]);
      }
    }
    run({{{-32768, -32768, -32768}, {32767, 32767, 32767}, {32767, 32767, 32766}}}, m, 1, 1);
    run({{{-32768, -32768, -32768}, {32767, 32767, 32767}}}, m, 4096, 1);
    run({{}, {}}, m, 0, 1);
  }
  // random sets: tight clusters with far points, up to three frames
  for (int it = 0; it < iters; ++it) {
    const int nf = 1 + (int)(rnd() % 3);
    std::vector<std::vector<P>> frames(nf);
    for (auto& fr : frames) {
      const int n = (int)(rnd() % 150), span = 1 + (int)(rnd() % (rnd() % 4 ? 12 : 3000));
      const int cx = (int)(rnd() % 60000) - 30000, cy = (int)(rnd() % 60000) - 30000, cz = (int)(rnd() % 60000) - 30000;
      for (int i = 0; i < n; ++i) {
        auto c = [&](int c0) { return std::max(-32768, std::min(32767, c0 + (int)(rnd() % span))); };
        if (rnd() % 16 == 0) fr.push_back({(int)(rnd() % 65536) - 32768, (int)(rnd() % 65536) - 32768, (int)(rnd() % 65536) - 32768});
        else fr.push_back({c(cx), c(cy), c(cz)});
      }
    }
    run(frames, (int)(rnd() % (rnd() % 2 ? 6 : 32)), radii[rnd() % 7], min_pts[rnd() % 4]);
  }
  // refusals
  uint64_t two[2] = {5, 5};
  int32_t labels[2];
  CHECK(pcc_cluster_replay_host(two, 2, 1, 0, 1, 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_DUP);
  two[1] = 4;
  CHECK(pcc_cluster_replay_host(two, 2, 1, 0, 1, 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  two[1] = 1ull << 48;
  CHECK(pcc_cluster_replay_host(two, 2, 1, 0, 1, 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_RANGE);
  two[1] = 6;
  CHECK(pcc_cluster_replay_host(two, 2, 1, 32, 1, 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  CHECK(pcc_cluster_replay_host(two, 2, 1, -1, 1, 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  CHECK(pcc_cluster_replay_host(two, 2, 1, 0, 4097, 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  CHECK(pcc_cluster_replay_host(two, 2, 1, 0, 1, 0, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  CHECK(pcc_cluster_replay_host(two, 2, 1, 0, 1, ((int64_t)1 << 27) + 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  CHECK(pcc_cluster_replay_host_reversed(two, 2, 0, 0, 1, 1, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_E_ARG);
  CHECK(pcc_cluster_replay_host(two, 2, 1, 31, 4096, (int64_t)1 << 27, labels, nullptr, nullptr, nullptr, nullptr, nullptr) == PCC_OK);
  CHECK(labels[0] == -1 && labels[1] == -1);
  printf("fuzz: %d random sets ok\n", iters);
  return 0;
}
