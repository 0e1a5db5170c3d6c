// The version-4 octree blob's header parser (csrc/octree4_blob.h) on damaged blobs and on blobs cut anywhere: error
// codes, never a read outside the bytes present, and what an accepted header lets the decoder size lies inside them.
// Built with -fsanitize=address,undefined by tests/test_fuzz_octree4_header.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "octree4_blob.h"
int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  uint64_t seed = 4244;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  // a well-formed blob: depth 9, 90000 points, the encoder's layout (256 nodes per lane), random run lengths
  const int d = 9, s_max = 256;
  const int64_t level_n[d] = {1, 8, 30, 100, 400, 1500, 6000, 20000, 50000}, n = 90000;
  int64_t n_nodes = 0;
  for (int L = 0; L < d; ++L) n_nodes += level_n[L];
  const int64_t nc = (n_nodes + kO4Lanes * s_max - 1) / (kO4Lanes * s_max);
  const int64_t S = ((n_nodes + kO4Lanes * nc - 1) / (kO4Lanes * nc) + 3) / 4 * 4;
  const int64_t off_p0 = kO4Header + 4 * d + 20, off_table = off_p0 + 2 * kO4Ctx, off_payload = off_table + 4 * nc;
  std::vector<uint8_t> blob((size_t)off_payload);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'O'; blob[1] = 4; blob[2] = d;
  put32(4, (uint32_t)n);
  put32(8, (uint32_t)-512); put32(12, 1024u); put32(16, (uint32_t)-32768);
  for (int L = 0; L < d; ++L) put32(kO4Header + 4 * L, (uint32_t)level_n[L]);
  put32(kO4Header + 4 * d, (uint32_t)S);
  put32(kO4Header + 4 * d + 4, (uint32_t)nc);
  put32(kO4Header + 4 * d + 8, 88888u);                                       // ref_n
  put32(kO4Header + 4 * d + 12, 0x89ABCDEFu); put32(kO4Header + 4 * d + 16, 0x01234567u);   // ref_sum
  for (int i = 0; i < kO4Ctx; ++i) { blob[off_p0 + 2 * i] = 0x00; blob[off_p0 + 2 * i + 1] = 0x08; }   // 2048
  for (int64_t c = 0; c < nc; ++c) {
    std::vector<uint8_t> ch(2 * 3 * kO4Lanes, 0x5A);
    uint32_t cw = 3 * kO4Lanes;
    for (int l = 0; l < kO4Lanes; ++l) {
      const uint32_t len = rnd() % 400;
      ch[4 * kO4Lanes + 2 * l] = (uint8_t)len;
      ch[4 * kO4Lanes + 2 * l + 1] = (uint8_t)(len >> 8);
      cw += len;
    }
    put32((size_t)(off_table + 4 * c), cw);
    ch.resize(2 * (size_t)cw, 0xA5);
    blob.insert(blob.end(), ch.begin(), ch.end());
  }
  put32(20, (uint32_t)(blob.size() - kO4Header));
  O4Info o;
  int rc = o4_parse(blob.data(), (int64_t)blob.size(), &o);
  printf("well-formed: rc %d n %lld nodes %lld S %lld chunks %lld ref_n %u of %zu bytes\n", rc, (long long)o.n, (long long)o.n_nodes,
         (long long)o.S, (long long)o.nc, o.ref_n, blob.size());
  if (rc != 0 || o.n != n || o.n_nodes != n_nodes || o.S != S || o.nc != nc || o.ref_n != 88888u || o.ref_sum != 0x0123456789ABCDEFull ||
      o.off_p0 != off_p0 || o.off_table != off_table || o.off_payload != off_payload)
    return 1;
  {   // two bytes short, two bytes long, version 2's header in its place
    std::vector<uint8_t> cut(blob.begin(), blob.end() - 2), longer(blob);
    longer.push_back(0); longer.push_back(0);
    if (o4_parse(cut.data(), (int64_t)cut.size(), &o) == 0 || o4_parse(longer.data(), (int64_t)longer.size(), &o) == 0) return 4;
    std::vector<uint8_t> v2(blob);
    v2[1] = 2;
    if (o4_parse(v2.data(), (int64_t)v2.size(), &o) == 0) return 5;
  }
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % (blob.size() + 1)) : (int64_t)blob.size();
    std::vector<uint8_t> b(blob.begin(), blob.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (it % 7 == 0) ? 0 : 1 + (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const int64_t at = (int64_t)(rnd() % (uint32_t)off_payload);   // the part the parser reads
      if (at < (int64_t)b.size()) b[(size_t)at] ^= (uint8_t)(1u << (rnd() & 7));
    }
    if (it % 11 == 0 && b.size() >= 24) {   // a cut blob whose announced length was made to fit
      const uint32_t pay = (uint32_t)(b.size() - kO4Header);
      for (int i = 0; i < 4; ++i) b[20 + i] = (uint8_t)(pay >> (8 * i));
    }
    O4Info q;
    const int r = o4_parse(b.empty() ? nullptr : b.data(), (int64_t)b.size(), &q);
    if (r == 0) {
      ++oks;   // accepted: everything the decoder sizes from lies inside what is present and under the header's bounds
      if (q.off_payload + 2 * q.payload_words != (int64_t)b.size()) return 2;
      if (q.n < 1 || q.depth < 1 || q.depth > 16 || q.n_nodes < q.depth || q.n_nodes > q.n * q.depth) return 8;
      if (q.S < 4 || q.S > kO4SLimit || q.S % 4 || q.nc < 1 || kO4Lanes * q.S * q.nc < q.n_nodes || kO4Lanes * q.S * (q.nc - 1) >= q.n_nodes) return 9;
      if (q.payload_words < 3 * kO4Lanes * q.nc || q.off_table + 4 * q.nc != q.off_payload) return 10;
      int64_t sum = 0;
      for (int L = 0; L < q.depth; ++L) sum += q.level_n[L];
      if (sum != q.n_nodes || q.n > 8 * q.level_n[q.depth - 1]) return 11;
    } else {
      ++errs;
    }
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 3;
}
