// The version-2 octree blob's header parser and level-of-detail plan (csrc/octree2_blob.h) on damaged blobs and on
// prefixes cut anywhere: error codes, never a read outside the bytes present, and an accepted plan sizes nothing beyond
// them.  Built with -fsanitize=address,undefined by tests/test_fuzz_octree2_header.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "octree2_blob.h"
int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  uint64_t seed = 4242;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  // a well-formed blob: depth 9, 90000 points, the encoder's layout, random run lengths in every chunk's length table
  const int d = 9;
  const int64_t level_n[d] = {1, 8, 30, 100, 400, 1500, 6000, 20000, 50000}, n = 90000;
  int64_t n_nodes = 0;
  for (int L = 0; L < d; ++L) n_nodes += level_n[L];
  int64_t nc = (n_nodes + kO2Lanes * kO2SMax - 1) / (kO2Lanes * kO2SMax);
  int64_t S = ((n_nodes + kO2Lanes * nc - 1) / (kO2Lanes * nc) + 3) / 4 * 4;
  const int64_t off_table = kO2Header + 4 * d + 8 + 2 * kO2Ctx, off_payload = off_table + 4 * nc;
  std::vector<uint8_t> blob((size_t)off_payload);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'O'; blob[1] = 2; blob[2] = d;
  put32(4, (uint32_t)n);
  put32(8, (uint32_t)-512); put32(12, 1024u); put32(16, (uint32_t)-32768);
  for (int L = 0; L < d; ++L) put32(kO2Header + 4 * L, (uint32_t)level_n[L]);
  put32(kO2Header + 4 * d, (uint32_t)S);
  put32(kO2Header + 4 * d + 4, (uint32_t)nc);
  for (int i = 0; i < kO2Ctx; ++i) { blob[kO2Header + 4 * d + 8 + 2 * i] = 0x00; blob[kO2Header + 4 * d + 9 + 2 * i] = 0x08; }   // 2048
  std::vector<int64_t> chunk_at;   // byte offset of every chunk
  for (int64_t c = 0; c < nc; ++c) {
    chunk_at.push_back((int64_t)blob.size());
    std::vector<uint8_t> ch(2 * 3 * kO2Lanes, 0x5A);
    uint32_t cw = 3 * kO2Lanes;
    for (int l = 0; l < kO2Lanes; ++l) {
      const uint32_t len = rnd() % 700;
      ch[4 * kO2Lanes + 2 * l] = (uint8_t)len;
      ch[4 * kO2Lanes + 2 * l + 1] = (uint8_t)(len >> 8);
      cw += len;
    }
    put32((size_t)(off_table + 4 * c), cw);
    ch.resize(2 * (size_t)cw, 0xA5);
    blob.insert(blob.end(), ch.begin(), ch.end());
  }
  put32(20, (uint32_t)(blob.size() - kO2Header));
  O2Info o;
  O2Plan pl;
  int rc = o2_parse(blob.data(), (int64_t)blob.size(), 0, true, &o, &pl);
  printf("well-formed: rc %d n %lld nodes %lld S %lld chunks %lld bytes %lld of %zu\n", rc, (long long)o.n, (long long)o.n_nodes,
         (long long)o.S, (long long)o.nc, (long long)pl.bytes, blob.size());
  if (rc != 0 || pl.bytes != (int64_t)blob.size() || pl.m != n || pl.n_dec != n_nodes) return 1;
  int64_t prev = pl.bytes;
  for (int k = 1; k <= kO2MaxLod; ++k) {   // every level from the whole blob and from exactly its own prefix
    O2Plan a, b;
    if (o2_parse(blob.data(), (int64_t)blob.size(), k, true, &o, &a) != 0) return 4;
    std::vector<uint8_t> pre(blob.begin(), blob.begin() + a.bytes);
    if (o2_parse(pre.data(), (int64_t)pre.size(), k, true, &o, &b) != 0 || b.bytes != a.bytes || b.m != a.m) return 5;
    if (a.bytes > 2 && a.n_dec > 0) {
      pre.resize(pre.size() - 2);
      std::vector<uint8_t> cut(pre.begin(), pre.end());
      if (o2_parse(cut.data(), (int64_t)cut.size(), k, true, &o, &b) == 0) return 6;   // two bytes short
    }
    if (a.bytes > prev) return 7;
    prev = a.bytes;
  }
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int lod = (int)(rnd() % 16);
    const bool need_all = rnd() % 4 != 0;
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % (blob.size() + 1)) : (int64_t)blob.size();
    std::vector<uint8_t> b(blob.begin(), blob.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (it % 7 == 0) ? 0 : 1 + (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      // the part the parser reads: header, tables, and the length tables of the chunks
      int64_t at = (int64_t)(rnd() % (uint32_t)off_payload);
      if (rnd() % 4 == 0) at = chunk_at[rnd() % chunk_at.size()] + 4 * kO2Lanes + (int64_t)(rnd() % (2 * kO2Lanes));
      if (at < (int64_t)b.size()) b[(size_t)at] ^= (uint8_t)(1u << (rnd() & 7));
    }
    O2Info q;
    O2Plan p;
    const int r = o2_parse(b.empty() ? nullptr : b.data(), (int64_t)b.size(), lod, need_all, &q, &p);
    if (r == 0) {
      ++oks;   // accepted: everything the decoder would size from must lie inside what is present and under the header's bounds
      if (need_all && p.bytes > (int64_t)b.size()) return 2;
      if (q.n == 0) {
        if (p.m != 0 || p.n_dec != 0 || p.chunks != 0) return 8;
        continue;
      }
      if (p.chunks > q.nc || p.n_dec > q.n_nodes || p.m > std::max<int64_t>(q.n, 1) || p.lanes > kO2Lanes) return 9;
      if (p.Lc >= 1 && p.m > 8 * q.level_n[p.Lc - 1]) return 10;
      if (p.n_dec > 0 && (p.chunks < 1 || p.lanes < 1 || q.off_payload + 2 * (p.last_off + p.last_words) != p.bytes)) return 11;
      if (p.n_dec > kO2Lanes * q.S * p.chunks) return 12;
    } else {
      ++errs;
    }
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 3;
}
