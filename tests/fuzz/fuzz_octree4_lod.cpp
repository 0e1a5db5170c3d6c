// The level-of-detail plan of a version-4 octree blob (csrc/octree4_blob.h, o4_parse_lod) on a blob cut at every length
// and on mutated headers: error codes or plans whose bytes lie inside the blob (inside the bytes present, in the
// decoder's form), never a read outside the bytes present.  Built with -fsanitize=address,undefined by
// tests/test_octree_inter_lod.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "octree4_blob.h"

// what an accepted plan promises, whatever the bytes were: 0, or the number of the promise it breaks
static int broken(const O4Info& q, const O4Plan& pl, int lod, bool need_all, int64_t len) {
  if (q.n < 1 || q.depth < 1 || q.depth > 16 || q.S < 4 || q.S > kO4SLimit || q.S % 4 || q.nc < 1) return 20;
  if (kO4Lanes * q.S * q.nc < q.n_nodes || kO4Lanes * q.S * (q.nc - 1) >= q.n_nodes) return 21;
  if (q.off_table + 4 * q.nc != q.off_payload || q.off_payload > len) return 22;
  if (pl.lod != lod) return 23;
  if (lod == 0) return pl.bytes == len && q.off_payload + 2 * q.payload_words == len && pl.m == q.n && pl.n_dec == q.n_nodes ? 0 : 24;
  const int Lc = q.depth > lod ? q.depth - lod : 0;
  if (pl.Lc != Lc || pl.m != (Lc ? q.level_n[Lc] : 1) || pl.m < 1 || pl.m > q.n) return 25;
  int64_t nd = 0;
  for (int L = 0; L < Lc; ++L) nd += q.level_n[L];
  if (pl.n_dec != nd || nd >= q.n_nodes) return 26;
  if (pl.bytes > q.off_payload + 2 * q.payload_words) return 27;   // never more than the blob
  if (need_all && pl.bytes > len) return 28;                       // the decoder's form: all of it present
  if (nd == 0) return pl.bytes == q.off_payload && pl.chunks == 0 ? 0 : 29;
  if (pl.chunks < 1 || pl.chunks > q.nc || pl.lanes < 1 || pl.lanes > kO4Lanes) return 30;
  if (((pl.chunks - 1) * kO4Lanes + pl.lanes) * q.S < nd || ((pl.chunks - 1) * kO4Lanes + pl.lanes - 1) * q.S >= nd) return 31;
  if (pl.last_words < 3 * kO4Lanes || pl.bytes != q.off_payload + 2 * (pl.last_off + pl.last_words)) return 32;
  if (q.off_payload + 2 * (pl.last_off + 3 * kO4Lanes) > len) return 33;   // the length table it was computed from is present
  return 0;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  uint64_t seed = 4245;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  // a well-formed blob: depth 9, 90000 points, 128 nodes per lane (10 chunks), short random runs
  const int d = 9;
  const int64_t level_n[d] = {1, 8, 30, 100, 400, 1500, 6000, 20000, 50000}, n = 90000, S = 128;
  int64_t n_nodes = 0;
  for (int L = 0; L < d; ++L) n_nodes += level_n[L];
  const int64_t nc = (n_nodes + kO4Lanes * S - 1) / (kO4Lanes * S);
  const int64_t off_p0 = kO4Header + 4 * d + 20, off_table = off_p0 + 2 * kO4Ctx, off_payload = off_table + 4 * nc;
  std::vector<uint8_t> blob((size_t)off_payload);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'O'; blob[1] = 4; blob[2] = d; blob[3] = 2;
  put32(4, (uint32_t)n);
  put32(8, (uint32_t)-512); put32(12, 1024u); put32(16, (uint32_t)-32768);
  for (int L = 0; L < d; ++L) put32(kO4Header + 4 * L, (uint32_t)level_n[L]);
  put32(kO4Header + 4 * d, (uint32_t)S);
  put32(kO4Header + 4 * d + 4, (uint32_t)nc);
  put32(kO4Header + 4 * d + 8, 88888u);
  put32(kO4Header + 4 * d + 12, 0x89ABCDEFu); put32(kO4Header + 4 * d + 16, 0x01234567u);
  for (int i = 0; i < kO4Ctx; ++i) { blob[off_p0 + 2 * i] = 0x00; blob[off_p0 + 2 * i + 1] = 0x08; }
  for (int64_t c = 0; c < nc; ++c) {
    std::vector<uint8_t> ch(2 * 3 * kO4Lanes, 0x5A);
    uint32_t cw = 3 * kO4Lanes;
    for (int l = 0; l < kO4Lanes; ++l) {
      const uint32_t len = rnd() % 12;
      ch[4 * kO4Lanes + 2 * l] = (uint8_t)len;
      ch[4 * kO4Lanes + 2 * l + 1] = 0;
      cw += len;
    }
    put32((size_t)(off_table + 4 * c), cw);
    ch.resize(2 * (size_t)cw, 0xA5);
    blob.insert(blob.end(), ch.begin(), ch.end());
  }
  put32(20, (uint32_t)(blob.size() - kO4Header));
  const int64_t whole = (int64_t)blob.size();
  // the plans of the whole blob: what every long enough prefix must answer with
  O4Info o;
  O4Plan want[16];
  for (int k = 0; k <= 15; ++k) {
    if (o4_parse_lod(blob.data(), whole, k, true, &o, &want[k]) != 0 || broken(o, want[k], k, true, whole)) return 1;
    if (k > 1 && want[k].bytes > want[k - 1].bytes) return 2;   // a coarser level never needs more
  }
  printf("well-formed: %lld bytes, %lld chunks; lod 1 / 2 / 4 / 9 need %lld / %lld / %lld / %lld bytes\n", (long long)whole, (long long)nc,
         (long long)want[1].bytes, (long long)want[2].bytes, (long long)want[4].bytes, (long long)want[9].bytes);
  if (want[1].chunks < 2 || want[9].n_dec != 0 || want[8].n_dec != 1) return 3;
  // cut at every length, every lod, both forms
  int64_t oks = 0, errs = 0;
  for (int64_t cut = 0; cut <= whole; ++cut) {
    std::vector<uint8_t> b(blob.begin(), blob.begin() + cut);   // exactly the bytes the parser may read
    for (int k = 0; k <= 15; ++k)
      for (int form = 0; form < 2; ++form) {
        O4Info q;
        O4Plan pl;
        const bool need_all = form == 1;
        const int r = o4_parse_lod(b.empty() ? nullptr : b.data(), cut, k, need_all, &q, &pl);
        // the decoder's form accepts exactly the prefixes that hold the plan's bytes; the other form needs no more
        if (need_all && (r == 0) != (cut >= want[k].bytes)) return 4;
        if (!need_all && k > 0 && r != 0 && cut >= want[k].bytes) return 5;
        if (r != 0) {
          ++errs;
          continue;
        }
        ++oks;
        const int why = broken(q, pl, k, need_all, cut);
        if (why) return why;
        if (pl.bytes != want[k].bytes || pl.m != want[k].m || pl.n_dec != want[k].n_dec) return 6;   // the blob's own plan
      }
  }
  printf("cuts: %lld accepted, %lld refused\n", (long long)oks, (long long)errs);
  if (!oks || !errs) return 7;
  // mutated headers and tables, cut or whole
  oks = errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % (blob.size() + 1)) : whole;
    std::vector<uint8_t> b(blob.begin(), blob.begin() + cut);
    const int flips = 1 + (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      // the head, the tables, or the length table of some chunk: everything a plan is computed from
      int64_t at = (int64_t)(rnd() % (uint32_t)off_payload);
      if (rnd() % 4 == 0) at = off_payload + (int64_t)(rnd() % (uint32_t)(whole - off_payload));
      if (at < (int64_t)b.size()) b[(size_t)at] ^= (uint8_t)(1u << (rnd() & 7));
    }
    if (it % 11 == 0 && b.size() >= 24) {   // a cut blob whose announced length was made to fit
      const uint32_t pay = (uint32_t)(b.size() - kO4Header);
      for (int i = 0; i < 4; ++i) b[20 + i] = (uint8_t)(pay >> (8 * i));
    }
    const int k = (int)(rnd() % 16);
    const bool need_all = (rnd() & 1) != 0;
    O4Info q;
    O4Plan pl;
    const int r = o4_parse_lod(b.empty() ? nullptr : b.data(), (int64_t)b.size(), k, need_all, &q, &pl);
    if (r != 0) {
      ++errs;
      continue;
    }
    ++oks;
    const int why = broken(q, pl, k, need_all, (int64_t)b.size());
    if (why) return 100 + why;
  }
  printf("fuzz: %lld accepted, %lld refused\n", (long long)oks, (long long)errs);
  return errs > 0 && oks > 0 ? 0 : 8;
}
