// The parser of attribute blob version 2 and its level-of-detail plan (csrc/attr_blob.h attr2_parse) on damaged and cut
// blobs at random levels: error codes, never a read outside the bytes given, and an accepted plan sizes nothing beyond
// them.  Built with -fsanitize=address,undefined by tests/test_fuzz_attr2.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"
int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  uint64_t seed = 4242;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  // a well-formed blob: 3 channels of uint8, n = 30000 points (several chunks), cells shrinking by 3 per level, random
  // lane lengths that add up to every chunk's word count
  const int bpv = 1, c = 3, nctx = attr_contexts(bpv, c);
  const int64_t n = 30000;
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int64_t head = kAttr2Head + 2 * nctx + 4 * nc;
  std::vector<uint8_t> blob((size_t)head);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'A'; blob[1] = 2; blob[2] = bpv; blob[3] = c;
  put32(4, (uint32_t)n);
  int64_t cells = n;
  for (int k = 0; k < 16; ++k) { put32(kAttrHead + 4 * k, (uint32_t)cells); cells = std::max<int64_t>(1, cells / 3); }
  put32(kAttrHead + 64, (uint32_t)S);
  put32(kAttrHead + 68, (uint32_t)nc);
  for (int i = 0; i < nctx; ++i) { blob[kAttr2Head + 2 * i] = 0x00; blob[kAttr2Head + 1 + 2 * i] = 0x08; }   // 2048
  int64_t words = 0;
  for (int64_t k = 0; k < nc; ++k) {
    std::vector<uint16_t> chunk(192, 0);
    uint32_t cw = 192;
    for (int l = 0; l < 64; ++l) { chunk[128 + l] = (uint16_t)(rnd() % 300); cw += chunk[128 + l]; }
    chunk.resize(cw, 0x5A5A);
    put32(kAttr2Head + 2 * nctx + 4 * k, cw);
    for (uint16_t w : chunk) { blob.push_back((uint8_t)w); blob.push_back((uint8_t)(w >> 8)); }
    words += cw;
  }
  put32(8, (uint32_t)(blob.size() - kAttrHead));
  Attr2Info o;
  Attr2Plan pl;
  int64_t prev = (int64_t)blob.size() + 1;
  for (int lod = 0; lod <= kAttrMaxLod; ++lod) {
    const int rc = attr2_parse(blob.data(), (int64_t)blob.size(), lod, true, &o, &pl);
    if (rc != 0 || o.payload_words != words || pl.bytes > prev || pl.bytes > (int64_t)blob.size()) return 1;
    // exactly the plan's bytes decode, two fewer do not; the info form needs the length table only
    Attr2Info o2;
    Attr2Plan p2;
    std::vector<uint8_t> pre(blob.begin(), blob.begin() + pl.bytes);
    if (attr2_parse(pre.data(), (int64_t)pre.size(), lod, true, &o2, &p2) != 0 || p2.bytes != pl.bytes || p2.m != pl.m) return 4;
    pre.resize(pre.size() - 2);
    if (attr2_parse(pre.data(), (int64_t)pre.size(), lod, true, &o2, &p2) == 0) return 5;
    prev = pl.bytes;
  }
  printf("well-formed: n %lld S %lld chunks %lld words %lld, lod 4 needs %lld of %lld bytes\n", (long long)o.n, (long long)o.S,
         (long long)o.nc, (long long)o.payload_words, (long long)prev, (long long)blob.size());
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int lod = (int)(rnd() % 16);
    const bool need_all = (rnd() & 1) != 0;
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % blob.size()) : (int64_t)blob.size();
    std::vector<uint8_t> b(blob.begin(), blob.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const int64_t span = (rnd() & 3) ? std::min<int64_t>(head + 384, (int64_t)b.size()) : (int64_t)b.size();
      b[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
    }
    Attr2Info q;
    Attr2Plan p;
    const int r = attr2_parse(b.empty() ? nullptr : b.data(), (int64_t)b.size(), lod, need_all, &q, &p);
    if (r == 0) {
      ++oks;   // accepted: everything the decoder would size from or upload must lie inside the bytes present
      if (q.n > 0) {
        if (q.S * q.c > kAttrMaxValues || kAttrLanes * q.S * q.nc < q.n || p.m < 1 || p.m > q.n || p.chunks < 1 || p.chunks > q.nc ||
            p.lanes < 1 || p.lanes > kAttrLanes || (p.chunks - 1) * kAttrLanes * q.S >= p.m || p.last_words < 192)
          return 2;
        if (q.off_payload + 2 * (p.last_off + p.last_words) != p.bytes) return 6;
        if (need_all && p.bytes > (int64_t)b.size()) return 7;
        if (!need_all && lod > 0 && q.off_payload + 2 * p.last_off + 384 > (int64_t)b.size()) return 8;
      }
    } else {
      ++errs;
    }
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 3;
}
