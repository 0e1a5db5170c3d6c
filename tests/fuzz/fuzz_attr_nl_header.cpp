// The parsers of the near-lossless attribute blobs, versions 4 and 7 (csrc/attr_blob.h attr_parse_kind and
// attr2_parse_kind with nl = true), on damaged and cut blobs at random levels: error codes, never a read outside the bytes
// given, an accepted max_error fits the value width, and an accepted plan sizes nothing beyond the bytes present.  The
// same bytes under the lossless version bytes must parse as before.  Built with -fsanitize=address,undefined by
// tests/test_fuzz_attr_nl.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"

static uint64_t seed = 777;
static uint32_t rnd() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); }

// a well-formed blob of version 1 / 4 (scal = false) or 2 / 7: n points, random lane lengths that add up to every chunk's
// word count; nl: max_error = e behind payload_len
static std::vector<uint8_t> make(bool scal, bool nl, int bpv, int c, int64_t n, uint32_t e, int64_t* words_out) {
  const int nctx = attr_contexts(bpv, c), x = nl ? 4 : 0;
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int64_t p0_at = (scal ? kAttr2Head : kAttrHead + 8) + x, head = p0_at + 2 * nctx + 4 * nc;
  std::vector<uint8_t> blob((size_t)head);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'A'; blob[1] = (uint8_t)(nl ? (scal ? 7 : 4) : (scal ? 2 : 1)); blob[2] = (uint8_t)bpv; blob[3] = (uint8_t)c;
  put32(4, (uint32_t)n);
  if (nl) put32(kAttrHead, e);
  if (scal) {
    int64_t cells = n;
    for (int k = 0; k < 16; ++k) { put32(kAttrHead + x + 4 * k, (uint32_t)cells); cells = std::max<int64_t>(1, cells / 3); }
  }
  put32(p0_at - 8, (uint32_t)S);
  put32(p0_at - 4, (uint32_t)nc);
  for (int i = 0; i < nctx; ++i) { blob[p0_at + 2 * i] = 0x00; blob[p0_at + 1 + 2 * i] = 0x08; }   // 2048
  int64_t words = 0;
  for (int64_t k = 0; k < nc; ++k) {
    std::vector<uint16_t> chunk(192, 0);
    uint32_t cw = 192;
    for (int l = 0; l < 64; ++l) { chunk[128 + l] = (uint16_t)(rnd() % 300); cw += chunk[128 + l]; }
    chunk.resize(cw, 0x5A5A);
    put32(p0_at + 2 * nctx + 4 * k, cw);
    for (uint16_t w : chunk) { blob.push_back((uint8_t)w); blob.push_back((uint8_t)(w >> 8)); }
    words += cw;
  }
  put32(8, (uint32_t)(blob.size() - kAttrHead));
  *words_out = words;
  return blob;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  int64_t w4, w7, w1, w2;
  const std::vector<uint8_t> b4 = make(false, true, 2, 2, 40000, 1000, &w4), b7 = make(true, true, 1, 3, 30000, 4, &w7);
  const std::vector<uint8_t> b1 = make(false, false, 2, 2, 40000, 0, &w1), b2 = make(true, false, 1, 3, 30000, 0, &w2);
  AttrInfo a;
  Attr2Info o;
  Attr2Plan pl;
  // well-formed: each kind under its own parser only, the lossless kinds as before
  if (attr_parse_kind(b4.data(), (int64_t)b4.size(), true, &a) != 0 || a.version != 4 || a.max_error != 1000 || a.payload_words != w4 ||
      a.off_p0 != kAttrHead + 12)
    return 1;
  if (attr_parse(b4.data(), (int64_t)b4.size(), &a) == 0 || attr_parse_kind(b1.data(), (int64_t)b1.size(), true, &a) == 0) return 9;
  if (attr_parse(b1.data(), (int64_t)b1.size(), &a) != 0 || a.version != 1 || a.max_error != 0 || a.off_p0 != kAttrHead + 8) return 10;
  if (attr2_parse(b2.data(), (int64_t)b2.size(), 3, true, &o, &pl) != 0 || o.version != 2 || o.max_error != 0) return 11;
  if (attr2_parse(b7.data(), (int64_t)b7.size(), 0, true, &o, &pl) == 0 || attr2_parse_kind(b2.data(), (int64_t)b2.size(), 0, true, true, &o, &pl) == 0)
    return 12;
  int64_t prev = (int64_t)b7.size() + 1;
  for (int lod = 0; lod <= kAttrMaxLod; ++lod) {
    if (attr2_parse_kind(b7.data(), (int64_t)b7.size(), lod, true, true, &o, &pl) != 0 || o.version != 7 || o.max_error != 4 ||
        o.payload_words != w7 || pl.bytes > prev || pl.bytes > (int64_t)b7.size())
      return 13;
    Attr2Info o2;
    Attr2Plan p2;
    std::vector<uint8_t> pre(b7.begin(), b7.begin() + pl.bytes);   // exactly the plan's bytes decode, two fewer do not
    if (attr2_parse_kind(pre.data(), (int64_t)pre.size(), lod, true, true, &o2, &p2) != 0 || p2.bytes != pl.bytes || p2.m != pl.m) return 4;
    pre.resize(pre.size() - 2);
    if (attr2_parse_kind(pre.data(), (int64_t)pre.size(), lod, true, true, &o2, &p2) == 0) return 5;
    prev = pl.bytes;
  }
  // max_error at and beyond its bounds
  for (int kind = 0; kind < 2; ++kind) {
    const int bpv = kind ? 1 : 2;
    for (uint32_t e : {0u, 1u, attr_max_error(bpv), attr_max_error(bpv) + 1u, 0xFFFFFFFFu}) {
      std::vector<uint8_t> b = kind ? b7 : b4;
      for (int i = 0; i < 4; ++i) b[kAttrHead + i] = (uint8_t)(e >> (8 * i));
      const int rc = kind ? attr2_parse_kind(b.data(), (int64_t)b.size(), 1, true, true, &o, &pl) : attr_parse_kind(b.data(), (int64_t)b.size(), true, &a);
      if ((rc == 0) != (e >= 1 && e <= attr_max_error(bpv))) return 14;
    }
  }
  printf("well-formed: version 4 %lld bytes, version 7 %lld bytes, lod 15 of it needs %lld\n", (long long)b4.size(), (long long)b7.size(),
         (long long)prev);
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const bool scal = (rnd() & 1) != 0;
    const std::vector<uint8_t>& src = scal ? b7 : b4;
    const int64_t head = scal ? kAttr2Head + 4 + 2 * attr_contexts(1, 3) : kAttrHead + 12 + 2 * attr_contexts(2, 2);
    const int lod = (int)(rnd() % 16);
    const bool need_all = (rnd() & 1) != 0;
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % src.size()) : (int64_t)src.size();
    std::vector<uint8_t> b(src.begin(), src.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const int64_t span = (rnd() & 3) ? std::min<int64_t>(head + 384, (int64_t)b.size()) : (int64_t)b.size();
      b[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
    }
    const uint8_t* p = b.empty() ? nullptr : b.data();
    if (!scal) {
      AttrInfo q;
      if (attr_parse_kind(p, (int64_t)b.size(), true, &q) != 0) { ++errs; continue; }
      ++oks;   // accepted: every size follows from the bytes present
      if (q.n > 0 && (q.version != 4 || q.max_error < 1 || q.max_error > attr_max_error(q.bpv) || q.S * q.c > kAttrMaxValues ||
                      kAttrLanes * q.S * q.nc < q.n || q.off_payload + 2 * q.payload_words != (int64_t)b.size() ||
                      q.off_table != q.off_p0 + 2 * q.nctx || q.off_p0 != kAttrHead + 12))
        return 2;
      continue;
    }
    Attr2Info q;
    Attr2Plan pn;
    if (attr2_parse_kind(p, (int64_t)b.size(), lod, need_all, true, &q, &pn) != 0) { ++errs; continue; }
    ++oks;
    if (q.n > 0) {
      if (q.version != 7 || q.max_error < 1 || q.max_error > attr_max_error(q.bpv) || q.off_p0 != kAttr2Head + 4) return 3;
      if (q.S * q.c > kAttrMaxValues || kAttrLanes * q.S * q.nc < q.n || pn.m < 1 || pn.m > q.n || pn.chunks < 1 || pn.chunks > q.nc ||
          pn.lanes < 1 || pn.lanes > kAttrLanes || (pn.chunks - 1) * kAttrLanes * q.S >= pn.m || pn.last_words < 192)
        return 6;
      if (q.off_payload + 2 * (pn.last_off + pn.last_words) != pn.bytes) return 7;
      if (need_all && pn.bytes > (int64_t)b.size()) return 8;
      if (!need_all && lod > 0 && q.off_payload + 2 * pn.last_off + 384 > (int64_t)b.size()) return 15;
    }
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 16;
}
