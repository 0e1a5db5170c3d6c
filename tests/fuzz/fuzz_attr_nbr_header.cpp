// The parser of the neighbour-predicted attribute blobs, versions 25 and 26 (csrc/attr_blob.h: attr2_parse_kind with
// nbr = true, the five-argument attr_kind / four-argument attr_version), on damaged and cut blobs at random levels: error
// codes, never a read outside the bytes given, an accepted plan sizes nothing beyond the bytes present, an accepted mask
// of version 26 is not empty and lies below the channels.  Both kinds parse under their own parser only, every other
// parser refuses them, the bounds are those of versions 2 and 11 (the same blob under the other version byte parses to
// the same header and plan), and the eight-kind attr_kind still knows its eight bytes and nothing else.  Built with
// -fsanitize=address,undefined by tests/test_fuzz_attr_nbr.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"

static uint64_t seed = 2526;
static uint32_t rnd() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); }

// a well-formed blob of version `ver` (2, 11, 25 or 26; m its mask, 0 for the plain two): n points, random lane lengths
// that add up to every chunk's word count
static std::vector<uint8_t> make(int ver, int m, int bpv, int c, int64_t n, int slod) {
  const int nctx = attr_contexts(bpv, c);
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int64_t p0_at = kAttr2Head, head = p0_at + 2 * nctx + 4 * nc;
  std::vector<uint8_t> blob((size_t)head);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'A'; blob[1] = (uint8_t)ver; blob[2] = (uint8_t)(bpv | (slod << 4)); blob[3] = (uint8_t)(c | (m << 4));
  put32(4, (uint32_t)n);
  int64_t cells = n;
  for (int k = 0; k < 16; ++k) { put32(kAttrHead + 4 * k, (uint32_t)cells); cells = std::max<int64_t>(1, cells / 3); }
  put32(p0_at - 8, (uint32_t)S);
  put32(p0_at - 4, (uint32_t)nc);
  for (int i = 0; i < nctx; ++i) { blob[p0_at + 2 * i] = 0x00; blob[p0_at + 1 + 2 * i] = 0x08; }   // 2048
  for (int64_t k = 0; k < nc; ++k) {
    std::vector<uint16_t> chunk(192, 0);
    uint32_t cw = 192;
    for (int l = 0; l < 64; ++l) { chunk[128 + l] = (uint16_t)(rnd() % 300); cw += chunk[128 + l]; }
    chunk.resize(cw, 0x5A5A);
    put32(p0_at + 2 * nctx + 4 * k, cw);
    for (uint16_t w : chunk) { blob.push_back((uint8_t)w); blob.push_back((uint8_t)(w >> 8)); }
  }
  put32(8, (uint32_t)(blob.size() - kAttrHead));
  return blob;
}

static bool same(const Attr2Info& a, const Attr2Info& b, const Attr2Plan& p, const Attr2Plan& q) {
  return a.bpv == b.bpv && a.c == b.c && a.cross == b.cross && a.slod == b.slod && a.n == b.n && a.S == b.S && a.nc == b.nc &&
         a.off_p0 == b.off_p0 && a.off_table == b.off_table && a.off_payload == b.off_payload && a.payload_words == b.payload_words &&
         memcmp(a.cells, b.cells, sizeof(a.cells)) == 0 && p.lod == q.lod && p.m == q.m && p.chunks == q.chunks && p.lanes == q.lanes &&
         p.bytes == q.bytes && p.last_off == q.last_off && p.last_words == q.last_words;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  // the version bytes: the eight of before under the old predicate, those and 25 / 26 under the new one
  for (int v = 0; v < 256; ++v) {
    bool s, n, x, nb;
    const bool eight = v == 1 || v == 2 || v == 4 || v == 7 || v == 8 || v == 11 || v == 13 || v == 14;
    if (attr_kind(v, &s, &n, &x) != eight) return 20;
    if (attr_kind(v, &s, &n, &x, &nb) != (eight || v == 25 || v == 26)) return 21;
    if ((eight || v == 25 || v == 26) && attr_version(s, n, x, nb) != v) return 22;
    if ((v == 25 || v == 26) && !(nb && s && !n && x == (v == 26))) return 23;
    if (eight && (nb || attr_version(s, n, x) != v)) return 24;
  }
  // 25 and 26 differ from each of the eleven bytes in use, and from each other, in at least two bits
  const int used[] = {1, 2, 4, 7, 8, 11, 13, 14, 19, 21, 22, 25, 26};
  for (int a : used)
    for (int b : {25, 26})
      if (a != b && __builtin_popcount((unsigned)(a ^ b)) < 2) return 25;
  // well-formed blobs: 2, 11, 25, 26 of the same shape.  Each parses under its own (cross, nbr) only
  const int vers[4] = {2, 11, 25, 26};
  std::vector<uint8_t> kind[4];
  for (int k = 0; k < 4; ++k) {
    seed = 99;   // the same lane lengths in all four
    kind[k] = make(vers[k], (k & 1) ? 5 : 0, 1, 4, 30000, 3);
  }
  for (int k = 0; k < 4; ++k)
    for (int p = 0; p < 8; ++p) {
      Attr2Info o;
      Attr2Plan pl;
      const bool nl = p & 4, cross = p & 1, nb = p & 2;
      const int rc = attr2_parse_kind(kind[k].data(), (int64_t)kind[k].size(), 2, true, nl, &o, &pl, cross, nb);
      if ((rc == 0) != (!nl && (int)cross == (k & 1) && (int)nb == (k >> 1))) return 26;
      if (rc == 0 && (o.version != vers[k] || o.cross != ((k & 1) ? 5 : 0) || o.c != 4 || o.slod != 3 || o.max_error != 0)) return 27;
    }
  // the other parsers refuse both bytes
  for (int k = 2; k < 4; ++k) {
    AttrInfo a;
    AttrTInfo t;
    AttrCInfo c;
    AttrSInfo s;
    Attr2Plan pl;
    const uint8_t* b = kind[k].data();
    const int64_t len = (int64_t)kind[k].size();
    for (int p = 0; p < 4; ++p)
      if (attr_parse_kind(b, len, p & 1, &a, p & 2) == 0) return 28;
    if (attr_t_parse(b, len, &t) == 0 || attr_c_parse(b, len, &c) == 0 || attr_s_parse(b, len, 0, kAttrSDecode, &s, &pl) == 0) return 29;
  }
  // the bounds are those of 2 and 11: header and plan of every level agree with the same bytes under the other version
  for (int k = 2; k < 4; ++k)
    for (int lod = 0; lod < 16; ++lod) {
      Attr2Info a, b;
      Attr2Plan p, q;
      const int ra = attr2_parse_kind(kind[k].data(), (int64_t)kind[k].size(), lod, false, false, &a, &p, k & 1, true);
      const int rb = attr2_parse_kind(kind[k - 2].data(), (int64_t)kind[k - 2].size(), lod, false, false, &b, &q, k & 1, false);
      if (ra != 0 || rb != 0 || !same(a, b, p, q)) return 30;
    }
  // empty frames: the 12-byte head
  {
    std::vector<uint8_t> b = {'A', 25, 1 | (2 << 4), 3, 0, 0, 0, 0, 0, 0, 0, 0};
    Attr2Info o;
    Attr2Plan pl;
    if (attr2_parse_kind(b.data(), 12, 0, true, false, &o, &pl, false, true) != 0 || o.n != 0 || o.c != 3 || o.cross != 0 || o.slod != 2) return 31;
    b[3] = 0x33;
    if (attr2_parse_kind(b.data(), 12, 0, true, false, &o, &pl, false, true) == 0) return 32;   // a plain kind with a mask
    b[1] = 26;
    if (attr2_parse_kind(b.data(), 12, 0, true, false, &o, &pl, true, true) != 0 || o.cross != 3 || o.c != 3) return 33;
    b[3] = 0x03;
    if (attr2_parse_kind(b.data(), 12, 0, true, false, &o, &pl, true, true) == 0) return 34;    // a cross kind without one
    b[8] = 1;
    if (attr2_parse_kind(b.data(), 12, 0, true, false, &o, &pl, true, true) == 0) return 35;    // no points, a payload
    if (attr2_parse_kind(b.data(), 12, 0, true, true, &o, &pl, true, true) == 0) return 36;     // no near-lossless form
  }
  printf("well-formed: version 25 %lld bytes, 26 %lld\n", (long long)kind[2].size(), (long long)kind[3].size());
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int k = 2 + (int)(rnd() & 1);
    const bool cross = k & 1;
    const std::vector<uint8_t>& src = kind[k];
    const int64_t head = kAttr2Head + 2 * attr_contexts(1, 4);
    const int lod = (int)(rnd() % 16);
    const bool need_all = (rnd() & 1) != 0;
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % src.size()) : (int64_t)src.size();
    std::vector<uint8_t> b(src.begin(), src.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const uint32_t where = rnd() & 7;
      const int64_t span = where == 0 ? (int64_t)b.size() : (where < 3 ? std::min<int64_t>(4, (int64_t)b.size()) : std::min<int64_t>(head + 384, (int64_t)b.size()));
      b[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
    }
    const uint8_t* p = b.empty() ? nullptr : b.data();
    Attr2Info q;
    Attr2Plan pn;
    if (attr2_parse_kind(p, (int64_t)b.size(), lod, need_all, false, &q, &pn, cross, true) != 0) { ++errs; continue; }
    ++oks;   // accepted: every size follows from the bytes present
    if (q.version != (cross ? 26 : 25) || q.c < 1 || q.c > 4 || q.max_error != 0) return 4;
    if (cross ? (q.c < 2 || q.cross < 1 || q.cross >= (1 << (q.c - 1))) : q.cross != 0) return 5;
    if (q.n > 0) {
      if (q.off_p0 != kAttr2Head || q.nctx != attr_contexts(q.bpv, q.c)) return 6;
      if (q.S * q.c > kAttrMaxValues || kAttrLanes * q.S * q.nc < q.n || pn.m < 1 || pn.m > q.n || pn.chunks < 1 || pn.chunks > q.nc ||
          pn.lanes < 1 || pn.lanes > kAttrLanes || (pn.chunks - 1) * kAttrLanes * q.S >= pn.m || pn.last_words < 192)
        return 7;
      if (q.off_payload + 2 * (pn.last_off + pn.last_words) != pn.bytes) return 8;
      if (need_all && pn.bytes > (int64_t)b.size()) return 9;
      if (!need_all && lod > 0 && q.off_payload + 2 * pn.last_off + 384 > (int64_t)b.size()) return 15;
      for (int j = 1; j < 16; ++j)
        if (q.cells[j] < 1 || q.cells[j] > q.cells[j - 1]) return 10;
    }
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 16;
}
