// The parser of the bounded-error neighbour-predicted attribute blobs, versions 28 and 31 (csrc/attr_blob.h:
// attr2_parse_kind with nbr = true and nl = true, attr_nbr_nl_kind, attr_kind12 and the four-argument attr_version), on
// damaged and cut blobs at random levels: error codes, never a read outside the bytes given, an accepted plan sizes
// nothing beyond the bytes present, an accepted max_error lies in 1 .. 2^(8 bpv - 1) - 1, an accepted mask of version 31
// is not empty and lies below the channels.  Both kinds parse under their own parser only, every other parser refuses
// them, the bounds are those of versions 7 and 14 (the same blob under the other version byte parses to the same header
// and plan at every level), and the predicates of before still know their eight and ten bytes and nothing else.  Built
// with -fsanitize=address,undefined by tests/test_fuzz_attr_nbr_nl.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"

static uint64_t seed = 2831;
static uint32_t rnd() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); }

// a well-formed blob of version `ver` (7, 14, 28 or 31; m its mask, 0 for the plain two): n points, random lane lengths
// that add up to every chunk's word count
static std::vector<uint8_t> make(int ver, int m, int bpv, int c, int64_t n, int slod, uint32_t e) {
  const int nctx = attr_contexts(bpv, c);
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int64_t p0_at = kAttr2Head + 4, head = p0_at + 2 * nctx + 4 * nc;
  std::vector<uint8_t> blob((size_t)head);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'A'; blob[1] = (uint8_t)ver; blob[2] = (uint8_t)(bpv | (slod << 4)); blob[3] = (uint8_t)(c | (m << 4));
  put32(4, (uint32_t)n);
  put32(kAttrHead, e);
  int64_t cells = n;
  for (int k = 0; k < 16; ++k) { put32(kAttrHead + 4 + 4 * k, (uint32_t)cells); cells = std::max<int64_t>(1, cells / 3); }
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
         a.max_error == b.max_error && a.off_p0 == b.off_p0 && a.off_table == b.off_table && a.off_payload == b.off_payload &&
         a.payload_words == b.payload_words && memcmp(a.cells, b.cells, sizeof(a.cells)) == 0 && p.lod == q.lod && p.m == q.m &&
         p.chunks == q.chunks && p.lanes == q.lanes && p.bytes == q.bytes && p.last_off == q.last_off && p.last_words == q.last_words;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  // all 256 version bytes: the eight and the ten of before under their predicates, 28 / 31 under the new one alone, the
  // twelve under attr_kind12
  for (int v = 0; v < 256; ++v) {
    bool s, n, x, nb, x2 = false;
    const bool eight = v == 1 || v == 2 || v == 4 || v == 7 || v == 8 || v == 11 || v == 13 || v == 14;
    const bool ten = eight || v == 25 || v == 26, two = v == 28 || v == 31;
    if (attr_kind(v, &s, &n, &x) != eight) return 20;
    if (attr_kind(v, &s, &n, &x, &nb) != ten) return 21;
    if (attr_nbr_nl_kind(v, &x2) != two || (two && x2 != (v == 31))) return 22;
    if (attr_kind12(v, &s, &n, &x, &nb) != (ten || two)) return 23;
    if ((ten || two) && attr_version(s, n, x, nb) != v) return 24;
    if (two && !(nb && s && n && x == (v == 31))) return 25;
    if (ten && (nb != (v == 25 || v == 26) || (nb && n))) return 26;
    if (attr_t_kind(v) && two) return 27;
    if ((attr_c_kind(v) || attr_s_kind(v)) && two) return 27;
  }
  // 28 and 31 differ from each of the thirteen bytes in use, and from each other, in at least two bits
  const int used[] = {1, 2, 4, 7, 8, 11, 13, 14, 19, 21, 22, 25, 26, 28, 31};
  for (int a : used)
    for (int b : {28, 31})
      if (a != b && __builtin_popcount((unsigned)(a ^ b)) < 2) return 28;
  // well-formed blobs: 7, 14, 28, 31 of the same shape.  Each parses under its own (nl, cross, nbr) only
  const int vers[4] = {7, 14, 28, 31};
  std::vector<uint8_t> kind[4];
  for (int k = 0; k < 4; ++k) {
    seed = 99;   // the same lane lengths in all four
    kind[k] = make(vers[k], (k & 1) ? 5 : 0, 1, 4, 30000, 3, 9);
  }
  for (int k = 0; k < 4; ++k)
    for (int p = 0; p < 8; ++p) {
      Attr2Info o;
      Attr2Plan pl;
      const bool nl = p & 4, cross = p & 1, nb = p & 2;
      const int rc = attr2_parse_kind(kind[k].data(), (int64_t)kind[k].size(), 2, true, nl, &o, &pl, cross, nb);
      if ((rc == 0) != (nl && (int)cross == (k & 1) && (int)nb == (k >> 1))) return 29;
      if (rc == 0 && (o.version != vers[k] || o.cross != ((k & 1) ? 5 : 0) || o.c != 4 || o.slod != 3 || o.max_error != 9)) return 30;
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
      if (attr_parse_kind(b, len, p & 1, &a, p & 2) == 0) return 31;
    if (attr_t_parse(b, len, &t) == 0 || attr_c_parse(b, len, &c) == 0 || attr_s_parse(b, len, 0, kAttrSDecode, &s, &pl) == 0) return 32;
  }
  // the bounds are those of 7 and 14: header and plan of every level agree with the same bytes under the other version
  for (int k = 2; k < 4; ++k)
    for (int lod = 0; lod < 16; ++lod) {
      Attr2Info a, b;
      Attr2Plan p, q;
      const int ra = attr2_parse_kind(kind[k].data(), (int64_t)kind[k].size(), lod, false, true, &a, &p, k & 1, true);
      const int rb = attr2_parse_kind(kind[k - 2].data(), (int64_t)kind[k - 2].size(), lod, false, true, &b, &q, k & 1, false);
      if (ra != 0 || rb != 0 || !same(a, b, p, q)) return 33;
    }
  // max_error at its ends, for both widths
  for (int bpv = 1; bpv <= 2; ++bpv)
    for (uint32_t e : {0u, 1u, attr_max_error(bpv), attr_max_error(bpv) + 1u, 0xFFFFFFFFu}) {
      seed = 7;
      const std::vector<uint8_t> b = make(28, 0, bpv, 2, 500, 0, e);
      Attr2Info o;
      Attr2Plan pl;
      const int rc = attr2_parse_kind(b.data(), (int64_t)b.size(), 0, true, true, &o, &pl, false, true);
      if ((rc == 0) != (e >= 1 && e <= attr_max_error(bpv))) return 34;
    }
  // empty frames: the 12-byte head
  {
    std::vector<uint8_t> b = {'A', 28, 1 | (2 << 4), 3, 0, 0, 0, 0, 0, 0, 0, 0};
    Attr2Info o;
    Attr2Plan pl;
    if (attr2_parse_kind(b.data(), 12, 0, true, true, &o, &pl, false, true) != 0 || o.n != 0 || o.c != 3 || o.cross != 0 || o.slod != 2 ||
        o.max_error != 0)
      return 35;
    b[3] = 0x33;
    if (attr2_parse_kind(b.data(), 12, 0, true, true, &o, &pl, false, true) == 0) return 36;   // a plain kind with a mask
    b[1] = 31;
    if (attr2_parse_kind(b.data(), 12, 0, true, true, &o, &pl, true, true) != 0 || o.cross != 3 || o.c != 3) return 37;
    b[3] = 0x03;
    if (attr2_parse_kind(b.data(), 12, 0, true, true, &o, &pl, true, true) == 0) return 38;    // a cross kind without one
    b[3] = 0x33;
    b[8] = 1;
    if (attr2_parse_kind(b.data(), 12, 0, true, true, &o, &pl, true, true) == 0) return 39;    // no points, a payload
  }
  printf("well-formed: version 28 %lld bytes, 31 %lld\n", (long long)kind[2].size(), (long long)kind[3].size());
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int k = 2 + (int)(rnd() & 1);
    const bool cross = k & 1;
    const std::vector<uint8_t>& src = kind[k];
    const int64_t head = kAttr2Head + 4 + 2 * attr_contexts(1, 4);
    const int lod = (int)(rnd() % 16);
    const bool need_all = (rnd() & 1) != 0;
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % src.size()) : (int64_t)src.size();
    std::vector<uint8_t> b(src.begin(), src.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const uint32_t where = rnd() & 7;
      const int64_t span = where == 0 ? (int64_t)b.size() : (where < 3 ? std::min<int64_t>(16, (int64_t)b.size()) : std::min<int64_t>(head + 384, (int64_t)b.size()));
      b[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
    }
    const uint8_t* p = b.empty() ? nullptr : b.data();
    Attr2Info q;
    Attr2Plan pn;
    if (attr2_parse_kind(p, (int64_t)b.size(), lod, need_all, true, &q, &pn, cross, true) != 0) { ++errs; continue; }
    ++oks;   // accepted: every size follows from the bytes present
    if (q.version != (cross ? 31 : 28) || q.c < 1 || q.c > 4) return 4;
    if (cross ? (q.c < 2 || q.cross < 1 || q.cross >= (1 << (q.c - 1))) : q.cross != 0) return 5;
    if (q.n > 0) {
      if (q.max_error < 1 || q.max_error > attr_max_error(q.bpv)) return 11;
      if (q.off_p0 != kAttr2Head + 4 || q.nctx != attr_contexts(q.bpv, q.c)) return 6;
      if (q.S * q.c > kAttrMaxValues || kAttrLanes * q.S * q.nc < q.n || pn.m < 1 || pn.m > q.n || pn.chunks < 1 || pn.chunks > q.nc ||
          pn.lanes < 1 || pn.lanes > kAttrLanes || (pn.chunks - 1) * kAttrLanes * q.S >= pn.m || pn.last_words < 192)
        return 7;
      if (q.off_payload + 2 * (pn.last_off + pn.last_words) != pn.bytes) return 8;
      if (need_all && pn.bytes > (int64_t)b.size()) return 9;
      if (!need_all && lod > 0 && q.off_payload + 2 * pn.last_off + 384 > (int64_t)b.size()) return 15;
      for (int j = 1; j < 16; ++j)
        if (q.cells[j] < 1 || q.cells[j] > q.cells[j - 1]) return 10;
      // the same bytes under 7 / 14 are accepted to the same header and plan
      std::vector<uint8_t> t = b;
      t[1] = (uint8_t)(cross ? 14 : 7);
      Attr2Info q7;
      Attr2Plan p7;
      if (attr2_parse_kind(t.data(), (int64_t)t.size(), lod, need_all, true, &q7, &p7, cross, false) != 0 || !same(q, q7, pn, p7)) return 12;
    }
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 16;
}
