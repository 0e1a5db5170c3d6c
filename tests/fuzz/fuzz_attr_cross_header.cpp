// The parsers of the cross-channel attribute blobs, versions 8, 11, 13 and 14 (csrc/attr_blob.h attr_parse_kind and
// attr2_parse_kind with cross = true, attr_kind, attr_channels), on damaged and cut blobs at random levels: error codes,
// never a read outside the bytes given, an accepted mask is not empty and lies below the channels, and an accepted plan
// sizes nothing beyond the bytes present.  Every kind parses under its own parser only, a plain kind with anything above
// the channels of byte 3 is refused, and the plain kinds parse as before.  Built with -fsanitize=address,undefined by
// tests/test_fuzz_attr_cross.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"

static uint64_t seed = 4242;
static uint32_t rnd() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); }

// a well-formed blob of the kind (scal, nl, mask m; m = 0: the plain kind): n points, random lane lengths that add up to
// every chunk's word count
static std::vector<uint8_t> make(bool scal, bool nl, int m, int bpv, int c, int64_t n, uint32_t e) {
  const int nctx = attr_contexts(bpv, c), x = nl ? 4 : 0;
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int64_t p0_at = (scal ? kAttr2Head : kAttrHead + 8) + x, head = p0_at + 2 * nctx + 4 * nc;
  std::vector<uint8_t> blob((size_t)head);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'A'; blob[1] = (uint8_t)attr_version(scal, nl, m != 0); blob[2] = (uint8_t)bpv; blob[3] = (uint8_t)(c | (m << 4));
  put32(4, (uint32_t)n);
  if (nl) put32(kAttrHead, e);
  if (scal) {
    int64_t cells = n;
    for (int k = 0; k < 16; ++k) { put32(kAttrHead + x + 4 * k, (uint32_t)cells); cells = std::max<int64_t>(1, cells / 3); }
  }
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

static int parse(const std::vector<uint8_t>& b, bool scal, bool nl, bool cross, int lod, AttrInfo* a) {
  if (!scal) return attr_parse_kind(b.data(), (int64_t)b.size(), nl, a, cross);
  Attr2Info o;
  Attr2Plan pl;
  const int rc = attr2_parse_kind(b.data(), (int64_t)b.size(), lod, true, nl, &o, &pl, cross);
  *a = o;
  return rc;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  // the eight version bytes and nothing else
  for (int v = 0; v < 256; ++v) {
    bool s, n, x;
    const bool valid = v == 1 || v == 2 || v == 4 || v == 7 || v == 8 || v == 11 || v == 13 || v == 14;
    if (attr_kind(v, &s, &n, &x) != valid) return 20;
    if (valid && attr_version(s, n, x) != v) return 21;
  }
  // byte 3: a cross kind needs a mask that is not empty and has no bit at c - 1 or above; a plain kind nothing above c
  for (int b3 = 0; b3 < 256; ++b3) {
    int c, m;
    const int lo = b3 & 15, hi = b3 >> 4;
    if (attr_channels((uint8_t)b3, true, &c, &m) != (lo >= 2 && lo <= 4 && hi != 0 && hi < (1 << (lo - 1)))) return 22;
    if (attr_channels((uint8_t)b3, false, &c, &m) != (b3 >= 1 && b3 <= 4)) return 23;
  }
  // well-formed blobs of the eight kinds: each under its own parser only
  std::vector<uint8_t> kind[8];
  for (int k = 0; k < 8; ++k) {
    const bool scal = k & 1, nl = k & 2, cross = k & 4;
    kind[k] = scal ? make(true, nl, cross ? 5 : 0, 1, 4, 30000, 4) : make(false, nl, cross ? 2 : 0, 2, 3, 40000, 1000);
  }
  for (int k = 0; k < 8; ++k)
    for (int p = 0; p < 8; ++p) {
      AttrInfo a;
      const int rc = parse(kind[k], p & 1, p & 2, p & 4, 2, &a);
      if ((rc == 0) != (k == p)) return 24;
      if (rc == 0 && (a.version != attr_version(k & 1, k & 2, k & 4) || a.cross != ((k & 4) ? ((k & 1) ? 5 : 2) : 0) || a.c != ((k & 1) ? 4 : 3)))
        return 25;
    }
  // every byte 3 over the well-formed cross blobs, and over the plain ones
  for (int k = 0; k < 8; ++k)
    for (int b3 = 0; b3 < 256; ++b3) {
      std::vector<uint8_t> b = kind[k];
      const int c0 = (k & 1) ? 4 : 3;
      b[3] = (uint8_t)b3;
      AttrInfo a;
      const int rc = parse(b, k & 1, k & 2, k & 4, 1, &a);
      const int lo = (k & 4) ? b3 & 15 : b3, hi = (k & 4) ? b3 >> 4 : 0;
      // another channel count moves the table: only the blob's own count can parse
      const bool want = lo == c0 && ((k & 4) ? (hi != 0 && hi < (1 << (lo - 1))) : true);
      if ((rc == 0) != want) return 26;
      if (rc == 0 && (a.c != c0 || a.cross != hi)) return 27;
    }
  // empty frames: the 12-byte head
  for (int k = 4; k < 8; ++k) {
    std::vector<uint8_t> b = {'A', (uint8_t)attr_version(k & 1, k & 2, true), 1, 0x33, 0, 0, 0, 0, 0, 0, 0, 0};
    AttrInfo a;
    if (parse(b, k & 1, k & 2, true, 0, &a) != 0 || a.n != 0 || a.cross != 3 || a.c != 3) return 28;
    b[3] = 0x03;
    if (parse(b, k & 1, k & 2, true, 0, &a) == 0) return 29;
    b[3] = 0x43;
    if (parse(b, k & 1, k & 2, true, 0, &a) == 0) return 30;
  }
  printf("well-formed: version 8 %lld bytes, 11 %lld, 13 %lld, 14 %lld\n", (long long)kind[4].size(), (long long)kind[5].size(),
         (long long)kind[6].size(), (long long)kind[7].size());
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int k = 4 + (int)(rnd() & 3);
    const bool scal = k & 1, nl = k & 2;
    const std::vector<uint8_t>& src = kind[k];
    const int64_t head = (scal ? kAttr2Head + 2 * attr_contexts(1, 4) : kAttrHead + 8 + 2 * attr_contexts(2, 3)) + (nl ? 4 : 0);
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
    if (!scal) {
      AttrInfo q;
      if (attr_parse_kind(p, (int64_t)b.size(), nl, &q, true) != 0) { ++errs; continue; }
      ++oks;   // accepted: every size follows from the bytes present, and the mask fits the channels
      if (q.version != attr_version(false, nl, true) || q.c < 2 || q.c > 4 || q.cross < 1 || q.cross >= (1 << (q.c - 1))) return 2;
      if (q.n > 0 && (q.S * q.c > kAttrMaxValues || kAttrLanes * q.S * q.nc < q.n || q.off_payload + 2 * q.payload_words != (int64_t)b.size() ||
                      q.off_table != q.off_p0 + 2 * q.nctx || q.off_p0 != kAttrHead + 8 + (nl ? 4 : 0) || q.nctx != attr_contexts(q.bpv, q.c)))
        return 3;
      continue;
    }
    Attr2Info q;
    Attr2Plan pn;
    if (attr2_parse_kind(p, (int64_t)b.size(), lod, need_all, nl, &q, &pn, true) != 0) { ++errs; continue; }
    ++oks;
    if (q.version != attr_version(true, nl, true) || q.c < 2 || q.c > 4 || q.cross < 1 || q.cross >= (1 << (q.c - 1))) return 4;
    if (q.n > 0) {
      if (q.off_p0 != kAttr2Head + (nl ? 4 : 0) || q.nctx != attr_contexts(q.bpv, q.c)) return 5;
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
