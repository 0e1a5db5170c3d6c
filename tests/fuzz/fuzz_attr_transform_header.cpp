// The parser of the transform-coded attribute blob, version 19 (csrc/attr_blob.h attr_t_parse, attr_t_kind), on damaged
// and cut blobs, whole and as prefixes: error codes, never a read outside the bytes given, an accepted q lies in
// 1 .. H - 1 and every accepted size follows from the bytes present.  Byte 19 is refused by the eight other parsers and
// the eight other bytes by this one; attr_kind still knows exactly its eight.  Built with -fsanitize=address,undefined by
// tests/test_fuzz_attr_transform.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"

static uint64_t seed = 1919;
static uint32_t rnd() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); }

static void put32(std::vector<uint8_t>& blob, size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); }

// the body behind the head of any kind: p0, a chunk table and chunks whose random lane lengths add up
static void body(std::vector<uint8_t>& blob, int64_t p0_at, int nctx, int64_t nc) {
  blob.resize((size_t)(p0_at + 2 * nctx + 4 * nc));
  for (int i = 0; i < nctx; ++i) { blob[p0_at + 2 * i] = 0x00; blob[p0_at + 1 + 2 * i] = 0x08; }   // 2048
  for (int64_t k = 0; k < nc; ++k) {
    std::vector<uint16_t> chunk(192, 0);
    uint32_t cw = 192;
    for (int l = 0; l < 64; ++l) { chunk[128 + l] = (uint16_t)(rnd() % 300); cw += chunk[128 + l]; }
    chunk.resize(cw, 0x5A5A);
    put32(blob, (size_t)(p0_at + 2 * nctx + 4 * k), cw);
    for (uint16_t w : chunk) { blob.push_back((uint8_t)w); blob.push_back((uint8_t)(w >> 8)); }
  }
  put32(blob, 8, (uint32_t)(blob.size() - kAttrHead));
}

// a well-formed version-19 blob
static std::vector<uint8_t> make_t(int bpv, int slod, int c, int64_t n, uint32_t q) {
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  std::vector<uint8_t> blob((size_t)kAttrTHead);
  blob[0] = 'A'; blob[1] = 19; blob[2] = (uint8_t)(bpv | (slod << 4)); blob[3] = (uint8_t)c;
  put32(blob, 4, (uint32_t)n);
  put32(blob, kAttrHead, q);
  put32(blob, kAttrHead + 4, (uint32_t)S);
  put32(blob, kAttrHead + 8, (uint32_t)nc);
  body(blob, kAttrTHead, attr_contexts(bpv, c), nc);
  return blob;
}

// a well-formed blob of one of the eight other kinds
static std::vector<uint8_t> make_old(bool scal, bool nl, int m, int bpv, int c, int64_t n, uint32_t e) {
  const int x = nl ? 4 : 0;
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int64_t p0_at = (scal ? kAttr2Head : kAttrHead + 8) + x;
  std::vector<uint8_t> blob((size_t)p0_at);
  blob[0] = 'A'; blob[1] = (uint8_t)attr_version(scal, nl, m != 0); blob[2] = (uint8_t)bpv; blob[3] = (uint8_t)(c | (m << 4));
  put32(blob, 4, (uint32_t)n);
  if (nl) put32(blob, kAttrHead, e);
  if (scal) {
    int64_t cells = n;
    for (int k = 0; k < 16; ++k) { put32(blob, (size_t)(kAttrHead + x + 4 * k), (uint32_t)cells); cells = std::max<int64_t>(1, cells / 3); }
  }
  put32(blob, (size_t)(p0_at - 8), (uint32_t)S);
  put32(blob, (size_t)(p0_at - 4), (uint32_t)nc);
  body(blob, p0_at, attr_contexts(bpv, c), nc);
  return blob;
}

static int parse_old(const std::vector<uint8_t>& b, bool scal, bool nl, bool cross) {
  AttrInfo a;
  if (!scal) return attr_parse_kind(b.data(), (int64_t)b.size(), nl, &a, cross);
  Attr2Info o;
  Attr2Plan pl;
  return attr2_parse_kind(b.data(), (int64_t)b.size(), 0, true, nl, &o, &pl, cross);
}

// what an accepted parse must hold, given the bytes it saw
static int check(const AttrTInfo& q, int64_t len, bool prefix) {
  if (q.version != 19 || (q.bpv != 1 && q.bpv != 2) || q.c < 1 || q.c > 4 || q.slod < 0 || q.slod > 15) return 2;
  if (q.nctx != attr_contexts(q.bpv, q.c) || q.max_error != 0 || q.cross != 0) return 3;
  if (q.n == 0) return q.qstep == 0 && len == kAttrHead ? 0 : 4;
  if (q.qstep < 1 || q.qstep >= (1u << (8 * q.bpv - 1)) || len < kAttrHead + 4) return 5;
  if (q.off_p0 != kAttrTHead || q.off_table != q.off_p0 + 2 * q.nctx) return 6;
  if (len >= kAttrTHead && (q.S * q.c > kAttrMaxValues || q.S < 1 || q.nc < 1 || kAttrLanes * q.S * q.nc < q.n || kAttrLanes * q.S * (q.nc - 1) >= q.n))
    return 7;
  if (!prefix && (q.off_payload != q.off_table + 4 * q.nc || q.off_payload + 2 * q.payload_words != len)) return 8;
  return 0;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  // attr_kind still knows its eight bytes and nothing else; attr_t_kind knows 19 alone
  for (int v = 0; v < 256; ++v) {
    bool s, n, x;
    const bool valid = v == 1 || v == 2 || v == 4 || v == 7 || v == 8 || v == 11 || v == 13 || v == 14;
    if (attr_kind(v, &s, &n, &x) != valid) return 20;
    if (attr_t_kind(v) != (v == 19)) return 21;
  }
  // well-formed heads are accepted, whole and from every prefix of 16 bytes and more, and read back what was written
  const std::vector<uint8_t> good[4] = {make_t(1, 0, 3, 30000, 32), make_t(2, 2, 2, 40000, 32767), make_t(1, 15, 4, 1, 127),
                                        make_t(2, 0, 1, 70000, 1)};
  const uint32_t good_q[4] = {32, 32767, 127, 1};
  const int64_t good_n[4] = {30000, 40000, 1, 70000};
  for (int k = 0; k < 4; ++k) {
    AttrTInfo a;
    if (attr_t_parse(good[k].data(), (int64_t)good[k].size(), &a) != 0 || check(a, (int64_t)good[k].size(), false)) return 22;
    if (a.qstep != good_q[k] || a.n != good_n[k]) return 23;
    for (int64_t cut = 16; cut <= (int64_t)good[k].size(); cut += 1 + (cut > 4096 ? 997 : 0)) {
      std::vector<uint8_t> b(good[k].begin(), good[k].begin() + cut);
      if (attr_t_parse(b.data(), cut, &a, true) != 0 || a.qstep != good_q[k] || a.n != good_n[k] || check(a, cut, true)) return 24;
      if (cut < (int64_t)good[k].size() && attr_t_parse(b.data(), cut, &a) == 0) return 25;   // a cut blob is no whole blob
    }
    for (int64_t cut = 0; cut < 16; ++cut) {
      std::vector<uint8_t> b(good[k].begin(), good[k].begin() + cut);
      if (attr_t_parse(cut ? b.data() : nullptr, cut, &a, true) == 0) return 26;
    }
    // q = 0 and q = H
    std::vector<uint8_t> b = good[k];
    put32(b, kAttrHead, 0);
    if (attr_t_parse(b.data(), (int64_t)b.size(), &a) == 0 || attr_t_parse(b.data(), 16, &a, true) == 0) return 27;
    put32(b, kAttrHead, 1u << (8 * (good[k][2] & 15) - 1));
    if (attr_t_parse(b.data(), (int64_t)b.size(), &a) == 0 || attr_t_parse(b.data(), 16, &a, true) == 0) return 28;
    // the eight old parsers refuse byte 19, also over this blob's bytes
    for (int p = 0; p < 8; ++p)
      if (parse_old(good[k], p & 1, p & 2, p & 4) == 0) return 29;
  }
  // the empty frame: 12 bytes, no q
  {
    std::vector<uint8_t> b = {'A', 19, 1 | (3 << 4), 3, 0, 0, 0, 0, 0, 0, 0, 0};
    AttrTInfo a;
    if (attr_t_parse(b.data(), 12, &a) != 0 || check(a, 12, false) || a.slod != 3 || a.c != 3) return 30;
    b[3] = 5;
    if (attr_t_parse(b.data(), 12, &a) == 0) return 31;
    b[3] = 0;
    if (attr_t_parse(b.data(), 12, &a) == 0) return 32;
  }
  // the eight old bytes are refused by the new parser: over their own blobs, and patched into a version-19 blob; byte 19
  // patched into their blobs is refused by their parsers and by this one (their layouts are not this one's)
  for (int k = 0; k < 8; ++k) {
    const bool scal = k & 1, nl = k & 2, cross = k & 4;
    std::vector<uint8_t> old = scal ? make_old(true, nl, cross ? 5 : 0, 1, 4, 30000, 4) : make_old(false, nl, cross ? 2 : 0, 2, 3, 40000, 1000);
    AttrTInfo a;
    if (parse_old(old, scal, nl, cross) != 0) return 33;
    if (attr_t_parse(old.data(), (int64_t)old.size(), &a) == 0 || attr_t_parse(old.data(), (int64_t)old.size(), &a, true) == 0) return 34;
    std::vector<uint8_t> b = good[0];
    b[1] = old[1];
    if (attr_t_parse(b.data(), (int64_t)b.size(), &a) == 0) return 35;
    old[1] = 19;
    for (int p = 0; p < 8; ++p)
      if (parse_old(old, p & 1, p & 2, p & 4) == 0) return 36;
    if (k != 2 && attr_t_parse(old.data(), (int64_t)old.size(), &a) == 0) return 37;   // version 4's layout IS this one's
  }
  printf("well-formed: version 19 %lld, %lld, %lld, %lld bytes\n", (long long)good[0].size(), (long long)good[1].size(),
         (long long)good[2].size(), (long long)good[3].size());
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const std::vector<uint8_t>& src = good[rnd() & 3];
    const bool prefix = (rnd() & 1) != 0;
    const int64_t head = kAttrTHead + 2 * attr_contexts(src[2] & 15, src[3]);
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % src.size()) : (int64_t)src.size();
    std::vector<uint8_t> b(src.begin(), src.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const uint32_t where = rnd() & 7;
      const int64_t span = where == 0 ? (int64_t)b.size() : (where < 3 ? std::min<int64_t>(4, (int64_t)b.size()) : std::min<int64_t>(head + 384, (int64_t)b.size()));
      b[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
    }
    AttrTInfo q;
    if (attr_t_parse(b.empty() ? nullptr : b.data(), (int64_t)b.size(), &q, prefix) != 0) { ++errs; continue; }
    ++oks;
    const int bad = check(q, (int64_t)b.size(), prefix);
    if (bad) return bad;
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 16;
}
