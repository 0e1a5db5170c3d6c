// The parser of the transform-coded attribute blob with a colour word and one step per channel, version 21
// (csrc/attr_blob.h attr_c_parse, attr_c_kind), on damaged and cut blobs, whole and as prefixes: error codes, never a
// read outside the bytes given, an accepted colour word is 0 or 1 (1 with three channels and more), every accepted step
// lies in 1 .. H - 1 and every accepted size follows from the bytes present.  Byte 21 is refused by the nine other
// parsers and the nine other bytes by this one; attr_kind still knows exactly its eight, attr_t_kind 19 alone.  Built with
// -fsanitize=address,undefined by tests/test_fuzz_attr_colour.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"

static uint64_t seed = 2121;
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

// a well-formed version-21 blob
static std::vector<uint8_t> make_c(int bpv, int slod, int c, int64_t n, uint32_t colour, const uint32_t* q) {
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int head = attr_c_head(c);
  std::vector<uint8_t> blob((size_t)head);
  blob[0] = 'A'; blob[1] = 21; blob[2] = (uint8_t)(bpv | (slod << 4)); blob[3] = (uint8_t)c;
  put32(blob, 4, (uint32_t)n);
  put32(blob, kAttrHead, colour);
  for (int ch = 0; ch < c; ++ch) put32(blob, (size_t)(kAttrHead + 4 + 4 * ch), q[ch]);
  put32(blob, (size_t)(head - 8), (uint32_t)S);
  put32(blob, (size_t)(head - 4), (uint32_t)nc);
  body(blob, head, attr_contexts(bpv, c), nc);
  return blob;
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

// a well-formed blob of one of the eight kinds of attr_kind
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

// the nine other parsers: p < 8 the kinds of attr_kind, p = 8 version 19's
static int parse_other(const std::vector<uint8_t>& b, int p) {
  if (p == 8) {
    AttrTInfo t;
    return attr_t_parse(b.data(), (int64_t)b.size(), &t) == 0 || attr_t_parse(b.data(), (int64_t)b.size(), &t, true) == 0 ? 0 : 1;
  }
  const bool scal = p & 1, nl = p & 2, cross = p & 4;
  AttrInfo a;
  if (!scal) return attr_parse_kind(b.data(), (int64_t)b.size(), nl, &a, cross);
  Attr2Info o;
  Attr2Plan pl;
  return attr2_parse_kind(b.data(), (int64_t)b.size(), 0, true, nl, &o, &pl, cross);
}

// what an accepted parse must hold, given the bytes it saw
static int check(const AttrCInfo& q, int64_t len, bool prefix) {
  if (q.version != 21 || (q.bpv != 1 && q.bpv != 2) || q.c < 1 || q.c > 4 || q.slod < 0 || q.slod > 15) return 2;
  if (q.nctx != attr_contexts(q.bpv, q.c) || q.max_error != 0 || q.cross != 0 || q.qstep != 0) return 3;
  if (q.n == 0) return q.colour == 0 && q.q[0] == 0 && q.q[1] == 0 && q.q[2] == 0 && q.q[3] == 0 && len == kAttrHead ? 0 : 4;
  const int head = attr_c_head(q.c);
  if (len < head - 8) return 5;
  if (q.colour > 1 || (q.colour == 1 && q.c < 3)) return 9;
  for (int ch = 0; ch < 4; ++ch)
    if (ch < q.c ? (q.q[ch] < 1 || q.q[ch] >= (1u << (8 * q.bpv - 1))) : q.q[ch] != 0) return 10;
  if (q.off_p0 != head || q.off_table != q.off_p0 + 2 * q.nctx) return 6;
  if (len >= head && (q.S * q.c > kAttrMaxValues || q.S < 1 || q.nc < 1 || kAttrLanes * q.S * q.nc < q.n || kAttrLanes * q.S * (q.nc - 1) >= q.n))
    return 7;
  if (!prefix && (q.off_payload != q.off_table + 4 * q.nc || q.off_payload + 2 * q.payload_words != len)) return 8;
  return 0;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  // attr_kind still knows its eight bytes and nothing else, attr_t_kind 19 alone, attr_c_kind 21 alone
  for (int v = 0; v < 256; ++v) {
    bool s, n, x;
    const bool valid = v == 1 || v == 2 || v == 4 || v == 7 || v == 8 || v == 11 || v == 13 || v == 14;
    if (attr_kind(v, &s, &n, &x) != valid) return 20;
    if (attr_t_kind(v) != (v == 19) || attr_c_kind(v) != (v == 21)) return 21;
  }
  // well-formed heads are accepted, whole and from every prefix that reaches q[c - 1], and read back what was written
  const uint32_t qs[4][4] = {{32, 64, 64, 0}, {32767, 1, 0, 0}, {127, 1, 2, 3}, {1, 0, 0, 0}};
  const uint32_t cols[4] = {1, 0, 1, 0};
  const int64_t good_n[4] = {30000, 40000, 1, 70000};
  const std::vector<uint8_t> good[4] = {make_c(1, 0, 3, 30000, 1, qs[0]), make_c(2, 2, 2, 40000, 0, qs[1]), make_c(1, 15, 4, 1, 1, qs[2]),
                                        make_c(2, 0, 1, 70000, 0, qs[3])};
  for (int k = 0; k < 4; ++k) {
    AttrCInfo a;
    const int c = good[k][3], bpv = good[k][2] & 15, reach = 16 + 4 * c;
    auto same = [&](const AttrCInfo& i) {
      for (int ch = 0; ch < 4; ++ch)
        if (i.q[ch] != (ch < c ? qs[k][ch] : 0u)) return false;
      return i.colour == cols[k] && i.n == good_n[k];
    };
    if (attr_c_parse(good[k].data(), (int64_t)good[k].size(), &a) != 0 || check(a, (int64_t)good[k].size(), false)) return 22;
    if (!same(a)) return 23;
    for (int64_t cut = reach; cut <= (int64_t)good[k].size(); cut += 1 + (cut > 4096 ? 997 : 0)) {
      std::vector<uint8_t> b(good[k].begin(), good[k].begin() + cut);
      if (attr_c_parse(b.data(), cut, &a, true) != 0 || !same(a) || check(a, cut, true)) return 24;
      if (cut < (int64_t)good[k].size() && attr_c_parse(b.data(), cut, &a) == 0) return 25;   // a cut blob is no whole blob
    }
    for (int64_t cut = 0; cut < reach; ++cut) {
      std::vector<uint8_t> b(good[k].begin(), good[k].begin() + cut);
      if (attr_c_parse(cut ? b.data() : nullptr, cut, &a, true) == 0) return 26;
    }
    // every step: 0 and H
    for (int ch = 0; ch < c; ++ch) {
      std::vector<uint8_t> b = good[k];
      put32(b, (size_t)(kAttrHead + 4 + 4 * ch), 0);
      if (attr_c_parse(b.data(), (int64_t)b.size(), &a) == 0 || attr_c_parse(b.data(), reach, &a, true) == 0) return 27;
      put32(b, (size_t)(kAttrHead + 4 + 4 * ch), 1u << (8 * bpv - 1));
      if (attr_c_parse(b.data(), (int64_t)b.size(), &a) == 0 || attr_c_parse(b.data(), reach, &a, true) == 0) return 28;
    }
    // the colour word: above 1; 1 with fewer than three channels, 1 and 0 with three and more
    {
      std::vector<uint8_t> b = good[k];
      for (uint32_t bad : {2u, 3u, 256u, 0x80000001u}) {
        put32(b, kAttrHead, bad);
        if (attr_c_parse(b.data(), (int64_t)b.size(), &a) == 0 || attr_c_parse(b.data(), reach, &a, true) == 0) return 38;
      }
      put32(b, kAttrHead, 1);
      if ((attr_c_parse(b.data(), (int64_t)b.size(), &a) == 0) != (c >= 3)) return 39;
      if ((attr_c_parse(b.data(), reach, &a, true) == 0) != (c >= 3)) return 40;
      put32(b, kAttrHead, 0);
      if (attr_c_parse(b.data(), (int64_t)b.size(), &a) != 0 || a.colour != 0) return 41;
    }
    // the nine other parsers refuse byte 21, also over this blob's bytes
    for (int p = 0; p < 9; ++p)
      if (parse_other(good[k], p) == 0) return 29;
  }
  // the empty frame: 12 bytes, neither colour nor steps
  {
    std::vector<uint8_t> b = {'A', 21, 1 | (3 << 4), 3, 0, 0, 0, 0, 0, 0, 0, 0};
    AttrCInfo a;
    if (attr_c_parse(b.data(), 12, &a) != 0 || check(a, 12, false) || a.slod != 3 || a.c != 3) return 30;
    b[3] = 5;
    if (attr_c_parse(b.data(), 12, &a) == 0) return 31;
    b[3] = 0;
    if (attr_c_parse(b.data(), 12, &a) == 0) return 32;
  }
  // the nine other bytes are refused by the new parser: over their own blobs, and patched into a version-21 blob; byte 21
  // patched into their blobs is refused by their parsers and by this one (their layouts are not this one's)
  for (int k = 0; k < 9; ++k) {
    const bool scal = k & 1, nl = k & 2, cross = k & 4;
    std::vector<uint8_t> old = k == 8 ? make_t(1, 0, 3, 30000, 32)
                                      : (scal ? make_old(true, nl, cross ? 5 : 0, 1, 4, 30000, 4) : make_old(false, nl, cross ? 2 : 0, 2, 3, 40000, 1000));
    AttrCInfo a;
    if (parse_other(old, k) != 0) return 33;
    if (attr_c_parse(old.data(), (int64_t)old.size(), &a) == 0 || attr_c_parse(old.data(), (int64_t)old.size(), &a, true) == 0) return 34;
    std::vector<uint8_t> b = good[0];
    b[1] = old[1];
    if (attr_c_parse(b.data(), (int64_t)b.size(), &a) == 0) return 35;
    for (int p = 0; p < 9; ++p)
      if (parse_other(b, p) == 0) return 42;
    old[1] = 21;
    for (int p = 0; p < 9; ++p)
      if (parse_other(old, p) == 0) return 36;
    if (attr_c_parse(old.data(), (int64_t)old.size(), &a) == 0) return 37;
  }
  printf("well-formed: version 21 %lld, %lld, %lld, %lld bytes\n", (long long)good[0].size(), (long long)good[1].size(),
         (long long)good[2].size(), (long long)good[3].size());
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const std::vector<uint8_t>& src = good[rnd() & 3];
    const bool prefix = (rnd() & 1) != 0;
    const int64_t head = attr_c_head(src[3]) + 2 * attr_contexts(src[2] & 15, src[3]);
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % src.size()) : (int64_t)src.size();
    std::vector<uint8_t> b(src.begin(), src.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const uint32_t where = rnd() & 7;
      const int64_t span = where == 0 ? (int64_t)b.size() : (where < 3 ? std::min<int64_t>(4, (int64_t)b.size()) : std::min<int64_t>(head + 384, (int64_t)b.size()));
      b[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
    }
    AttrCInfo q;
    if (attr_c_parse(b.empty() ? nullptr : b.data(), (int64_t)b.size(), &q, prefix) != 0) { ++errs; continue; }
    ++oks;
    const int bad = check(q, (int64_t)b.size(), prefix);
    if (bad) return bad;
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 16;
}
