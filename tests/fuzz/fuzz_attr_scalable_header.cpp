// The parser of the transform-coded attribute blob with level-of-detail prefixes, version 22 (csrc/attr_blob.h
// attr_s_parse in its three modes, attr_s_kind, attr_lod_plan), on damaged and cut blobs, whole and as prefixes: error
// codes, never a read outside the bytes given; an accepted K lies in 1 .. 15 - slod, the accepted counts are version
// 2's, every accepted plan lies inside the blob and, in the decoder's mode, inside the bytes given; a level above K is
// PCC_E_ARG.  Byte 22 is refused by the ten other parsers and their bytes by this one.  Built with
// -fsanitize=address,undefined by tests/test_fuzz_attr_scalable.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"

static uint64_t seed = 2222;
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

static void counts(std::vector<uint8_t>& blob, size_t at, int64_t n) {
  int64_t cells = n;
  for (int k = 0; k < 16; ++k) { put32(blob, at + 4 * k, (uint32_t)cells); cells = std::max<int64_t>(1, cells / 3); }
}

// a well-formed version-22 blob
static std::vector<uint8_t> make_s(int bpv, int slod, int c, int64_t n, uint32_t colour, const uint32_t* q, uint32_t K) {
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int head = attr_s_head(c);
  std::vector<uint8_t> blob((size_t)head);
  blob[0] = 'A'; blob[1] = 22; blob[2] = (uint8_t)(bpv | (slod << 4)); blob[3] = (uint8_t)c;
  put32(blob, 4, (uint32_t)n);
  put32(blob, kAttrHead, colour);
  for (int ch = 0; ch < c; ++ch) put32(blob, (size_t)(kAttrHead + 4 + 4 * ch), q[ch]);
  put32(blob, (size_t)(kAttrHead + 4 + 4 * c), K);
  counts(blob, (size_t)(kAttrHead + 8 + 4 * c), n);
  put32(blob, (size_t)(head - 8), (uint32_t)S);
  put32(blob, (size_t)(head - 4), (uint32_t)nc);
  body(blob, head, attr_contexts(bpv, c), nc);
  return blob;
}

// a well-formed blob of one of the ten other kinds: k < 8 the kinds of attr_kind, 8 version 19, 9 version 21
static std::vector<uint8_t> make_other(int k) {
  const bool scal = k & 1, nl = k & 2;
  const int m = k < 8 && (k & 4) ? 2 : 0, bpv = 1, c = 3;
  const int64_t n = 30000;
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  const int64_t p0_at = k == 8 ? kAttrTHead : (k == 9 ? attr_c_head(c) : (scal ? kAttr2Head : kAttrHead + 8) + (nl ? 4 : 0));
  std::vector<uint8_t> blob((size_t)p0_at);
  blob[0] = 'A'; blob[1] = (uint8_t)(k == 8 ? 19 : (k == 9 ? 21 : attr_version(scal, nl, m != 0))); blob[2] = (uint8_t)bpv;
  blob[3] = (uint8_t)(c | (m << 4));
  put32(blob, 4, (uint32_t)n);
  if (k == 9) { put32(blob, kAttrHead, 1); for (int ch = 0; ch < c; ++ch) put32(blob, (size_t)(kAttrHead + 4 + 4 * ch), 7); }
  else if (k == 8 || nl) put32(blob, kAttrHead, 5);
  if (k < 8 && scal) counts(blob, (size_t)(kAttrHead + (nl ? 4 : 0)), n);
  put32(blob, (size_t)(p0_at - 8), (uint32_t)S);
  put32(blob, (size_t)(p0_at - 4), (uint32_t)nc);
  body(blob, p0_at, attr_contexts(bpv, c), nc);
  return blob;
}

static int parse_other(const std::vector<uint8_t>& b, int p) {
  if (p >= 8) {
    AttrCInfo t;
    return attr_tc_parse(b.data(), (int64_t)b.size(), &t, p == 9 ? &t : nullptr, false) == 0 ||
                   attr_tc_parse(b.data(), (int64_t)b.size(), &t, p == 9 ? &t : nullptr, true) == 0 ? 0 : 1;
  }
  const bool scal = p & 1, nl = p & 2, cross = p & 4;
  AttrInfo a;
  if (!scal) return attr_parse_kind(b.data(), (int64_t)b.size(), nl, &a, cross);
  Attr2Info o;
  Attr2Plan pl;
  return attr2_parse_kind(b.data(), (int64_t)b.size(), 0, true, nl, &o, &pl, cross);
}

// what an accepted parse must hold, given the bytes it saw
static int check(const AttrSInfo& q, const Attr2Plan& pl, int64_t len, int lod, AttrSMode mode) {
  if (q.version != 22 || (q.bpv != 1 && q.bpv != 2) || q.c < 1 || q.c > 4 || q.slod < 0 || q.slod > 15) return 2;
  if (q.nctx != attr_contexts(q.bpv, q.c) || q.max_error != 0 || q.cross != 0 || q.qstep != 0) return 3;
  if (q.n == 0) return q.colour == 0 && q.K == 0 && q.q[0] == 0 && q.q[3] == 0 && len == kAttrHead ? 0 : 4;
  const int head = attr_s_head(q.c);
  if (len < kAttrHead + 8 + 4 * q.c) return 5;
  if (q.K < 1 || q.K + q.slod > 15) return 6;
  if (q.colour > 1 || (q.colour == 1 && q.c < 3)) return 9;
  for (int ch = 0; ch < 4; ++ch)
    if (ch < q.c ? (q.q[ch] < 1 || q.q[ch] >= (1u << (8 * q.bpv - 1))) : q.q[ch] != 0) return 10;
  if (q.off_p0 != head || q.off_table != q.off_p0 + 2 * q.nctx) return 7;
  if (mode == kAttrSHead) return 0;
  if (lod < 0 || lod > q.K) return 11;
  if (q.cells[0] != q.n) return 12;
  for (int k = 1; k < 16; ++k)
    if (q.cells[k] < 1 || q.cells[k] > q.cells[k - 1] || 8 * q.cells[k] < q.cells[k - 1]) return 12;
  if (q.S * q.c > kAttrMaxValues || q.S < 1 || q.nc < 1 || kAttrLanes * q.S * q.nc < q.n || kAttrLanes * q.S * (q.nc - 1) >= q.n) return 13;
  const int64_t total = q.off_payload + 2 * q.payload_words;
  if (q.off_payload != q.off_table + 4 * q.nc || len > total) return 8;
  if (pl.m != q.cells[lod] || pl.bytes > total || pl.bytes < q.off_payload || pl.chunks < 1 || pl.chunks > q.nc) return 14;
  if (mode == kAttrSDecode && pl.bytes > len) return 15;
  if (lod == 0 && pl.bytes != total) return 17;
  return 0;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  for (int v = 0; v < 256; ++v) {
    bool s, n, x;
    const bool valid = v == 1 || v == 2 || v == 4 || v == 7 || v == 8 || v == 11 || v == 13 || v == 14;
    if (attr_kind(v, &s, &n, &x) != valid) return 20;
    if (attr_t_kind(v) != (v == 19) || attr_c_kind(v) != (v == 21) || attr_s_kind(v) != (v == 22)) return 21;
  }
  const uint32_t qs[4][4] = {{32, 64, 64, 0}, {32767, 1, 0, 0}, {127, 1, 2, 3}, {1, 0, 0, 0}};
  const uint32_t cols[4] = {1, 0, 1, 0}, Ks[4] = {3, 13, 1, 15};
  const int slods[4] = {0, 2, 14, 0};
  const int64_t good_n[4] = {30000, 40000, 1, 70000};
  const std::vector<uint8_t> good[4] = {make_s(1, 0, 3, 30000, 1, qs[0], 3), make_s(2, 2, 2, 40000, 0, qs[1], 13), make_s(1, 14, 4, 1, 1, qs[2], 1),
                                        make_s(2, 0, 1, 70000, 0, qs[3], 15)};
  for (int k = 0; k < 4; ++k) {
    AttrSInfo a;
    Attr2Plan pl;
    const int c = good[k][3], reach = kAttrHead + 8 + 4 * c, at_k = reach - 4;
    const int64_t size = (int64_t)good[k].size();
    auto same = [&](const AttrSInfo& i) {
      for (int ch = 0; ch < 4; ++ch)
        if (i.q[ch] != (ch < c ? qs[k][ch] : 0u)) return false;
      return i.colour == cols[k] && i.n == good_n[k] && i.K == (int)Ks[k] && i.slod == slods[k];
    };
    // every level 0 .. K: the decoder's form over the plan's bytes and not one byte less; the plan from a prefix
    for (int lod = 0; lod <= (int)Ks[k]; ++lod) {
      if (attr_s_parse(good[k].data(), size, lod, kAttrSPlan, &a, &pl) != 0 || !same(a) || check(a, pl, size, lod, kAttrSPlan)) return 22;
      const int64_t need = pl.bytes;
      Attr2Plan p2;
      if (attr_s_parse(good[k].data(), need, lod, kAttrSDecode, &a, &p2) != 0 || p2.bytes != need || check(a, p2, need, lod, kAttrSDecode)) return 23;
      if (attr_s_parse(good[k].data(), need - 1, lod, kAttrSDecode, &a, &p2) == 0) return 24;
    }
    if (attr_s_parse(good[k].data(), size, (int)Ks[k] + 1, kAttrSPlan, &a, &pl) != PCC_E_ARG) return 26;
    if (attr_s_parse(good[k].data(), size, (int)Ks[k] + 1, kAttrSDecode, &a, &pl) != PCC_E_ARG) return 26;
    if (attr_s_parse(good[k].data(), size, -1, kAttrSPlan, &a, &pl) != PCC_E_ARG) return 26;
    // the head from every prefix that reaches K, and from none that does not
    for (int64_t cut = reach; cut <= size; cut += 1 + (cut > 4096 ? 997 : 0)) {
      std::vector<uint8_t> b(good[k].begin(), good[k].begin() + cut);
      if (attr_s_parse(b.data(), cut, 0, kAttrSHead, &a, nullptr) != 0 || !same(a) || check(a, pl, cut, 0, kAttrSHead)) return 27;
      if (cut < size && attr_s_parse(b.data(), cut, 0, kAttrSDecode, &a, &pl) == 0) return 28;   // a cut blob is no whole blob
    }
    for (int64_t cut = 0; cut < reach; ++cut) {
      std::vector<uint8_t> b(good[k].begin(), good[k].begin() + cut);
      if (attr_s_parse(cut ? b.data() : nullptr, cut, 0, kAttrSHead, &a, nullptr) == 0) return 29;
    }
    // K: 0, beyond 15 - slod, and huge
    for (uint32_t bad : {0u, (uint32_t)(16 - slods[k]), 16u, 0x80000001u}) {
      std::vector<uint8_t> b = good[k];
      put32(b, (size_t)at_k, bad);
      if (attr_s_parse(b.data(), size, 0, kAttrSDecode, &a, &pl) == 0 || attr_s_parse(b.data(), reach, 0, kAttrSHead, &a, nullptr) == 0) return 30;
    }
    // the counts: count[0] != n, a level that grows, a level below an eighth, a zero
    for (int what = 0; what < 4; ++what) {
      std::vector<uint8_t> b = good[k];
      const size_t at = (size_t)reach;
      if (what == 0) put32(b, at, (uint32_t)good_n[k] + 1);
      if (what == 1) put32(b, at + 8, attr_u32(b.data() + at + 4) + 1);
      if (what == 2) put32(b, at + 4, (uint32_t)(good_n[k] / 9));
      if (what == 3) put32(b, at + 60, 0);
      if (what == 2 && good_n[k] < 9) continue;
      if (attr_s_parse(b.data(), size, 0, kAttrSDecode, &a, &pl) == 0 || attr_s_parse(b.data(), size, 0, kAttrSPlan, &a, &pl) == 0) return 31;
    }
    // steps and the colour word, as version 21
    for (int ch = 0; ch < c; ++ch)
      for (uint32_t bad : {0u, 1u << (8 * (good[k][2] & 15) - 1)}) {
        std::vector<uint8_t> b = good[k];
        put32(b, (size_t)(kAttrHead + 4 + 4 * ch), bad);
        if (attr_s_parse(b.data(), size, 0, kAttrSDecode, &a, &pl) == 0 || attr_s_parse(b.data(), reach, 0, kAttrSHead, &a, nullptr) == 0) return 32;
      }
    {
      std::vector<uint8_t> b = good[k];
      put32(b, kAttrHead, 2);
      if (attr_s_parse(b.data(), size, 0, kAttrSDecode, &a, &pl) == 0) return 33;
      put32(b, kAttrHead, 1);
      if ((attr_s_parse(b.data(), size, 0, kAttrSDecode, &a, &pl) == 0) != (c >= 3)) return 34;
    }
    // the ten other parsers refuse byte 22, also over this blob's bytes
    for (int p = 0; p < 10; ++p)
      if (parse_other(good[k], p) == 0) return 35;
  }
  // the empty frame: 12 bytes, at every level
  {
    std::vector<uint8_t> b = {'A', 22, 1 | (3 << 4), 3, 0, 0, 0, 0, 0, 0, 0, 0};
    AttrSInfo a;
    Attr2Plan pl;
    for (int lod = 0; lod <= 15; ++lod)
      if (attr_s_parse(b.data(), 12, lod, kAttrSDecode, &a, &pl) != 0 || check(a, pl, 12, lod, kAttrSDecode) || pl.bytes != 12 || pl.m != 0) return 36;
    b[3] = 5;
    if (attr_s_parse(b.data(), 12, 0, kAttrSDecode, &a, &pl) == 0) return 37;
    b[3] = 3; b[8] = 4;
    if (attr_s_parse(b.data(), 12, 0, kAttrSHead, &a, nullptr) == 0) return 37;
  }
  // the ten other bytes are refused by the new parser, over their own blobs and patched into a version-22 blob; byte 22
  // patched into their blobs is refused by their parsers and by this one
  for (int k = 0; k < 10; ++k) {
    std::vector<uint8_t> old = make_other(k);
    AttrSInfo a;
    Attr2Plan pl;
    if (parse_other(old, k) != 0) return 38;
    for (AttrSMode mode : {kAttrSDecode, kAttrSPlan, kAttrSHead})
      if (attr_s_parse(old.data(), (int64_t)old.size(), 0, mode, &a, &pl) == 0) return 39;
    std::vector<uint8_t> b = good[0];
    b[1] = old[1];
    if (attr_s_parse(b.data(), (int64_t)b.size(), 0, kAttrSDecode, &a, &pl) == 0) return 40;
    for (int p = 0; p < 10; ++p)
      if (parse_other(b, p) == 0) return 41;
    old[1] = 22;
    for (int p = 0; p < 10; ++p)
      if (parse_other(old, p) == 0) return 42;
    if (attr_s_parse(old.data(), (int64_t)old.size(), 0, kAttrSDecode, &a, &pl) == 0) return 43;
  }
  printf("well-formed: version 22 %lld, %lld, %lld, %lld bytes\n", (long long)good[0].size(), (long long)good[1].size(),
         (long long)good[2].size(), (long long)good[3].size());
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const std::vector<uint8_t>& src = good[rnd() & 3];
    const AttrSMode mode = (AttrSMode)(rnd() % 3);
    const int lod = (int)(rnd() % 18) - 1;
    const int64_t head = attr_s_head(src[3]) + 2 * attr_contexts(src[2] & 15, src[3]);
    const int64_t cut = (it % 3 == 0) ? (int64_t)(rnd() % src.size()) : (int64_t)src.size();
    std::vector<uint8_t> b(src.begin(), src.begin() + cut);   // exactly the bytes the parser may read
    const int flips = (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) {
      const uint32_t where = rnd() & 7;
      const int64_t span = where == 0 ? (int64_t)b.size() : (where < 3 ? std::min<int64_t>(4, (int64_t)b.size()) : std::min<int64_t>(head + 384, (int64_t)b.size()));
      b[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
    }
    AttrSInfo q;
    Attr2Plan pl;
    if (attr_s_parse(b.empty() ? nullptr : b.data(), (int64_t)b.size(), lod, mode, &q, &pl) != 0) { ++errs; continue; }
    ++oks;
    const int bad = check(q, pl, (int64_t)b.size(), lod, mode);
    if (bad) return bad;
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 && oks > 0 ? 0 : 16;
}
