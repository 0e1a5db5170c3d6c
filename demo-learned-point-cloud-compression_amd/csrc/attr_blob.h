// attr_blob.h — the header of an attribute blob (attr.hip), parsed and checked on the host before anything is reserved
// or launched.  Plain C++ (no HIP): tests/fuzz/fuzz_attr_header.cpp, fuzz_attr2_header.cpp, fuzz_attr_nl_header.cpp,
// fuzz_attr_cross_header.cpp, fuzz_attr_transform_header.cpp, fuzz_attr_colour_header.cpp,
// fuzz_attr_scalable_header.cpp, fuzz_attr_nbr_header.cpp and fuzz_attr_nbr_nl_header.cpp put it under the sanitizers.
//
// Every size the decoder reserves or reads follows from what this parse accepted: the chunk table must add up to the
// blob's own length, so a header cannot announce more words than the blob holds; n is bounded by the chunks
// (64 S nc >= n > 64 S (nc - 1)) and the chunks by the table.
//
// Attribute blob, version 2 (attr2_parse): the values of every coarser level of detail are a prefix of its bytes.
//
//   'A' 2 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 cells[16] | u32 S | u32 n_chunks | u16 p0[nctx] |
//   u32 words[n_chunks] | chunk payloads                 (n == 0: the 12 bytes up to payload_len = 0, nothing more)
//   slod: 0, or the level of detail the SENDER coded its cells at (pcc_attr_encode_frames_v2's key_shift / 3): the keys
//   below are then those of the cells p >> slod, biased by 32768 >> slod
//   chunk = 64 x (state lo, state hi) | u16 len[64] | words of lane 0 | words of lane 1 | ..   (as version 1)
//
// The frame's n distinct points in Morton order, their merged values v_i and 48-bit Morton keys key_i:
//   size of introduction   s(0) = 16; s(i) = floor(hb(key_i xor key_{i-1}) / 3) in 0 .. 15 (hb: highest set bit): point
//                          i is the Morton-first point of its cell p >> k exactly when s(i) >= k
//   cells[k]               #{i : s(i) >= k}: the cells of level of detail k (cells[0] = n)
//   introduction order     (s descending, Morton index ascending): the values of level k are the first cells[k]
//   predictor              first(i) = lower_bound(keys, key_i with its low 3 (s(i) + 1) bits cleared), i > 0: the
//                          Morton-first point of the next larger cell around i, introduced at a strictly larger size
//   residual               per channel r = ((v_i - v_first(i) + h) & mask) - h (point 0: against 0), h = 2^(8 bpv - 1)
// The residuals in introduction order are dealt to lanes and chunks (S points per lane, attr_layout) and coded as
// version 1 codes its residuals — same binarisation, contexts (channel, bucket of the channel's previous residual in the
// lane's run, position) and model — without version 1's prediction inside the run.
// Level of detail k of a blob of n > 0 values: m = cells[k] values, row j the value of the Morton-first point of the
// j-th cell (Morton order).  The cell keys key >> 3k give s - k, the same first and the same order, so a decoder runs
// the rule above on the cells of its geometry, biased by 32768 >> (slod + k) (slod + k <= 15).  Shortest prefix: k = 0 the whole blob; else lanes = ceil(m / S),
// c* = (lanes - 1) / 64, l* = (lanes - 1) % 64: off_payload + 2 (words[0] + .. + words[c* - 1]) + 2 (192 + len[0] + ..
// + len[l*]), len being chunk c*'s own length table (the rule of octree2_blob.h).  Header, p0 and the whole chunk table
// are always needed.  tests/attr2_ref.py restates the format in numpy.
//
// Near-lossless kinds, versions 4 and 7 (attr_parse_kind / attr2_parse_kind): version 1's and version 2's layouts with
// a u32 max_error = e directly behind payload_len (counted in it; everything behind it 4 bytes later; n == 0: the 12
// bytes alone, which do not record e).  The valid version bytes 1, 2, 4, 7 differ pairwise in two bits.  What the lanes
// code is, instead of a wrapped residual, the INDEX j of the quantised prediction error of a closed loop (the predictor
// sees what the decoder will see; include/pcc.h states the rule in full):
//   q = 2 e + 1, 1 <= e < 2^(8 bpv - 1);  d = v - p (no wrap);  j = sgn(d) floor((|d| + e) / q);  v^ = p + j q kept as an
//   unclamped signed integer inside the loop, clamp(v^, 0, mask) written out;  |v - v^| <= e and |j| < 2^(8 bpv - 1)
//   version 4   p = 0, v^[s-1], (v^[s-1] + v^[s-2] + 1) >> 1 (arithmetic shift) for s = 0, 1, >= 2 of the lane's run
//   version 7   p = v^[first(i)] (point 0: 0), so v^_i = q x the sum of j along i -> first(i) -> .. -> 0; the value of a
//               cell at a level of detail is the reconstruction of its Morton-first point
// Binarisation, contexts (bucket of |j| of the channel's previous point in the run, edges 2 / 5 / 12 / 30, not retuned),
// model, S, chunks, word runs and the prefix rule are unchanged.  tests/attr_nl_ref.py restates both kinds in numpy.
//
// Cross-channel kinds, versions 8, 11, 13 and 14 (the cross forms of 1, 2, 4 and 7; the eight valid version bytes keep
// odd parity, so any two differ in two bits): the plain kind's layout, byte for byte, with byte 3 = c | m << 4, bit
// ch - 1 of m set for every channel ch of the mask M, a subset of {1 .. c - 1} (m != 0, m < 2^(c - 1); a plain kind
// keeps byte 3 = c).  An empty frame is the 12-byte head with the cross version byte and that channel byte.
// Let w[i][ch] be what the plain kind codes for point i, channel ch in its coding order — the wrapped residual r of
// versions 1 and 2, the index j of versions 4 and 7 — an integer in [-h, h), h = 2^(8 bpv - 1).  The cross kind codes
//   x[i][ch] = w[i][ch]                                         ch = 0 or ch not in M
//   x[i][ch] = ((w[i][ch] - w[i][ch - 1] + h) & mask) - h       ch in M: a chain, against the ORIGINAL w of channel
//                                                               ch - 1, not against x
// through the coder as version 2's residuals go (no prediction inside the run; context = the bucket of |x| of the
// channel's previous point in the lane's run, 0 for the run's first point).  The decoder undoes it per point, channel by
// channel in ascending order (w[ch] = ((x[ch] + w[ch - 1] + h) & mask) - h), then continues exactly as the plain kind
// does: a cross kind decodes to the values of the plain kind of the same call, at every level of detail, and the
// near-lossless bound holds unchanged.  Binarisation, model, p0, S, chunks, word runs and the prefix rule are unchanged.
// tests/attr_cross_ref.py restates the four kinds in numpy.
//
// Neighbour-predicted kinds, versions 25 and 26 (attr2_parse_kind with nbr = true; 26 is the cross form of 25 as 11 is
// of 2; 25 = 11001b and 26 = 11010b keep the odd parity of the eleven bytes 1, 2, 4, 7, 8, 11, 13, 14, 19, 21, 22 and so
// differ from each in two bits): lossless and scalable.  Layout, chunks, coder, contexts, model, introduction order,
// cells[], slod and the prefix rule are version 2's, byte for byte; only the predictor differs.
//   'A' 25 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 cells[16] | u32 S | u32 n_chunks | u16 p0[nctx] |
//   u32 words[n_chunks] | chunk payloads      (n == 0: the 12-byte head; version 26: byte 3 = c | m << 4 as version 11)
// Coordinates are biased by 32768 >> slod; the lattice is [0, 65536 >> slod) per axis.
//   candidates of i > 0   s = s(i), P its biased coordinates, u = P >> s, C = P >> (s + 1).  For each o in {-1, 0, 1}^3
//                         whose cell C + o of side 2^(s + 1) lies inside the lattice (every axis: 0 <= C + o and
//                         (C + o) << (s + 1) below the lattice's side), j(o) = the frame's Morton-first point inside that
//                         cell, if it holds one: one lower bound over the sorted keys.  o = 0 is version 2's first(i) and
//                         always exists.  Every candidate was introduced at a size >= s + 1; its Morton index may be
//                         above i
//   choice                d(o) = |(P_j >> s) - u|^2, an integer in 1 .. 27 (never 0: i and j are the first points of
//                         different cells of side 2^s).  The up to three candidates with the smallest (d, Morton index
//                         of j) are kept, each with the weight w = floor(65536 / d)
//   predictor             per channel p = floor((2 sum(w v_j) + sum(w)) / (2 sum(w))), in 64-bit integers (three weights
//                         of 65536 times a uint16 do not fit 32 bits)
//   residual              r = ((v_i - p + h) & mask) - h; point 0 is coded against 0
// The residuals go in introduction order through version 2's coder (no prediction inside the run; contexts = channel,
// bucket of the channel's previous residual in the lane's run, position).  Version 26: the cross rule above applied to
// these residuals.  Level of detail k: a point present at level k has s >= k, and u, C, the candidate cells and d are
// functions of P >> s and P >> (s + 1), which the cells P >> k give; the candidates' values are exact, the kind being
// lossless.  So a decoder runs the same rule on the cells of its geometry, biased by 32768 >> (slod + k), the sizes
// 16 down to 0 one after the other (a point's candidates are all of larger sizes); row j is the value of the
// Morton-first point of cell j, the shortest prefix is version 2's.  tests/attr_nbr_ref.py restates both kinds in numpy.
//
// Bounded-error neighbour kinds, versions 28 and 31 (attr2_parse_kind with nbr = true and nl = true; 31 is the cross form
// of 28 as 14 is of 7; 28 = 11100b and 31 = 11111b keep the odd parity of the thirteen bytes above): |v - v^| <= e,
// scalable.  The layout is version 7's (14's), byte for byte, under the version byte: max_error behind payload_len,
// cells[16], S, n_chunks, p0, chunk table, chunks, slod in byte 2, the mask in the high nibble of byte 3; the prefix rule
// is version 7's.  Candidates, d, the tie-break on (d, Morton index) and w = floor(65536 / d) are version 25's: functions
// of the geometry alone.  q = 2 e + 1, mask = 2^(8 bpv) - 1.
//   predictor             point 0: p = 0.  i > 0: per channel p = floor((2 sum(w v^_j) + sum(w)) / (2 sum(w))) over its
//                         candidates' DECODED values v^_j (clamped, what a decoder returns), in 64-bit integers
//   index                 j_i = sgn(d) floor((|d| + e) / q), d = v_i - p: no wrap (|d| <= mask, so |j_i| < 2^(8 bpv - 1))
//   decoded value         v^_i = clip(p + j_i q, 0, mask); v_i is in range, so |v_i - v^_i| <= e
// A closed loop: the encoder forms v^ size by size, 16 down to 0, since every candidate was introduced at a larger size.
// The j go in introduction order through version 7's coder; version 31 applies the cross rule to them.  Level of detail
// k: a point present at level k has s >= k and its candidates sizes >= s + 1, so a decoder at a cut forms the same p
// from its cells alone; row j is v^ of the Morton-first point of cell j, within e of the row versions 25 / 26 return at
// that lod.  A decoder forms p + j q in 64 bits (a damaged uint16 stream at e = 32767 reaches 2^31), clamps, and reports
// a sum outside [-e, mask + e], which no encoder's reconstruction is.  tests/attr_nbr_nl_ref.py restates both in numpy.
#pragma once
#include <stdint.h>

#include "../../include/pcc.h"

void pcc_set_error(const char* fmt, ...);

#if defined(__HIPCC__)
#define ATTR_HD __host__ __device__
#else
#define ATTR_HD
#endif

constexpr int kAttrHead = 12;          // 'A' 1 bpv c | u32 n | u32 payload_len
constexpr int kAttrBuckets = 5;        // previous residual's magnitude: edges 2, 5, 12, 30
constexpr int kAttrMaxValues = 512;    // values per lane run: S c <= 512
constexpr int kAttrLanes = 64;

// binarisation positions per (channel, bucket): zero flag, sign, kmax prefix bits, kmax suffix bits (kmax = 8 bpv - 1)
ATTR_HD static inline int attr_positions(int bpv) { return 16 * bpv; }
ATTR_HD static inline int attr_contexts(int bpv, int c) { return c * kAttrBuckets * attr_positions(bpv); }

struct AttrInfo {
  int version;          // 1 | 4 | 8 | 13 (attr_parse_kind), 2 | 7 | 11 | 14 | 25 | 26 | 28 | 31 (attr2_parse_kind)
  uint32_t max_error;   // e of versions 4, 7, 13, 14, 28 and 31 (0: lossless, and every blob without points)
  int cross;            // m of the cross-channel kinds (bit ch - 1: channel ch is coded against ch - 1), 0: a plain kind
  int bpv, c, nctx;
  int64_t n, S, nc;
  int64_t off_p0, off_table, off_payload, payload_words;
};

static inline uint32_t attr_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// S (points per lane) and the chunk count of a frame of n points with c channels: as few chunks as the 512 values per
// lane allow, the points spread evenly over their lanes
static inline void attr_layout(int64_t n, int c, int64_t* S, int64_t* nc) {
  const int64_t smax = kAttrMaxValues / c;
  int64_t k = (n + kAttrLanes * smax - 1) / (kAttrLanes * smax);
  if (k < 1) k = 1;
  int64_t s = (n + kAttrLanes * k - 1) / (kAttrLanes * k);
  if (s < 1) s = 1;
  *S = s;
  *nc = k;
}

// the largest e of a value width: e < 2^(8 bpv - 1)
ATTR_HD static inline uint32_t attr_max_error(int bpv) { return (1u << (8 * bpv - 1)) - 1u; }

// the eight kinds of attribute blob: what a version byte says; false for every other byte
static inline bool attr_kind(int version, bool* scalable, bool* nl, bool* cross) {
  const int plain = version == 8 ? 1 : (version == 11 ? 2 : (version == 13 ? 4 : (version == 14 ? 7 : version)));
  if (plain != 1 && plain != 2 && plain != 4 && plain != 7) return false;
  *scalable = plain == 2 || plain == 7;
  *nl = plain == 4 || plain == 7;
  *cross = plain != version;
  return true;
}
ATTR_HD static inline int attr_version(bool scalable, bool nl, bool cross) {
  return cross ? (scalable ? (nl ? 14 : 11) : (nl ? 13 : 8)) : (scalable ? (nl ? 7 : 2) : (nl ? 4 : 1));
}

// the ten lossless-or-bounded kinds: the eight above and versions 25 / 26, which are scalable, lossless, and *nbr
constexpr int kAttrNVersion = 25, kAttrNXVersion = 26;
static inline bool attr_kind(int version, bool* scalable, bool* nl, bool* cross, bool* nbr) {
  *nbr = version == kAttrNVersion || version == kAttrNXVersion;
  if (!*nbr) return attr_kind(version, scalable, nl, cross);
  *scalable = true;
  *nl = false;
  *cross = version == kAttrNXVersion;
  return true;
}
// versions 28 / 31, the bounded-error forms of 25 / 26 (nbr with nl): scalable too
constexpr int kAttrNLVersion = 28, kAttrNLXVersion = 31;
ATTR_HD static inline int attr_version(bool scalable, bool nl, bool cross, bool nbr) {
  return nbr ? (nl ? (cross ? kAttrNLXVersion : kAttrNLVersion) : (cross ? kAttrNXVersion : kAttrNVersion)) : attr_version(scalable, nl, cross);
}
// the two bounded-error neighbour kinds have a predicate of their own, and the twelve kinds one over both: the
// predicates above answer for their eight and ten bytes as before
static inline bool attr_nbr_nl_kind(int version, bool* cross) {
  *cross = version == kAttrNLXVersion;
  return version == kAttrNLVersion || version == kAttrNLXVersion;
}
static inline bool attr_kind12(int version, bool* scalable, bool* nl, bool* cross, bool* nbr) {
  if (!attr_nbr_nl_kind(version, cross)) return attr_kind(version, scalable, nl, cross, nbr);
  *scalable = *nl = *nbr = true;
  return true;
}

// byte 3 of a head: c channels (1 .. 4) and, in a cross kind, the mask m above them (m != 0, bits below c - 1 only); a
// plain kind has nothing above c
static inline bool attr_channels(uint8_t b3, bool cross, int* c, int* m) {
  *c = cross ? b3 & 15 : b3;
  *m = cross ? b3 >> 4 : 0;
  return *c >= 1 && *c <= 4 && (!cross || (*m != 0 && *m < (1 << (*c - 1))));
}

// the nctx initial probabilities at b + off lie in [16, 4080]; else *bad_p is the first that does not
static inline bool attr_check_p0(const uint8_t* b, int64_t off, int nctx, uint32_t* bad_p) {
  for (int i = 0; i < nctx; ++i) {
    const uint32_t p = (uint32_t)b[off + 2 * i] | ((uint32_t)b[off + 2 * i + 1] << 8);
    if (p < 16 || p > 4080) {
      *bad_p = p;
      return false;
    }
  }
  return true;
}

// *words = the sum of a chunk table's nc entries; false at the first chunk (*bad_k) whose words (*bad_cw) a chunk cannot
// have: a lane codes at most 512 values of at most 16 bpv decisions, one word each
static inline bool attr_sum_chunks(const uint8_t* table, int64_t nc, int bpv, int64_t* words, int64_t* bad_k, int64_t* bad_cw) {
  *words = 0;
  for (int64_t k = 0; k < nc; ++k) {
    const int64_t cw = (int64_t)attr_u32(table + 4 * k);
    if (cw < 3 * kAttrLanes || cw > 3 * kAttrLanes + (int64_t)kAttrLanes * kAttrMaxValues * attr_positions(bpv)) {
      *bad_k = k;
      *bad_cw = cw;
      return false;
    }
    *words += cw;
  }
  return true;
}

// version 1 (nl = false) or 4 (nl = true): x = 4 bytes of max_error move everything behind payload_len; cross: their
// cross-channel forms 8 and 13, the mask above the channels of byte 3
static inline int attr_parse_kind(const uint8_t* b, int64_t len, bool nl, AttrInfo* o, bool cross = false) {
  const char* tag = cross ? (nl ? " v13" : " v8") : (nl ? " v4" : "");
  const int x = nl ? 4 : 0;
  if (!b || len < kAttrHead || b[0] != 'A' || b[1] != attr_version(false, nl, cross)) {
    pcc_set_error("attribute blob%s: bad header (len=%lld)", tag, (long long)len);
    return PCC_E_STREAM;
  }
  o->version = b[1];
  o->max_error = 0;
  o->bpv = b[2];
  if ((o->bpv != 1 && o->bpv != 2) || !attr_channels(b[3], cross, &o->c, &o->cross)) {
    pcc_set_error("attribute blob%s: %d bytes per value, %d channels%s", tag, o->bpv, o->c, cross ? ", or their mask" : "");
    return PCC_E_STREAM;
  }
  o->nctx = attr_contexts(o->bpv, o->c);
  o->n = (int64_t)attr_u32(b + 4);
  const int64_t payload = (int64_t)attr_u32(b + 8);
  if (kAttrHead + payload != len) {
    pcc_set_error("attribute blob%s: payload of %lld bytes in a blob of %lld", tag, (long long)payload, (long long)len);
    return PCC_E_STREAM;
  }
  o->S = o->nc = 0;
  o->off_p0 = o->off_table = o->off_payload = len;
  o->payload_words = 0;
  if (o->n == 0) {
    if (payload != 0) {
      pcc_set_error("attribute blob%s: no points, %lld bytes of payload", tag, (long long)payload);
      return PCC_E_STREAM;
    }
    return PCC_OK;
  }
  if (o->n >= ((int64_t)1 << 27) || payload < 8 + x) {
    pcc_set_error("attribute blob%s: %lld points, payload %lld", tag, (long long)o->n, (long long)payload);
    return PCC_E_STREAM;
  }
  if (nl) {
    o->max_error = attr_u32(b + kAttrHead);
    if (o->max_error < 1 || o->max_error > attr_max_error(o->bpv)) {
      pcc_set_error("attribute blob%s: max_error %u with %d bytes per value", tag, o->max_error, o->bpv);
      return PCC_E_STREAM;
    }
  }
  o->S = (int64_t)attr_u32(b + kAttrHead + x);
  o->nc = (int64_t)attr_u32(b + kAttrHead + x + 4);
  if (o->S < 1 || o->S * o->c > kAttrMaxValues || o->nc < 1 || o->nc > o->n || kAttrLanes * o->S * o->nc < o->n ||
      kAttrLanes * o->S * (o->nc - 1) >= o->n) {
    pcc_set_error("attribute blob%s: %lld points in %lld chunks of 64 x %lld", tag, (long long)o->n, (long long)o->nc, (long long)o->S);
    return PCC_E_STREAM;
  }
  o->off_p0 = kAttrHead + 8 + x;
  o->off_table = o->off_p0 + 2 * (int64_t)o->nctx;
  if (o->off_table + 4 * o->nc > len) {
    pcc_set_error("attribute blob%s: truncated header (%lld chunks)", tag, (long long)o->nc);
    return PCC_E_STREAM;
  }
  uint32_t bad_p = 0;
  if (!attr_check_p0(b, o->off_p0, o->nctx, &bad_p)) {
    pcc_set_error("attribute blob%s: initial probability %u", tag, bad_p);
    return PCC_E_STREAM;
  }
  int64_t words = 0, bad_k = 0, bad_cw = 0;
  if (!attr_sum_chunks(b + o->off_table, o->nc, o->bpv, &words, &bad_k, &bad_cw)) {
    pcc_set_error("attribute blob%s: chunk %lld has %lld words", tag, (long long)bad_k, (long long)bad_cw);
    return PCC_E_STREAM;
  }
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  if (o->off_payload + 2 * words != len) {
    pcc_set_error("attribute blob%s: chunks take %lld bytes, blob has %lld", tag, (long long)(2 * words),
                  (long long)(len - o->off_payload));
    return PCC_E_STREAM;
  }
  return PCC_OK;
}

static inline int attr_parse(const uint8_t* b, int64_t len, AttrInfo* o) { return attr_parse_kind(b, len, false, o); }

// ---- version 2 ---------------------------------------------------------------------------------------------------
constexpr int kAttr2Head = kAttrHead + 64 + 8;   // .. | u32 cells[16] | u32 S | u32 n_chunks
constexpr int kAttrMaxLod = 15;

struct Attr2Info : AttrInfo {
  int slod;   // the sender's level of detail
  int64_t cells[16];
};

// the plan of one level of detail of a version-2 blob
struct Attr2Plan {
  int lod;
  int64_t m;               // values
  int64_t chunks, lanes;   // chunks needed (c* + 1) and lanes needed of the last of them (l* + 1)
  int64_t bytes;           // the shortest prefix that decodes
  int64_t last_off;        // where the last needed chunk starts, in 16-bit words from off_payload
  int64_t last_words;      // its words inside that prefix: 192 + len[0] + .. + len[l*] (lod 0: all of its words)
};

#define ATTR2_REQUIRE(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      pcc_set_error(__VA_ARGS__);  \
      return PCC_E_STREAM;         \
    }                              \
  } while (0)

// the plan of level of detail `lod` of a blob whose header o holds (S, the chunk table at off_table, off_payload,
// payload_words): m values, the first m of the coding order (lod 0: all n, the whole blob of `total` bytes).  b[0 .. len)
// reaches the chunk table; need_all: the plan's bytes must be there, else only the last needed chunk's length table
static inline int attr_lod_plan(const uint8_t* b, int64_t len, int lod, bool need_all, int tag, const AttrInfo& o, int64_t m, int64_t total,
                                Attr2Plan* pl) {
  const uint8_t* q = b + o.off_table;
  if (lod == 0) {
    const int64_t last = (int64_t)attr_u32(q + 4 * (o.nc - 1));
    pl->m = o.n;
    pl->chunks = o.nc;
    pl->lanes = kAttrLanes;
    pl->bytes = total;
    pl->last_off = o.payload_words - last;
    pl->last_words = last;
    return PCC_OK;
  }
  pl->m = m;
  const int64_t lanes = (pl->m + o.S - 1) / o.S, cs = (lanes - 1) / kAttrLanes, ls = (lanes - 1) % kAttrLanes;
  for (int64_t k = 0; k < cs; ++k) pl->last_off += (int64_t)attr_u32(q + 4 * k);
  const int64_t cw = (int64_t)attr_u32(q + 4 * cs);
  const int64_t at = o.off_payload + 2 * pl->last_off;   // the chunk: 128 state words, then its length table
  ATTR2_REQUIRE(len >= at + 2 * 3 * kAttrLanes, "attribute blob v%d: truncated in front of the length table of chunk %lld", tag,
                (long long)cs);
  int64_t run = 3 * kAttrLanes;
  for (int64_t l = 0; l <= ls; ++l) run += (int64_t)b[at + 4 * kAttrLanes + 2 * l] | ((int64_t)b[at + 4 * kAttrLanes + 2 * l + 1] << 8);
  ATTR2_REQUIRE(run <= cw, "attribute blob v%d: the runs of chunk %lld take %lld words of its %lld", tag, (long long)cs, (long long)run,
                (long long)cw);
  pl->chunks = cs + 1;
  pl->lanes = ls + 1;
  pl->last_words = run;
  pl->bytes = at + 2 * run;
  ATTR2_REQUIRE(!need_all || pl->bytes <= len, "attribute blob v%d: truncated (level of detail %d needs %lld bytes, %lld are here)", tag, lod,
                (long long)pl->bytes, (long long)len);
  return PCC_OK;
}

// b[0 .. len): the blob, or a prefix of it.  need_all: the decoder's form — the plan's bytes must be present (lod 0: the
// blob, whole and nothing behind it); otherwise (pcc_attr_lod_info) the bytes must only reach what the plan is computed
// from, the last needed chunk's length table.  Nothing beyond b[len) is read.
// Version 2 (nl = false) or 7 (nl = true, x = 4 bytes of max_error in front of cells[16]); cross: their cross-channel
// forms 11 and 14, the mask above the channels of byte 3.  nbr: versions 25 and 26 (nl = false) and 28 and 31 (nl = true),
// the layouts of 2, 11, 7 and 14 under their own version bytes.
static inline int attr2_parse_kind(const uint8_t* b, int64_t len, int lod, bool need_all, bool nl, Attr2Info* o, Attr2Plan* pl,
                                   bool cross = false, bool nbr = false) {
  const int tag = attr_version(true, nl, cross, nbr), x = nl ? 4 : 0;
  ATTR2_REQUIRE(b && len >= kAttrHead && b[0] == 'A' && b[1] == tag, "attribute blob v%d: bad header (len=%lld)", tag, (long long)len);
  o->version = tag;
  o->max_error = 0;
  o->bpv = b[2] & 15;
  o->slod = b[2] >> 4;
  ATTR2_REQUIRE((o->bpv == 1 || o->bpv == 2) && attr_channels(b[3], cross, &o->c, &o->cross),
                "attribute blob v%d: %d bytes per value, %d channels%s", tag, o->bpv, o->c, cross ? ", or their mask" : "");
  o->nctx = attr_contexts(o->bpv, o->c);
  o->n = (int64_t)attr_u32(b + 4);
  const int64_t payload = (int64_t)attr_u32(b + 8), total = kAttrHead + payload;
  ATTR2_REQUIRE(len <= total, "attribute blob v%d: payload of %lld bytes in a blob of %lld", tag, (long long)payload, (long long)len);
  ATTR2_REQUIRE(!(need_all && lod == 0) || len == total, "attribute blob v%d: truncated (%lld bytes of %lld)", tag, (long long)len,
                (long long)total);
  o->S = o->nc = 0;
  o->off_p0 = o->off_table = o->off_payload = kAttrHead;
  o->payload_words = 0;
  for (int k = 0; k < 16; ++k) o->cells[k] = 0;
  pl->lod = lod;
  pl->m = pl->chunks = pl->lanes = pl->last_off = pl->last_words = 0;
  pl->bytes = kAttrHead;
  if (o->n == 0) {
    ATTR2_REQUIRE(payload == 0, "attribute blob v%d: no points, %lld bytes of payload", tag, (long long)payload);
    return PCC_OK;
  }
  o->off_p0 = kAttr2Head + x;
  o->off_table = o->off_p0 + 2 * (int64_t)o->nctx;
  ATTR2_REQUIRE(o->n < ((int64_t)1 << 27) && payload >= o->off_table - kAttrHead + 4 + 2 * 3 * kAttrLanes,
                "attribute blob v%d: %lld points, payload %lld", tag, (long long)o->n, (long long)payload);
  ATTR2_REQUIRE(len >= o->off_table, "attribute blob v%d: truncated header", tag);
  if (nl) {
    o->max_error = attr_u32(b + kAttrHead);
    ATTR2_REQUIRE(o->max_error >= 1 && o->max_error <= attr_max_error(o->bpv), "attribute blob v%d: max_error %u with %d bytes per value",
                  tag, o->max_error, o->bpv);
  }
  for (int k = 0; k < 16; ++k) {
    o->cells[k] = (int64_t)attr_u32(b + kAttrHead + x + 4 * k);
    ATTR2_REQUIRE(k == 0 ? o->cells[0] == o->n : (o->cells[k] >= 1 && o->cells[k] <= o->cells[k - 1] && 8 * o->cells[k] >= o->cells[k - 1]),
                  "attribute blob v%d: level of detail %d has %lld values", tag, k, (long long)o->cells[k]);
  }
  o->S = (int64_t)attr_u32(b + kAttrHead + x + 64);
  o->nc = (int64_t)attr_u32(b + kAttrHead + x + 68);
  ATTR2_REQUIRE(o->S >= 1 && o->S * o->c <= kAttrMaxValues && o->nc >= 1 && o->nc <= o->n && kAttrLanes * o->S * o->nc >= o->n &&
                    kAttrLanes * o->S * (o->nc - 1) < o->n,
                "attribute blob v%d: %lld points in %lld chunks of 64 x %lld", tag, (long long)o->n, (long long)o->nc, (long long)o->S);
  uint32_t bad_p = 0;
  ATTR2_REQUIRE(attr_check_p0(b, o->off_p0, o->nctx, &bad_p), "attribute blob v%d: initial probability %u", tag, bad_p);
  ATTR2_REQUIRE(total - o->off_table >= 4 * o->nc, "attribute blob v%d: truncated chunk table", tag);
  ATTR2_REQUIRE(len - o->off_table >= 4 * o->nc, "attribute blob v%d: truncated inside the chunk table", tag);
  const uint8_t* q = b + o->off_table;
  int64_t words = 0, bad_k = 0, bad_cw = 0;
  ATTR2_REQUIRE(attr_sum_chunks(q, o->nc, o->bpv, &words, &bad_k, &bad_cw), "attribute blob v%d: chunk %lld has %lld words", tag,
                (long long)bad_k, (long long)bad_cw);
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  ATTR2_REQUIRE(o->off_payload + 2 * words == total, "attribute blob v%d: chunks take %lld bytes, blob has %lld", tag,
                (long long)(2 * words), (long long)(total - o->off_payload));
  return attr_lod_plan(b, len, lod, need_all, tag, *o, o->cells[lod], total, pl);
}

static inline int attr2_parse(const uint8_t* b, int64_t len, int lod, bool need_all, Attr2Info* o, Attr2Plan* pl) {
  return attr2_parse_kind(b, len, lod, need_all, false, o, pl);
}

// ---- version 19: transform-coded attributes ------------------------------------------------------------------------
// A ninth kind, lossy, for rates below about a byte per point (compress(..., qstep=q)): an integer lifting form of the
// region-adaptive hierarchical transform over the binary splits of the Morton tree.  Version 4's layout with version 2's
// slod nibble:
//
//   'A' 19 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 qstep | u32 S | u32 n_chunks | u16 p0[nctx] |
//   u32 words[n_chunks] | chunk payloads                  (n == 0: the 12 bytes up to payload_len = 0; they record no q)
//
// Byte 19 keeps the odd parity of the eight bytes above, so it differs from each of them in two bits; it is not one of
// attr_kind's and has its own predicate (attr_t_kind) and parser (attr_t_parse, over attr_tc_parse below).
// The frame's n distinct points in Morton order, their 48-bit keys key_i (biased by 32768 >> slod) and merged values v_i
// per channel; H = 2^(8 bpv - 1), mask = 2 H - 1, q = qstep in 1 .. H - 1:
//   sublevel of introduction   b(0) = 48; b(i) = hb(key_i xor key_{i-1}) in 0 .. 47: point i is the first leaf of the
//                              RIGHT child of exactly one binary split of the Morton tree, the one at bit b(i) (version
//                              2's size of introduction at bit granularity, s = floor(b / 3))
//   the pair of point i, b(i) = t:  lo = lower_bound(keys, key_i with its low t + 1 bits cleared), hi = lower_bound(keys,
//                              (key_i | (2^t - 1)) + 1) within the frame; wa = i - lo, wb = hi - i, w = wa + wb: the
//                              leaves of the left child, of the right child, of the node
//   step                       s = max(2, isqrt(floor(q^2 w / (wa wb))))        (the product stays below 2^63)
// Forward, val = v as signed integers never clamped inside, sublevels t = 0, 1, .., 47 in that order, the pairs of a
// sublevel independent of each other (no two touch the same slot):
//   h = val[i] - val[lo];  val[lo] += floor(wb h / w) (towards -inf: the node's value, kept at its first leaf)
//   x[i] = sgn(h) min(floor((|h| + floor(s / 2)) / s), H - 1)     (s >= 2 and |h| <= mask: the min moves an index by at
//                                                                  most 1)
// and after sublevel 47  x[0] = val[0] - H, the frame's integer weighted mean, in [-H, H), not quantised.
// Inverse, val[0] = x[0] + H, sublevels t = 47 .. 0 with the same lo, hi, wa, wb, s:
//   h^ = x[i] s;  va = val[lo] - floor(wb h^ / w);  val[lo] = va;  val[i] = va + h^;      output clamp(val, 0, mask)
// A step of 1 would let the min clamp indices (it cost the first form of this kind 10 dB), hence the floor of 2: the
// kind has no lossless setting.
// Coding order: (b descending, Morton index ascending), point 0 first.  x in that order is dealt to lanes and chunks
// (attr_layout) and coded exactly as version 2 codes its residuals — binarisation, contexts (channel, bucket of |x| of
// the channel's previous point in the lane's run, position; the buckets are not retuned), p0 and model, no prediction
// inside the run.  The decoder needs the frame's keys, so the kind decodes against the cells of its geometry at lod 0 and
// has no level-of-detail prefixes: a decoder at a cut does not know how many points lie under a cell and cannot form the
// weights.  tests/attr_transform_ref.py restates the kind in numpy.
constexpr int kAttrTVersion = 19;
constexpr int kAttrTHead = kAttrHead + 12;   // .. | u32 qstep | u32 S | u32 n_chunks

struct AttrTInfo : AttrInfo {
  int slod;          // the sender's level of detail
  uint32_t qstep;    // q (0: a blob without points)
};

static inline bool attr_t_kind(int version) { return version == kAttrTVersion; }

// ---- version 21: transform-coded attributes with a colour transform and one step per channel ------------------------
// A tenth kind (compress(..., qstep=(q0, q1, ..)) and compress(..., qstep=q, colour="ycocg")): version 19 with a colour
// word and c steps where version 19 keeps its one q:
//
//   'A' 21 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 colour | u32 q[c] | u32 S | u32 n_chunks | u16 p0[nctx] |
//   u32 words[n_chunks] | chunk payloads                  (n == 0: the 12 bytes up to payload_len = 0; they record
//                                                          neither colour nor steps)
//
// Byte 21 = 10101b has odd parity as the nine bytes above, so it differs from each of them in two bits; it has its own
// predicate (attr_c_kind) and parser (attr_c_parse, over attr_tc_parse below), and every other parser refuses it.
// Everything is version 19's — keys, sublevels, pairs, weights, forward and inverse lift, the mean, coding order,
// entropy stage, the clamp of an index at H - 1 — except:
//   steps      q[ch] in 1 .. H - 1 for every channel ch < c; the step of a pair in channel ch is
//              s[ch] = max(2, isqrt(floor(q[ch]^2 w / (wa wb)))).  With all q[ch] equal and colour = 0 the indices are
//              exactly version 19's; only the head differs.
//   colour     0: none.  1 (frames with c >= 3; channels 0, 1, 2 = R, G, B, a fourth channel is untouched): applied to
//              the merged values of every distinct point after the merge and before the first lift.  Signed integers,
//              >> the arithmetic shift (floor), H = 2^(8 bpv - 1), mask = 2 H - 1:
//                co = R - B;  t = B + (co >> 1);  cg = G - t;  y = t + (cg >> 1)
//                Y = y,  Co = (co >> 1) + H,  Cg = (cg >> 1) + H                      all three in 0 .. mask
//              YCoCg-R with the low bit of each chroma difference dropped, so the three values fit the value width and
//              a node's value stays a uint16.  Inverse, applied to the inverse lift's output after its clamp to
//              0 .. mask, then clamped again per channel:
//                co' = 2 (Co - H);  cg' = 2 (Cg - H);  t = Y - (cg' >> 1)
//                G = cg' + t;  B = t - (co' >> 1);  R = B + co'
//              Without quantisation the round trip moves no channel by more than 1.  Anything but 0 and 1, and 1 with
//              c < 3, is PCC_E_STREAM.
// tests/attr_colour_ref.py restates the kind in numpy.
constexpr int kAttrCVersion = 21;

struct AttrCInfo : AttrTInfo {
  uint32_t colour;   // 0 | 1 (0: a blob without points)
  uint32_t q[4];     // q[ch], ch < c (0s: a blob without points); qstep stays 0
};

static inline bool attr_c_kind(int version) { return version == kAttrCVersion; }
static inline int attr_c_head(int c) { return kAttrHead + 4 + 4 * c + 8; }   // .. | u32 colour | u32 q[c] | u32 S | u32 n_chunks

// ---- versions 19 and 21: one parser ----------------------------------------------------------------------------------
// b[0 .. len): the whole blob, and nothing behind it; or (prefix: pcc_attr_info, pcc_attr_qstep, pcc_attr_transform_info)
// the blob or a prefix of it that reaches its last step (q of version 19: 16 bytes; q[c - 1] of version 21: 16 + 4 c),
// of which every part of the header that is there is checked as the whole blob's is — S and n_chunks against n and the
// blob's announced length, p0, the chunk table against that length.  Nothing beyond b[len) is read.
// oc: where version 21's colour word and steps go (o itself as an AttrCInfo); nullptr: version 19.  The two heads differ
// in what stands between payload_len and S: one q, or the colour word and c steps.
static inline int attr_tc_parse(const uint8_t* b, int64_t len, AttrTInfo* o, AttrCInfo* oc, bool prefix) {
  const int v = oc ? kAttrCVersion : kAttrTVersion;
  ATTR2_REQUIRE(b && len >= kAttrHead && b[0] == 'A' && b[1] == v, "attribute blob v%d: bad header (len=%lld)", v, (long long)len);
  o->version = v;
  o->max_error = 0;
  o->cross = 0;
  o->qstep = 0;
  if (oc) oc->colour = 0;
  for (int ch = 0; oc && ch < 4; ++ch) oc->q[ch] = 0;
  o->bpv = b[2] & 15;
  o->slod = b[2] >> 4;
  o->c = b[3];
  ATTR2_REQUIRE((o->bpv == 1 || o->bpv == 2) && o->c >= 1 && o->c <= 4 && o->slod <= kAttrMaxLod,
                "attribute blob v%d: %d bytes per value, %d channels", v, o->bpv, o->c);
  o->nctx = attr_contexts(o->bpv, o->c);
  o->n = (int64_t)attr_u32(b + 4);
  const int64_t payload = (int64_t)attr_u32(b + 8), total = kAttrHead + payload;
  ATTR2_REQUIRE(prefix ? len <= total : len == total, "attribute blob v%d: payload of %lld bytes in a blob of %lld", v, (long long)payload,
                (long long)len);
  o->S = o->nc = 0;
  o->off_p0 = o->off_table = o->off_payload = kAttrHead;
  o->payload_words = 0;
  if (o->n == 0) {
    ATTR2_REQUIRE(payload == 0, "attribute blob v%d: no points, %lld bytes of payload", v, (long long)payload);
    return PCC_OK;
  }
  const int head = oc ? attr_c_head(o->c) : kAttrTHead;   // S and n_chunks are its last 8 bytes
  o->off_p0 = head;
  o->off_table = o->off_p0 + 2 * (int64_t)o->nctx;
  ATTR2_REQUIRE(o->n < ((int64_t)1 << 27) && payload >= o->off_table - kAttrHead + 4 + 2 * 3 * kAttrLanes,
                "attribute blob v%d: %lld points, payload %lld", v, (long long)o->n, (long long)payload);
  ATTR2_REQUIRE(len >= head - 8, "attribute blob v%d: truncated in front of %s (len=%lld)", v, oc ? "its steps" : "qstep", (long long)len);
  if (oc) {
    oc->colour = attr_u32(b + kAttrHead);
    ATTR2_REQUIRE(oc->colour <= 1 && (oc->colour == 0 || o->c >= 3), "attribute blob v21: colour transform %u with %d channels", oc->colour,
                  o->c);
    for (int ch = 0; ch < o->c; ++ch) {
      oc->q[ch] = attr_u32(b + kAttrHead + 4 + 4 * ch);
      ATTR2_REQUIRE(oc->q[ch] >= 1 && oc->q[ch] <= attr_max_error(o->bpv), "attribute blob v21: qstep %u of channel %d with %d bytes per value",
                    oc->q[ch], ch, o->bpv);
    }
  } else {
    o->qstep = attr_u32(b + kAttrHead);
    ATTR2_REQUIRE(o->qstep >= 1 && o->qstep <= attr_max_error(o->bpv), "attribute blob v19: qstep %u with %d bytes per value", o->qstep,
                  o->bpv);
  }
  if (len < head && prefix) return PCC_OK;
  ATTR2_REQUIRE(len >= head, "attribute blob v%d: truncated header", v);
  o->S = (int64_t)attr_u32(b + head - 8);
  o->nc = (int64_t)attr_u32(b + head - 4);
  ATTR2_REQUIRE(o->S >= 1 && o->S * o->c <= kAttrMaxValues && o->nc >= 1 && o->nc <= o->n && kAttrLanes * o->S * o->nc >= o->n &&
                    kAttrLanes * o->S * (o->nc - 1) < o->n,
                "attribute blob v%d: %lld points in %lld chunks of 64 x %lld", v, (long long)o->n, (long long)o->nc, (long long)o->S);
  ATTR2_REQUIRE(total - o->off_table >= 4 * o->nc, "attribute blob v%d: truncated chunk table", v);
  if (len < o->off_table && prefix) return PCC_OK;
  ATTR2_REQUIRE(len >= o->off_table, "attribute blob v%d: truncated header", v);
  uint32_t bad_p = 0;
  ATTR2_REQUIRE(attr_check_p0(b, o->off_p0, o->nctx, &bad_p), "attribute blob v%d: initial probability %u", v, bad_p);
  if (len - o->off_table < 4 * o->nc && prefix) return PCC_OK;
  int64_t words = 0, bad_k = 0, bad_cw = 0;
  ATTR2_REQUIRE(attr_sum_chunks(b + o->off_table, o->nc, o->bpv, &words, &bad_k, &bad_cw), "attribute blob v%d: chunk %lld has %lld words", v,
                (long long)bad_k, (long long)bad_cw);
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  ATTR2_REQUIRE(o->off_payload + 2 * words == total, "attribute blob v%d: chunks take %lld bytes, blob has %lld", v, (long long)(2 * words),
                (long long)(total - o->off_payload));
  return PCC_OK;
}

static inline int attr_t_parse(const uint8_t* b, int64_t len, AttrTInfo* o, bool prefix = false) {
  return attr_tc_parse(b, len, o, nullptr, prefix);
}
static inline int attr_c_parse(const uint8_t* b, int64_t len, AttrCInfo* o, bool prefix = false) {
  return attr_tc_parse(b, len, o, o, prefix);
}

// ---- version 22: transform-coded attributes with level-of-detail prefixes -------------------------------------------
// An eleventh kind (compress(..., qstep=.., scalable_to=K)): version 21 with weights that a decoder at a cut can form,
// so that the coefficients of every level of detail 0 .. K are a prefix of the blob as version 2's values are.
//
//   'A' 22 (bpv | slod << 4) c | u32 n | u32 payload_len | u32 colour | u32 q[c] | u32 K | u32 count[16] | u32 S |
//   u32 n_chunks | u16 p0[nctx] | u32 words[n_chunks] | chunk payloads      (n == 0: the 12 bytes up to payload_len = 0)
//
// Byte 22 = 10110b has odd parity as the ten bytes above; it has its own predicate (attr_s_kind) and parser
// (attr_s_parse), and every other parser refuses it.  count[j] = #{i : b(i) >= 3 j}: version 2's cells[j].
// Everything is version 21's — keys, sublevels b(i), pairs lo / hi, x[0], coding order, entropy stage, the clamp of an
// index at H - 1, the colour word, one step q[ch] per channel — except the weights and the steps.  K = the sender's
// deepest cut, 1 <= K, slod + K <= 15:
//   K-cells    first(i) = 1 if i == 0 or key_i >> 3 K != key_{i-1} >> 3 K (that is b(i) >= 3 K); g(i) = the number of
//              firsts among points 0 .. i - 1, C = g(n) = count[K].  A node split at bit t >= 3 K begins and ends on
//              K-cell boundaries: g(b) - g(a) is the number of K-cells in [a, b)
//   scale      M = max(1, floor((2 n + C) / (2 C))): the rounded mean number of points in a K-cell
//   t >= 3 K   ca = g(i) - g(lo), cb = g(hi) - g(i), w = ca + cb take the places of version 19's wa, wb, w in both
//              lifts; s[ch] = max(2, isqrt(floor(q[ch]^2 w / (ca cb M))))      (q^2 w < 2^58, ca cb M < 2^55)
//   t < 3 K    (inside a K-cell; hi is not needed) forward val[lo] += floor(h / 2), inverse va = val[lo] - floor(h^ / 2);
//              s[ch] = max(2, isqrt(floor(2 q[ch]^2 / 2^floor(2 t / 3))))
// A decoder at a cut j, 0 <= j <= K, runs the same procedure on the m_j = count[j] cell keys kappa = key >> 3 j of its
// geometry at lod j (biased by 32768 >> (slod + j)): b'(r) = hb(kappa_r xor kappa_{r-1}), the absolute sublevel
// t = b' + 3 j, K-cells kappa >> 3 (K - j), the first m_j coefficients of the coding order, the inverse over sublevels
// 47 .. 3 j, M from the head's n and count[K].  Row r is the node value of cell r — the cell's mean under the rule's
// weights — clamped and colour-inverted as version 21's values are.  Cells that give another number of K-cells than
// count[K] are PCC_E_STREAM.  The prefix of lod j is version 2's (attr_lod_plan).  tests/attr_scalable_ref.py restates
// the kind in numpy.
constexpr int kAttrSVersion = 22;

struct AttrSInfo : AttrCInfo {
  int K;               // the deepest cut (0: a blob without points)
  int64_t cells[16];   // count[j]
};

static inline bool attr_s_kind(int version) { return version == kAttrSVersion; }
// .. | u32 colour | u32 q[c] | u32 K | u32 count[16] | u32 S | u32 n_chunks
static inline int attr_s_head(int c) { return kAttrHead + 4 + 4 * c + 4 + 64 + 8; }

enum AttrSMode {
  kAttrSDecode,   // the decoder's form: the plan's bytes must be there (lod 0: the blob, whole and nothing behind it)
  kAttrSPlan,     // pcc_attr_lod_info: the blob or a prefix that reaches the last needed chunk's length table
  kAttrSHead      // pcc_attr_info and its kin: the blob or a prefix that reaches K (20 + 4 c bytes); no plan, lod unread
};

// Nothing beyond b[len) is read.  lod above K: PCC_E_ARG (modes kAttrSDecode and kAttrSPlan)
static inline int attr_s_parse(const uint8_t* b, int64_t len, int lod, AttrSMode mode, AttrSInfo* o, Attr2Plan* pl) {
  const int v = kAttrSVersion;
  ATTR2_REQUIRE(b && len >= kAttrHead && b[0] == 'A' && b[1] == v, "attribute blob v%d: bad header (len=%lld)", v, (long long)len);
  o->version = v;
  o->max_error = 0;
  o->cross = 0;
  o->qstep = 0;
  o->colour = 0;
  o->K = 0;
  for (int ch = 0; ch < 4; ++ch) o->q[ch] = 0;
  for (int k = 0; k < 16; ++k) o->cells[k] = 0;
  o->bpv = b[2] & 15;
  o->slod = b[2] >> 4;
  o->c = b[3];
  ATTR2_REQUIRE((o->bpv == 1 || o->bpv == 2) && o->c >= 1 && o->c <= 4, "attribute blob v%d: %d bytes per value, %d channels", v, o->bpv,
                o->c);
  o->nctx = attr_contexts(o->bpv, o->c);
  o->n = (int64_t)attr_u32(b + 4);
  const int64_t payload = (int64_t)attr_u32(b + 8), total = kAttrHead + payload;
  ATTR2_REQUIRE(len <= total, "attribute blob v%d: payload of %lld bytes in a blob of %lld", v, (long long)payload, (long long)len);
  ATTR2_REQUIRE(!(mode == kAttrSDecode && lod == 0) || len == total, "attribute blob v%d: truncated (%lld bytes of %lld)", v, (long long)len,
                (long long)total);
  o->S = o->nc = 0;
  o->off_p0 = o->off_table = o->off_payload = kAttrHead;
  o->payload_words = 0;
  if (pl) {
    pl->lod = lod;
    pl->m = pl->chunks = pl->lanes = pl->last_off = pl->last_words = 0;
    pl->bytes = kAttrHead;
  }
  if (o->n == 0) {
    ATTR2_REQUIRE(payload == 0, "attribute blob v%d: no points, %lld bytes of payload", v, (long long)payload);
    return PCC_OK;
  }
  const int head = attr_s_head(o->c), at_k = kAttrHead + 4 + 4 * o->c;
  o->off_p0 = head;
  o->off_table = o->off_p0 + 2 * (int64_t)o->nctx;
  ATTR2_REQUIRE(o->n < ((int64_t)1 << 27) && payload >= o->off_table - kAttrHead + 4 + 2 * 3 * kAttrLanes,
                "attribute blob v%d: %lld points, payload %lld", v, (long long)o->n, (long long)payload);
  ATTR2_REQUIRE(len >= at_k + 4, "attribute blob v%d: truncated in front of scalable_to (len=%lld)", v, (long long)len);
  o->colour = attr_u32(b + kAttrHead);
  ATTR2_REQUIRE(o->colour <= 1 && (o->colour == 0 || o->c >= 3), "attribute blob v%d: colour transform %u with %d channels", v, o->colour,
                o->c);
  for (int ch = 0; ch < o->c; ++ch) {
    o->q[ch] = attr_u32(b + kAttrHead + 4 + 4 * ch);
    ATTR2_REQUIRE(o->q[ch] >= 1 && o->q[ch] <= attr_max_error(o->bpv), "attribute blob v%d: qstep %u of channel %d with %d bytes per value", v,
                  o->q[ch], ch, o->bpv);
  }
  const uint32_t K = attr_u32(b + at_k);
  ATTR2_REQUIRE(K >= 1 && (int64_t)K + o->slod <= kAttrMaxLod, "attribute blob v%d: scalable_to %u with the sender's level of detail %d", v, K,
                o->slod);
  o->K = (int)K;
  if (mode == kAttrSHead && len < o->off_table) return PCC_OK;
  ATTR2_REQUIRE(len >= o->off_table, "attribute blob v%d: truncated header", v);
  for (int k = 0; k < 16; ++k) {
    o->cells[k] = (int64_t)attr_u32(b + at_k + 4 + 4 * k);
    ATTR2_REQUIRE(k == 0 ? o->cells[0] == o->n : (o->cells[k] >= 1 && o->cells[k] <= o->cells[k - 1] && 8 * o->cells[k] >= o->cells[k - 1]),
                  "attribute blob v%d: level of detail %d has %lld values", v, k, (long long)o->cells[k]);
  }
  o->S = (int64_t)attr_u32(b + head - 8);
  o->nc = (int64_t)attr_u32(b + head - 4);
  ATTR2_REQUIRE(o->S >= 1 && o->S * o->c <= kAttrMaxValues && o->nc >= 1 && o->nc <= o->n && kAttrLanes * o->S * o->nc >= o->n &&
                    kAttrLanes * o->S * (o->nc - 1) < o->n,
                "attribute blob v%d: %lld points in %lld chunks of 64 x %lld", v, (long long)o->n, (long long)o->nc, (long long)o->S);
  uint32_t bad_p = 0;
  ATTR2_REQUIRE(attr_check_p0(b, o->off_p0, o->nctx, &bad_p), "attribute blob v%d: initial probability %u", v, bad_p);
  ATTR2_REQUIRE(total - o->off_table >= 4 * o->nc, "attribute blob v%d: truncated chunk table", v);
  if (mode == kAttrSHead && len - o->off_table < 4 * o->nc) return PCC_OK;
  ATTR2_REQUIRE(len - o->off_table >= 4 * o->nc, "attribute blob v%d: truncated inside the chunk table", v);
  int64_t words = 0, bad_k = 0, bad_cw = 0;
  ATTR2_REQUIRE(attr_sum_chunks(b + o->off_table, o->nc, o->bpv, &words, &bad_k, &bad_cw), "attribute blob v%d: chunk %lld has %lld words", v,
                (long long)bad_k, (long long)bad_cw);
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  ATTR2_REQUIRE(o->off_payload + 2 * words == total, "attribute blob v%d: chunks take %lld bytes, blob has %lld", v, (long long)(2 * words),
                (long long)(total - o->off_payload));
  if (mode == kAttrSHead) return PCC_OK;
  if (lod < 0 || lod > o->K) {
    pcc_set_error("attribute blob v%d: level of detail %d beyond its scalable_to %d", v, lod, o->K);
    return PCC_E_ARG;
  }
  return attr_lod_plan(b, len, lod, mode == kAttrSDecode, v, *o, o->cells[lod], total, pl);
}
