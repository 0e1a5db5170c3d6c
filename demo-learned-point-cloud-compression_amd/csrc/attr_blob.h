// attr_blob.h — the header of an attribute blob (attr.hip), parsed and checked on the host before anything is reserved
// or launched.  Plain C++ (no HIP): tests/fuzz/fuzz_attr_header.cpp and fuzz_attr2_header.cpp put it under the
// sanitizers.
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

static inline int attr_parse(const uint8_t* b, int64_t len, AttrInfo* o) {
  if (!b || len < kAttrHead || b[0] != 'A' || b[1] != 1) {
    pcc_set_error("attribute blob: bad header (len=%lld)", (long long)len);
    return PCC_E_STREAM;
  }
  o->bpv = b[2];
  o->c = b[3];
  if ((o->bpv != 1 && o->bpv != 2) || o->c < 1 || o->c > 4) {
    pcc_set_error("attribute blob: %d bytes per value, %d channels", o->bpv, o->c);
    return PCC_E_STREAM;
  }
  o->nctx = attr_contexts(o->bpv, o->c);
  o->n = (int64_t)attr_u32(b + 4);
  const int64_t payload = (int64_t)attr_u32(b + 8);
  if (kAttrHead + payload != len) {
    pcc_set_error("attribute blob: payload of %lld bytes in a blob of %lld", (long long)payload, (long long)len);
    return PCC_E_STREAM;
  }
  o->S = o->nc = 0;
  o->off_p0 = o->off_table = o->off_payload = len;
  o->payload_words = 0;
  if (o->n == 0) {
    if (payload != 0) {
      pcc_set_error("attribute blob: no points, %lld bytes of payload", (long long)payload);
      return PCC_E_STREAM;
    }
    return PCC_OK;
  }
  if (o->n >= ((int64_t)1 << 27) || payload < 8) {
    pcc_set_error("attribute blob: %lld points, payload %lld", (long long)o->n, (long long)payload);
    return PCC_E_STREAM;
  }
  o->S = (int64_t)attr_u32(b + kAttrHead);
  o->nc = (int64_t)attr_u32(b + kAttrHead + 4);
  if (o->S < 1 || o->S * o->c > kAttrMaxValues || o->nc < 1 || o->nc > o->n || kAttrLanes * o->S * o->nc < o->n ||
      kAttrLanes * o->S * (o->nc - 1) >= o->n) {
    pcc_set_error("attribute blob: %lld points in %lld chunks of 64 x %lld", (long long)o->n, (long long)o->nc, (long long)o->S);
    return PCC_E_STREAM;
  }
  o->off_p0 = kAttrHead + 8;
  o->off_table = o->off_p0 + 2 * (int64_t)o->nctx;
  if (o->off_table + 4 * o->nc > len) {
    pcc_set_error("attribute blob: truncated header (%lld chunks)", (long long)o->nc);
    return PCC_E_STREAM;
  }
  for (int i = 0; i < o->nctx; ++i) {
    const uint32_t p = (uint32_t)b[o->off_p0 + 2 * i] | ((uint32_t)b[o->off_p0 + 2 * i + 1] << 8);
    if (p < 16 || p > 4080) {
      pcc_set_error("attribute blob: initial probability %u", p);
      return PCC_E_STREAM;
    }
  }
  int64_t words = 0;
  for (int64_t k = 0; k < o->nc; ++k) {
    const int64_t cw = (int64_t)attr_u32(b + o->off_table + 4 * k);
    // a lane codes at most 512 values of at most 16 bpv decisions, one word each
    if (cw < 3 * kAttrLanes || cw > 3 * kAttrLanes + (int64_t)kAttrLanes * kAttrMaxValues * attr_positions(o->bpv)) {
      pcc_set_error("attribute blob: chunk %lld has %lld words", (long long)k, (long long)cw);
      return PCC_E_STREAM;
    }
    words += cw;
  }
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  if (o->off_payload + 2 * words != len) {
    pcc_set_error("attribute blob: chunks take %lld bytes, blob has %lld", (long long)(2 * words),
                  (long long)(len - o->off_payload));
    return PCC_E_STREAM;
  }
  return PCC_OK;
}

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

// b[0 .. len): the blob, or a prefix of it.  need_all: the decoder's form — the plan's bytes must be present (lod 0: the
// blob, whole and nothing behind it); otherwise (pcc_attr_lod_info) the bytes must only reach what the plan is computed
// from, the last needed chunk's length table.  Nothing beyond b[len) is read.
static inline int attr2_parse(const uint8_t* b, int64_t len, int lod, bool need_all, Attr2Info* o, Attr2Plan* pl) {
  ATTR2_REQUIRE(b && len >= kAttrHead && b[0] == 'A' && b[1] == 2, "attribute blob v2: bad header (len=%lld)", (long long)len);
  o->bpv = b[2] & 15;
  o->slod = b[2] >> 4;
  o->c = b[3];
  ATTR2_REQUIRE((o->bpv == 1 || o->bpv == 2) && o->c >= 1 && o->c <= 4, "attribute blob v2: %d bytes per value, %d channels",
                o->bpv, o->c);
  o->nctx = attr_contexts(o->bpv, o->c);
  o->n = (int64_t)attr_u32(b + 4);
  const int64_t payload = (int64_t)attr_u32(b + 8), total = kAttrHead + payload;
  ATTR2_REQUIRE(len <= total, "attribute blob v2: payload of %lld bytes in a blob of %lld", (long long)payload, (long long)len);
  ATTR2_REQUIRE(!(need_all && lod == 0) || len == total, "attribute blob v2: truncated (%lld bytes of %lld)", (long long)len,
                (long long)total);
  o->S = o->nc = 0;
  o->off_p0 = o->off_table = o->off_payload = kAttrHead;
  o->payload_words = 0;
  for (int k = 0; k < 16; ++k) o->cells[k] = 0;
  pl->lod = lod;
  pl->m = pl->chunks = pl->lanes = pl->last_off = pl->last_words = 0;
  pl->bytes = kAttrHead;
  if (o->n == 0) {
    ATTR2_REQUIRE(payload == 0, "attribute blob v2: no points, %lld bytes of payload", (long long)payload);
    return PCC_OK;
  }
  o->off_p0 = kAttr2Head;
  o->off_table = o->off_p0 + 2 * (int64_t)o->nctx;
  ATTR2_REQUIRE(o->n < ((int64_t)1 << 27) && payload >= o->off_table - kAttrHead + 4 + 2 * 3 * kAttrLanes,
                "attribute blob v2: %lld points, payload %lld", (long long)o->n, (long long)payload);
  ATTR2_REQUIRE(len >= o->off_table, "attribute blob v2: truncated header");
  for (int k = 0; k < 16; ++k) {
    o->cells[k] = (int64_t)attr_u32(b + kAttrHead + 4 * k);
    ATTR2_REQUIRE(k == 0 ? o->cells[0] == o->n : (o->cells[k] >= 1 && o->cells[k] <= o->cells[k - 1] && 8 * o->cells[k] >= o->cells[k - 1]),
                  "attribute blob v2: level of detail %d has %lld values", k, (long long)o->cells[k]);
  }
  o->S = (int64_t)attr_u32(b + kAttrHead + 64);
  o->nc = (int64_t)attr_u32(b + kAttrHead + 68);
  ATTR2_REQUIRE(o->S >= 1 && o->S * o->c <= kAttrMaxValues && o->nc >= 1 && o->nc <= o->n && kAttrLanes * o->S * o->nc >= o->n &&
                    kAttrLanes * o->S * (o->nc - 1) < o->n,
                "attribute blob v2: %lld points in %lld chunks of 64 x %lld", (long long)o->n, (long long)o->nc, (long long)o->S);
  for (int i = 0; i < o->nctx; ++i) {
    const uint32_t p = (uint32_t)b[o->off_p0 + 2 * i] | ((uint32_t)b[o->off_p0 + 2 * i + 1] << 8);
    ATTR2_REQUIRE(p >= 16 && p <= 4080, "attribute blob v2: initial probability %u", p);
  }
  ATTR2_REQUIRE(total - o->off_table >= 4 * o->nc, "attribute blob v2: truncated chunk table");
  ATTR2_REQUIRE(len - o->off_table >= 4 * o->nc, "attribute blob v2: truncated inside the chunk table");
  const uint8_t* q = b + o->off_table;
  int64_t words = 0;
  for (int64_t k = 0; k < o->nc; ++k) {
    const int64_t cw = (int64_t)attr_u32(q + 4 * k);
    // a lane codes at most 512 values of at most 16 bpv decisions, one word each
    ATTR2_REQUIRE(cw >= 3 * kAttrLanes && cw <= 3 * kAttrLanes + (int64_t)kAttrLanes * kAttrMaxValues * attr_positions(o->bpv),
                  "attribute blob v2: chunk %lld has %lld words", (long long)k, (long long)cw);
    words += cw;
  }
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  ATTR2_REQUIRE(o->off_payload + 2 * words == total, "attribute blob v2: chunks take %lld bytes, blob has %lld",
                (long long)(2 * words), (long long)(total - o->off_payload));
  // the plan
  if (lod == 0) {
    const int64_t last = (int64_t)attr_u32(q + 4 * (o->nc - 1));
    pl->m = o->n;
    pl->chunks = o->nc;
    pl->lanes = kAttrLanes;
    pl->bytes = total;
    pl->last_off = words - last;
    pl->last_words = last;
    return PCC_OK;
  }
  pl->m = o->cells[lod];
  const int64_t lanes = (pl->m + o->S - 1) / o->S, cs = (lanes - 1) / kAttrLanes, ls = (lanes - 1) % kAttrLanes;
  for (int64_t k = 0; k < cs; ++k) pl->last_off += (int64_t)attr_u32(q + 4 * k);
  const int64_t cw = (int64_t)attr_u32(q + 4 * cs);
  const int64_t at = o->off_payload + 2 * pl->last_off;   // the chunk: 128 state words, then its length table
  ATTR2_REQUIRE(len >= at + 2 * 3 * kAttrLanes, "attribute blob v2: truncated in front of the length table of chunk %lld",
                (long long)cs);
  int64_t run = 3 * kAttrLanes;
  for (int64_t l = 0; l <= ls; ++l) run += (int64_t)b[at + 4 * kAttrLanes + 2 * l] | ((int64_t)b[at + 4 * kAttrLanes + 2 * l + 1] << 8);
  ATTR2_REQUIRE(run <= cw, "attribute blob v2: the runs of chunk %lld take %lld words of its %lld", (long long)cs, (long long)run,
                (long long)cw);
  pl->chunks = cs + 1;
  pl->lanes = ls + 1;
  pl->last_words = run;
  pl->bytes = at + 2 * run;
  ATTR2_REQUIRE(!need_all || pl->bytes <= len, "attribute blob v2: truncated (level of detail %d needs %lld bytes, %lld are here)", lod,
                (long long)pl->bytes, (long long)len);
  return PCC_OK;
}
