// octree4_blob.h — the host side of octree blob version 4, a PREDICTED frame (octree4.hip; include/pcc.h has the rule):
// its header, parsed and checked against the blob's length before anything is reserved or launched.  Plain C++ (no
// HIP): tests/fuzz/fuzz_octree4_header.cpp puts it under the sanitizers.
//
//   'O' 4 depth (W - 1) | u32 n | i32 origin[3] | u32 payload_len |
//   u32 level_n[depth] | u32 S | u32 n_chunks | u32 ref_n | u64 ref_sum | u16 p0[324] | u32 words[n_chunks] | chunks
//   chunk           = 64 x (state lo, state hi) | u16 len[64] | words of lane 0 | words of lane 1 | ..
//
// W - 1: the reference is the union of the W decoded frames in front of the blob's (0: the one frame, the bytes of
// before history=; the parser records any value, the decode entries refuse a window above 8).
// Version 2 (octree2_blob.h) with a context split in three by the reference byte of the node; a version-4 blob always
// has points (a frame without points is the 24-byte version-2 blob).  The checks are version 2's: every level at most 8
// times the one above and at most n, the chunk count what S and the node count make it, the chunk table's sum the
// payload's length — every size the decoder reserves or launches from is bounded by the blob's length.
//
// Levels of detail.  The layout of nodes, lanes and chunks is version 2's, so the levels above a cut are a prefix of
// the bytes here too: cut level, cells, nodes needed and shortest prefix are octree2_blob.h's formulas over this
// header's offsets (off_payload = 24 + 4 depth + 20 + 648 + 4 nc), O4Plan / o4_parse_lod below.  A node above the cut
// at lod k has child cubes of side >= 2^k, each a union of whole lod-k cells (the root corner is a multiple of 2^depth
// in biased coordinates, 32768 a multiple of 2^k), so its reference byte needs only the reference's CELLS at lod k.
// What a prefix cannot verify: the level sizes below the cut and n (bounded by the header checks alone), and ref_n /
// ref_sum, which describe the reference's full-resolution points.
#pragma once
#include <stdint.h>

#include "../../include/pcc.h"

void pcc_set_error(const char* fmt, ...);

constexpr int kO4Header = 24;
constexpr int kO4Ctx = 324;        // 3 (reference byte 0 / its bit 0 / its bit 1) x 108 of version 2
constexpr int kO4SLimit = 512;     // nodes per lane a decoder accepts
constexpr int kO4Lanes = 64;

struct O4Info {
  int depth;
  int window;             // W: byte 3 + 1
  int64_t n, n_nodes, S, nc, level_n[16];
  int32_t origin[3];
  uint32_t ref_n;
  uint64_t ref_sum;
  int64_t off_p0, off_table, off_payload, payload_words;
};

static inline uint32_t o4_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

#define O4_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      pcc_set_error(__VA_ARGS__);  \
      return PCC_E_STREAM;         \
    }                              \
  } while (0)

// the plan of one level of detail of that blob (octree2_blob.h has the formulas: they are version 2's over version 4's
// offsets)
struct O4Plan {
  int lod, Lc;             // cut level: the cells are the nodes of level Lc
  int64_t m, n_dec;        // cells; nodes needed N'
  int64_t chunks, lanes;   // chunks needed (c* + 1, or 0) and lanes needed of the last of them (l* + 1)
  int64_t bytes;           // the shortest prefix that decodes
  int64_t last_off;        // where the last needed chunk starts, in 16-bit words from off_payload
  int64_t last_words;      // its words inside that prefix: 192 + len[0] + .. + len[l*] (lod 0: all of its words)
};

// h_in[0 .. len): the blob, or a prefix of it (never more than the blob).  lod 0: the whole blob, whatever need_all.
// lod > 0 with need_all (the decoder's form): the plan's bytes must be present; without (pcc_octree_lod_info): the bytes
// must only reach what the plan is computed from, the last needed chunk's length table.  Nothing beyond h_in[len) is
// read.
static inline int o4_parse_lod(const uint8_t* h_in, int64_t len, int lod, bool need_all, O4Info* o, O4Plan* pl) {
  O4_REQUIRE(h_in && len >= kO4Header && h_in[0] == 'O' && h_in[1] == 4, "octree blob v4: bad header");
  o->depth = h_in[2];
  o->window = (int)h_in[3] + 1;
  o->n = (int64_t)o4_u32(h_in + 4);
  for (int a = 0; a < 3; ++a) o->origin[a] = (int32_t)o4_u32(h_in + 8 + 4 * a);
  const int64_t payload = (int64_t)o4_u32(h_in + 20);
  O4_REQUIRE(lod == 0 ? kO4Header + payload == len : kO4Header + payload >= len, "octree blob v4: %lld bytes announced, %lld are here",
             (long long)(kO4Header + payload), (long long)len);
  const int d = o->depth;
  O4_REQUIRE(o->n >= 1, "octree blob v4: no points (a frame without points is a version-2 blob)");
  O4_REQUIRE(d >= 1 && d <= 16 && payload >= 4 * d + 8 + 12 + 2 * kO4Ctx + 4, "octree blob v4: depth %d, payload %lld", d,
             (long long)payload);
  O4_REQUIRE(len >= kO4Header + 4 * d + 8 + 12 + 2 * kO4Ctx, "octree blob v4: truncated header");
  const uint8_t* q = h_in + kO4Header;
  o->n_nodes = 0;
  for (int L = 0; L < d; ++L, q += 4) {
    o->level_n[L] = (int64_t)o4_u32(q);
    o->n_nodes += o->level_n[L];
    O4_REQUIRE(o->level_n[L] >= 1 && (L == 0 ? o->level_n[0] == 1 : o->level_n[L] <= 8 * o->level_n[L - 1]) && o->level_n[L] <= o->n,
               "octree blob v4: level %d has %lld nodes", L, (long long)o->level_n[L]);
  }
  for (int L = d; L < 16; ++L) o->level_n[L] = 0;
  O4_REQUIRE(o->n <= 8 * o->level_n[d - 1] && o->n >= o->level_n[d - 1] && o->n_nodes < ((int64_t)1 << 28),
             "octree blob v4: %lld points under %lld nodes", (long long)o->n, (long long)o->level_n[d - 1]);
  o->S = (int64_t)o4_u32(q);
  o->nc = (int64_t)o4_u32(q + 4);
  o->ref_n = o4_u32(q + 8);
  o->ref_sum = (uint64_t)o4_u32(q + 12) | ((uint64_t)o4_u32(q + 16) << 32);
  q += 20;
  O4_REQUIRE(o->S >= 4 && o->S % 4 == 0 && o->S <= kO4SLimit && o->nc >= 1 && kO4Lanes * o->S * o->nc >= o->n_nodes &&
                 kO4Lanes * o->S * (o->nc - 1) < o->n_nodes,
             "octree blob v4: %lld nodes in %lld chunks of 64 x %lld", (long long)o->n_nodes, (long long)o->nc, (long long)o->S);
  O4_REQUIRE(o->ref_n >= 1, "octree blob v4: a reference without points");
  o->off_p0 = q - h_in;
  for (int i = 0; i < kO4Ctx; ++i, q += 2) {
    const uint32_t p = (uint32_t)q[0] | ((uint32_t)q[1] << 8);
    O4_REQUIRE(p >= 16 && p <= 4080, "octree blob v4: initial probability %u", p);
  }
  o->off_table = q - h_in;
  O4_REQUIRE(len - o->off_table >= 4 * o->nc, "octree blob v4: truncated chunk table");
  int64_t words = 0;
  for (int64_t c = 0; c < o->nc; ++c) {
    const int64_t cw = (int64_t)o4_u32(q + 4 * c);
    O4_REQUIRE(cw >= 3 * kO4Lanes, "octree blob v4: chunk %lld has no states", (long long)c);
    words += cw;
  }
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  O4_REQUIRE(o->off_payload + 2 * words == kO4Header + payload, "octree blob v4: chunks take %lld bytes, blob has %lld",
             (long long)(2 * words), (long long)(kO4Header + payload - o->off_payload));
  // the plan
  pl->lod = lod;
  pl->last_off = 0;
  if (lod == 0) {
    const int64_t last = (int64_t)o4_u32(q + 4 * (o->nc - 1));
    pl->Lc = d;
    pl->m = o->n;
    pl->n_dec = o->n_nodes;
    pl->chunks = o->nc;
    pl->lanes = kO4Lanes;
    pl->bytes = len;
    pl->last_off = words - last;
    pl->last_words = last;
    return PCC_OK;
  }
  pl->Lc = d > lod ? d - lod : 0;
  pl->m = pl->Lc ? o->level_n[pl->Lc] : 1;
  pl->n_dec = pl->chunks = pl->lanes = pl->last_words = 0;
  for (int L = 0; L < pl->Lc; ++L) pl->n_dec += o->level_n[L];
  pl->bytes = o->off_payload;
  if (pl->n_dec == 0) return PCC_OK;
  const int64_t lanes = (pl->n_dec + o->S - 1) / o->S, cs = (lanes - 1) / kO4Lanes, ls = (lanes - 1) % kO4Lanes;
  for (int64_t c = 0; c < cs; ++c) pl->last_off += (int64_t)o4_u32(q + 4 * c);
  const int64_t cw = (int64_t)o4_u32(q + 4 * cs);
  const int64_t at = o->off_payload + 2 * pl->last_off;   // the chunk: 128 state words, then its length table
  O4_REQUIRE(len >= at + 2 * 3 * kO4Lanes, "octree blob v4: truncated in front of the length table of chunk %lld", (long long)cs);
  int64_t run = 3 * kO4Lanes;
  for (int64_t l = 0; l <= ls; ++l) run += (int64_t)h_in[at + 4 * kO4Lanes + 2 * l] | ((int64_t)h_in[at + 4 * kO4Lanes + 2 * l + 1] << 8);
  O4_REQUIRE(run <= cw, "octree blob v4: the runs of chunk %lld take %lld words of its %lld", (long long)cs, (long long)run,
             (long long)cw);
  pl->chunks = cs + 1;
  pl->lanes = ls + 1;
  pl->last_words = run;
  pl->bytes = at + 2 * run;
  O4_REQUIRE(!need_all || pl->bytes <= len, "octree blob v4: truncated (level of detail %d needs %lld bytes, %lld are here)", lod,
             (long long)pl->bytes, (long long)len);
  return PCC_OK;
}

// h_in[0 .. len): the whole blob (lod 0).  Nothing beyond h_in[len) is read.
static inline int o4_parse(const uint8_t* h_in, int64_t len, O4Info* o) {
  O4Plan pl;
  return o4_parse_lod(h_in, len, 0, true, o, &pl);
}
