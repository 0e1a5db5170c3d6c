// octree2_blob.h — the host side of blob version 2 (octree2.hip): its header, parsed and checked before anything is
// reserved or launched, and the plan of a LEVEL OF DETAIL — which prefix of the blob holds the levels above a cut, and
// what decoding them gives.  Plain C++ (no HIP): tests/fuzz/fuzz_octree2_header.cpp puts it under the sanitizers.
//
//   'O' 2 depth 0 | u32 n | i32 origin[3] | u32 payload_len |
//   u32 level_n[depth] | u32 S | u32 n_chunks | u16 p0[108] | u32 words[n_chunks] | chunk payloads (16-bit words)
//   chunk           = 64 x (state lo, state hi) | u16 len[64] | words of lane 0 | words of lane 1 | ..
//
// Levels of detail.  Nodes are numbered breadth-first and dealt to lanes and chunks in that order, the chunk table lies
// in front of the payload and every lane owns a contiguous run of words: the levels above a cut are a prefix of the
// bytes.  For n > 0 points, depth d and lod k in 0 .. 15 (16 is excluded: 32768 is not a multiple of 2^16, the two cells
// of the int16 range would not nest in a root cube):
//   cut level   Lc = max(d - k, 0)
//   cells       m  = n (k = 0), level_n[Lc] (0 < k < d), 1 (k >= d)
//   nodes       N' = level_n[0] + .. + level_n[Lc - 1]            (all of them for k = 0, none for k >= d)
//   result      int32 [m, 3] cell indices p >> k (arithmetic shift) of the frame's points, distinct, in Morton order:
//               the root cube is aligned to 2^d in biased coordinates, so the nodes of level Lc ARE the global cells.
//               Corner of a cell c << k, centre (c << k) + ((1 << k) >> 1).  k = 0 is the points themselves.
//   prefix      k = 0: the whole blob.  N' = 0: off_payload bytes (header, level table, S, nc, p0 and the WHOLE chunk
//               table are always needed).  Otherwise lanes = ceil(N' / S), c* = (lanes - 1) / 64, l* = (lanes - 1) % 64:
//               off_payload + 2 (words[0] + .. + words[c* - 1]) + 2 (192 + len[0] + .. + len[l*]), len being chunk c*'s
//               own length table.  Any longer prefix, the whole blob included, decodes to the same result.
//   An empty blob (24 bytes, n = 0) has 0 cells and needs its 24 bytes at every k.
// What a prefix cannot verify — the level sizes below the cut and n itself — stays bounded by the header checks alone
// (every level at most 8 times the one above and at most n); every size the decoder reserves from (N', m) is verified
// by the stream (k_o2_link).
#pragma once
#include <stdint.h>

#include "../../include/pcc.h"

void pcc_set_error(const char* fmt, ...);

constexpr int kO2Header = 24;
constexpr int kO2Ctx = 108;        // 3 level classes x 36 (bit position, ones so far)
constexpr int kO2SMax = 512;       // nodes per lane
constexpr int kO2Lanes = 64;
constexpr int kO2MaxLod = 15;

// header of a version-2 blob, checked against its length: everything a decoder sizes from
struct O2Info {
  int depth;
  int64_t n, n_nodes, S, nc, level_n[16];
  int32_t origin[3];
  int64_t off_p0, off_table, off_payload, payload_words;
};

// the plan of one level of detail of that blob
struct O2Plan {
  int lod, Lc;             // cut level: the cells are the nodes of level Lc
  int64_t m, n_dec;        // cells; nodes needed N'
  int64_t chunks, lanes;   // chunks needed (c* + 1, or 0) and lanes needed of the last of them (l* + 1)
  int64_t bytes;           // the shortest prefix that decodes
  int64_t last_off;        // where the last needed chunk starts, in 16-bit words from off_payload
  int64_t last_words;      // its words inside that prefix: 192 + len[0] + .. + len[l*] (lod 0: all of its words)
};

static inline uint32_t o2_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

#define O2_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      pcc_set_error(__VA_ARGS__);  \
      return PCC_E_STREAM;         \
    }                              \
  } while (0)

// h_in[0 .. len): the blob, or a prefix of it.  need_all: the decoder's form — the plan's bytes must be present (lod 0:
// the whole blob, today's check); otherwise (pcc_octree_lod_info) the bytes must only reach what the plan is computed
// from, the last needed chunk's length table.  Nothing beyond h_in[len) is read.
static inline int o2_parse(const uint8_t* h_in, int64_t len, int lod, bool need_all, O2Info* o, O2Plan* pl) {
  O2_REQUIRE(h_in && len >= kO2Header && h_in[0] == 'O' && h_in[1] == 2, "octree blob v2: bad header");
  o->depth = h_in[2];
  o->n = (int64_t)o2_u32(h_in + 4);
  for (int a = 0; a < 3; ++a) o->origin[a] = (int32_t)o2_u32(h_in + 8 + 4 * a);
  const int64_t payload = (int64_t)o2_u32(h_in + 20);
  const bool whole = need_all && lod == 0;
  O2_REQUIRE(!whole || kO2Header + payload <= len, "octree blob v2: truncated");
  pl->lod = lod;
  pl->Lc = 0;
  pl->m = pl->n_dec = pl->chunks = pl->lanes = pl->last_off = pl->last_words = 0;
  pl->bytes = kO2Header;
  if (o->n == 0) {
    o->n_nodes = 0;
    if (lod == 0) pl->bytes = kO2Header + payload;
    return PCC_OK;
  }
  const int d = o->depth;
  O2_REQUIRE(d >= 1 && d <= 16 && payload >= 4 * d + 8 + 2 * kO2Ctx + 4, "octree blob v2: depth %d, payload %lld", d,
             (long long)payload);
  O2_REQUIRE(len >= kO2Header + 4 * d + 8 + 2 * kO2Ctx, "octree blob v2: truncated header");
  const uint8_t* q = h_in + kO2Header;
  o->n_nodes = 0;
  for (int L = 0; L < d; ++L, q += 4) {
    o->level_n[L] = (int64_t)o2_u32(q);
    o->n_nodes += o->level_n[L];
    O2_REQUIRE(o->level_n[L] >= 1 && (L == 0 ? o->level_n[0] == 1 : o->level_n[L] <= 8 * o->level_n[L - 1]) && o->level_n[L] <= o->n,
               "octree blob v2: level %d has %lld nodes", L, (long long)o->level_n[L]);
  }
  O2_REQUIRE(o->n <= 8 * o->level_n[d - 1] && o->n >= o->level_n[d - 1] && o->n_nodes < ((int64_t)1 << 28),
             "octree blob v2: %lld points under %lld nodes", (long long)o->n, (long long)o->level_n[d - 1]);
  o->S = (int64_t)o2_u32(q);
  o->nc = (int64_t)o2_u32(q + 4);
  q += 8;
  // S <= kO2SMax, as the encoder writes it: a chunk then codes at most 32768 nodes, so the announced node count is bound
  // by the chunk table's length (every chunk has at least 384 bytes of states and lengths)
  O2_REQUIRE(o->S >= 4 && o->S % 4 == 0 && o->S <= kO2SMax && o->nc >= 1 && kO2Lanes * o->S * o->nc >= o->n_nodes &&
                 kO2Lanes * o->S * (o->nc - 1) < o->n_nodes,
             "octree blob v2: %lld nodes in %lld chunks of 64 x %lld", (long long)o->n_nodes, (long long)o->nc, (long long)o->S);
  o->off_p0 = q - h_in;
  for (int i = 0; i < kO2Ctx; ++i, q += 2) {
    const uint32_t p = (uint32_t)q[0] | ((uint32_t)q[1] << 8);
    O2_REQUIRE(p >= 16 && p <= 4080, "octree blob v2: initial probability %u", p);
  }
  o->off_table = q - h_in;
  O2_REQUIRE(kO2Header + payload - o->off_table >= 4 * o->nc, "octree blob v2: truncated chunk table");
  O2_REQUIRE(len - o->off_table >= 4 * o->nc, "octree blob v2: truncated inside the chunk table");
  int64_t words = 0;
  for (int64_t c = 0; c < o->nc; ++c) {
    const int64_t cw = (int64_t)o2_u32(q + 4 * c);
    O2_REQUIRE(cw >= 3 * kO2Lanes, "octree blob v2: chunk %lld has no states", (long long)c);
    words += cw;
  }
  o->off_payload = o->off_table + 4 * o->nc;
  o->payload_words = words;
  O2_REQUIRE(o->off_payload + 2 * words == kO2Header + payload, "octree blob v2: chunks take %lld bytes, blob has %lld",
             (long long)(2 * words), (long long)(kO2Header + payload - o->off_payload));
  // the plan
  if (lod == 0) {
    const int64_t last = (int64_t)o2_u32(q + 4 * (o->nc - 1));
    pl->Lc = d;
    pl->m = o->n;
    pl->n_dec = o->n_nodes;
    pl->chunks = o->nc;
    pl->lanes = kO2Lanes;
    pl->bytes = kO2Header + payload;
    pl->last_off = words - last;
    pl->last_words = last;
    return PCC_OK;
  }
  pl->Lc = d > lod ? d - lod : 0;
  pl->m = pl->Lc ? o->level_n[pl->Lc] : 1;
  for (int L = 0; L < pl->Lc; ++L) pl->n_dec += o->level_n[L];
  pl->bytes = o->off_payload;
  if (pl->n_dec == 0) return PCC_OK;
  const int64_t lanes = (pl->n_dec + o->S - 1) / o->S, cs = (lanes - 1) / kO2Lanes, ls = (lanes - 1) % kO2Lanes;
  for (int64_t c = 0; c < cs; ++c) pl->last_off += (int64_t)o2_u32(q + 4 * c);
  const int64_t cw = (int64_t)o2_u32(q + 4 * cs);
  const int64_t at = o->off_payload + 2 * pl->last_off;   // the chunk: 128 state words, then its length table
  O2_REQUIRE(len >= at + 2 * 3 * kO2Lanes, "octree blob v2: truncated in front of the length table of chunk %lld", (long long)cs);
  int64_t run = 3 * kO2Lanes;
  for (int64_t l = 0; l <= ls; ++l) run += (int64_t)h_in[at + 4 * kO2Lanes + 2 * l] | ((int64_t)h_in[at + 4 * kO2Lanes + 2 * l + 1] << 8);
  O2_REQUIRE(run <= cw, "octree blob v2: the runs of chunk %lld take %lld words of its %lld", (long long)cs, (long long)run,
             (long long)cw);
  pl->chunks = cs + 1;
  pl->lanes = ls + 1;
  pl->last_words = run;
  pl->bytes = at + 2 * run;
  O2_REQUIRE(!need_all || pl->bytes <= len, "octree blob v2: truncated (level of detail %d needs %lld bytes, %lld are here)", lod,
             (long long)pl->bytes, (long long)len);
  return PCC_OK;
}
