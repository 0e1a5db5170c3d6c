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
// has points (a frame without points is the 24-byte version-2 blob) and is read whole (lod 0).  The checks are version
// 2's: every level at most 8 times the one above and at most n, the chunk count what S and the node count make it, the
// chunk table's sum the payload's length — every size the decoder reserves or launches from is bounded by the blob's
// length.
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

// h_in[0 .. len): the whole blob.  Nothing beyond h_in[len) is read.
static inline int o4_parse(const uint8_t* h_in, int64_t len, O4Info* o) {
  O4_REQUIRE(h_in && len >= kO4Header && h_in[0] == 'O' && h_in[1] == 4, "octree blob v4: bad header");
  o->depth = h_in[2];
  o->window = (int)h_in[3] + 1;
  o->n = (int64_t)o4_u32(h_in + 4);
  for (int a = 0; a < 3; ++a) o->origin[a] = (int32_t)o4_u32(h_in + 8 + 4 * a);
  const int64_t payload = (int64_t)o4_u32(h_in + 20);
  O4_REQUIRE(kO4Header + payload == len, "octree blob v4: %lld bytes announced, %lld are here", (long long)(kO4Header + payload),
             (long long)len);
  const int d = o->depth;
  O4_REQUIRE(o->n >= 1, "octree blob v4: no points (a frame without points is a version-2 blob)");
  O4_REQUIRE(d >= 1 && d <= 16 && payload >= 4 * d + 8 + 12 + 2 * kO4Ctx + 4, "octree blob v4: depth %d, payload %lld", d,
             (long long)payload);
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
  O4_REQUIRE(o->off_payload + 2 * words == len, "octree blob v4: chunks take %lld bytes, blob has %lld", (long long)(2 * words),
             (long long)(len - o->off_payload));
  return PCC_OK;
}
