// attr_blob.h — the header of an attribute blob (attr.hip), parsed and checked on the host before anything is reserved
// or launched.  Plain C++ (no HIP): tests/fuzz/fuzz_attr_header.cpp puts it under the sanitizers.
//
// Every size the decoder reserves or reads follows from what this parse accepted: the chunk table must add up to the
// blob's own length, so a header cannot announce more words than the blob holds; n is bounded by the chunks
// (64 S nc >= n > 64 S (nc - 1)) and the chunks by the table.
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
