// The attribute blob's header parser (csrc/attr_blob.h) on damaged and cut blobs: error codes, never a read outside
// the blob.  Built with -fsanitize=address,undefined by tests/test_fuzz_attr.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
void pcc_set_error(const char* fmt, ...) {}
#include "attr_blob.h"
int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  uint64_t seed = 777;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  // a well-formed blob: 3 channels of uint8, n = 9000 points, the encoder's layout, chunks of random word counts
  const int bpv = 1, c = 3, nctx = attr_contexts(bpv, c);
  const int64_t n = 9000;
  int64_t S, nc;
  attr_layout(n, c, &S, &nc);
  std::vector<uint8_t> blob(kAttrHead + 8 + 2 * nctx + 4 * nc);
  auto put32 = [&](size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) blob[at + i] = (uint8_t)(v >> (8 * i)); };
  blob[0] = 'A'; blob[1] = 1; blob[2] = bpv; blob[3] = c;
  put32(4, (uint32_t)n);
  put32(kAttrHead, (uint32_t)S);
  put32(kAttrHead + 4, (uint32_t)nc);
  for (int i = 0; i < nctx; ++i) { blob[kAttrHead + 8 + 2 * i] = 0x00; blob[kAttrHead + 9 + 2 * i] = 0x08; }   // 2048
  int64_t words = 0;
  for (int64_t k = 0; k < nc; ++k) {
    const uint32_t cw = 192 + rnd() % 4000;
    put32(kAttrHead + 8 + 2 * nctx + 4 * k, cw);
    words += cw;
  }
  blob.resize(blob.size() + 2 * words, 0x5A);
  put32(8, (uint32_t)(blob.size() - kAttrHead));
  AttrInfo o;
  int rc = attr_parse(blob.data(), (int64_t)blob.size(), &o);
  printf("well-formed: rc %d n %lld S %lld chunks %lld words %lld\n", rc, (long long)o.n, (long long)o.S, (long long)o.nc,
         (long long)o.payload_words);
  if (rc != 0 || o.payload_words != words) return 1;
  int oks = 0, errs = 0;
  for (int it = 0; it < iters; ++it) {
    const int64_t head = kAttrHead + 8 + 2 * nctx + 4 * nc;
    const int64_t cut = (it % 5 == 0) ? (int64_t)(rnd() % blob.size()) : (int64_t)blob.size();
    std::vector<uint8_t> b(blob.begin(), blob.begin() + cut);   // exactly the bytes the parser may read
    const int flips = 1 + (int)(rnd() % 3);
    for (int f = 0; f < flips && !b.empty(); ++f) b[rnd() % std::min<int64_t>(head, (int64_t)b.size())] ^= (uint8_t)(1u << (rnd() & 7));
    AttrInfo q;
    const int r = attr_parse(b.empty() ? nullptr : b.data(), (int64_t)b.size(), &q);
    if (r == 0) {
      ++oks;   // accepted: everything the decoder would size from must lie inside the blob
      if (q.n > 0 && (q.off_payload + 2 * q.payload_words != (int64_t)b.size() || q.S * q.c > kAttrMaxValues ||
                      kAttrLanes * q.S * q.nc < q.n)) return 2;
    } else {
      ++errs;
    }
  }
  printf("fuzz: %d accepted, %d refused\n", oks, errs);
  return errs > 0 ? 0 : 3;
}
