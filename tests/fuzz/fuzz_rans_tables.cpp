// the decoder's z job (codec.hip): pcc_rans_decode8_gated with coder tables built once (pcc_rans_tables_build), byte
// indexes and no chunk gate, on intact, damaged and cut streams
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pcc.h"
void pcc_set_error(const char* fmt, ...) {}
#include "rans_host.cpp"
int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  uint64_t seed = 7; auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  const int pitch = 20; int32_t cdfs[2 * pitch] = {0}; int32_t sizes[2] = {12, 7}, offs[2] = {-5, -2};
  { int32_t c = 0; for (int i = 0; i < 12; ++i) { cdfs[i] = c; c += (i == 11) ? 0 : (i == 5 ? 40000 : 2321); } cdfs[11] = 65536; }
  { int32_t v[7] = {0, 100, 5000, 60000, 65000, 65500, 65536}; for (int i = 0; i < 7; ++i) cdfs[pitch + i] = v[i]; }
  const int64_t n = 4000;
  std::vector<int32_t> sym(n), idx(n);
  std::vector<uint8_t> idx8(n);
  for (int64_t i = 0; i < n; ++i) { idx[i] = idx8[i] = (uint8_t)(i >= n / 2); int32_t s = (int32_t)(rnd() % 9) - 4; if (rnd() % 300 == 0) s = (int32_t)(rnd() % 100000) - 50000; sym[i] = s; }
  std::vector<uint8_t> out(n * 8 + 64); int64_t len = 0;
  int rc = pcc_rans_encode(sym.data(), idx.data(), n, cdfs, pitch, sizes, offs, 2, out.data(), (int64_t)out.size(), &len);
  printf("enc rc %d len %lld\n", rc, (long long)len);
  PccRansTables* t = pcc_rans_tables_build(cdfs, pitch, sizes, offs, 2);
  if (!t) { printf("no tables\n"); return 1; }
  std::vector<int32_t> dec(n, -1), gen(n, -1);
  rc = pcc_rans_decode8_gated(out.data(), len, idx8.data(), n, cdfs, pitch, sizes, offs, 2, dec.data(), nullptr, t);
  const int rc2 = pcc_rans_decode(out.data(), len, idx.data(), n, cdfs, pitch, sizes, offs, 2, gen.data());
  printf("cached tables equal generic: %d\n", (int)(rc == 0 && rc2 == 0 && dec == sym && gen == sym));
  int errs = 0, oks = 0, diff = 0;
  for (int it = 0; it < iters; ++it) {
    std::vector<uint8_t> b(out.begin(), out.begin() + len);
    b[rnd() % len] ^= (uint8_t)(1u << (rnd() & 7));
    if (it % 3 == 0) b[rnd() % len] = (uint8_t)rnd();
    const int64_t cut = (it % 7 == 0) ? (int64_t)(rnd() % len) : len;
    std::vector<int32_t> d1(n, -1), d2(n, -1);
    const int r1 = pcc_rans_decode8_gated(b.data(), cut, idx8.data(), n, cdfs, pitch, sizes, offs, 2, d1.data(), nullptr, t);
    const int r2 = pcc_rans_decode(b.data(), cut, idx.data(), n, cdfs, pitch, sizes, offs, 2, d2.data());
    if (r1 != r2 || (r1 == 0 && d1 != d2)) ++diff;
    if (r1 == 0) ++oks; else ++errs;
  }
  pcc_rans_tables_free(t);
  printf("fuzz: %d ok, %d errors, %d differ from the generic decoder\n", oks, errs, diff);
  return diff ? 1 : 0;
}
