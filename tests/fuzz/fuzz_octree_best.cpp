// The host side of pcc_octree_encode_frames_inter_best (csrc/octree_best_host.h): the windows of a call, the choice
// among a frame's candidates and the copy of the winners out of the staging, on random calls — empty frames, reference
// frames, intra periods, equal lengths, a capacity of zero and one byte short, candidates that leave the staging.
// Every result is compared with a plain restatement; built with -fsanitize=address,undefined by
// tests/test_octree_inter_best.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "octree_best_host.h"

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  uint64_t seed = 9091;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  long long copied = 0, refused = 0, outside = 0;
  for (int it = 0; it < iters; ++it) {
    const int n_frames = 1 + (int)(rnd() % 12), history = 1 + (int)(rnd() % 8);
    const int n_ref = (int)(rnd() % (uint32_t)std::min(history + 1, n_frames));
    const int period = (int)(rnd() % 5);
    std::vector<int64_t> offs((size_t)n_frames + 1, 0);
    for (int f = 0; f < n_frames; ++f) offs[(size_t)f + 1] = offs[(size_t)f] + (rnd() % 4 == 0 ? 0 : 1 + rnd() % 50);
    std::vector<int> wmax;
    o4_best_windows(offs.data(), n_frames, n_ref, period, history, &wmax);
    // the rule, restated frame by frame
    for (int f = 0; f < n_frames; ++f) {
      const bool pts = offs[(size_t)f + 1] > offs[(size_t)f];
      int want = -1;
      if (f >= n_ref && pts) {
        auto sched = [&](int q) { return q >= n_ref && (period > 0 ? (q - n_ref) % period == 0 : q == 0); };
        auto has = [&](int q) { return q >= 0 && offs[(size_t)q + 1] > offs[(size_t)q]; };
        if (sched(f) || !has(f - 1)) want = 0;
        else {
          want = 0;
          for (int q = f - 1; q >= 0 && want < history && has(q); --q) {
            ++want;
            if (sched(q) || !has(q - 1)) break;   // an intra frame is in the window, nothing in front of it
          }
        }
      }
      if (wmax[(size_t)f] != want) { printf("windows: frame %d of %d: %d, want %d\n", f, n_frames, wmax[(size_t)f], want); return 1; }
    }
    // candidates as the two batches leave them: a staging of random bytes, lengths that often tie
    const int64_t stage_bytes = (int64_t)(rnd() % 3000);
    std::vector<uint8_t> stage((size_t)stage_bytes);
    for (auto& b : stage) b = (uint8_t)rnd();
    std::vector<O4BestCand> cands;
    const bool stray = rnd() % 8 == 0;   // a candidate that does not lie inside the staging
    for (int f = 0; f < n_frames; ++f) {
      if (wmax[(size_t)f] < 0) continue;
      for (int W = 0; W <= wmax[(size_t)f]; ++W) {
        O4BestCand c;
        c.frame = f;
        c.window = W;
        c.len = 24 + (int64_t)(rnd() % 6) * 8;
        c.off = stage_bytes > c.len ? (int64_t)(rnd() % (uint32_t)(stage_bytes - c.len + 1)) : 0;
        if (stage_bytes < c.len || (stray && rnd() % 4 == 0)) c.off = stage_bytes - (int64_t)(rnd() % 20);
        cands.push_back(c);
      }
    }
    for (size_t i = cands.size(); i > 1; --i) std::swap(cands[i - 1], cands[rnd() % i]);   // any order
    std::vector<int64_t> choice;
    o4_best_choose(cands.data(), (int64_t)cands.size(), n_frames, &choice);
    int64_t total = 0;
    bool leaves = false;
    for (int f = 0; f < n_frames; ++f) {
      int64_t best = -1;
      for (size_t c = 0; c < cands.size(); ++c)
        if (cands[c].frame == f && (best < 0 || cands[c].len < cands[(size_t)best].len ||
                                    (cands[c].len == cands[(size_t)best].len && cands[c].window < cands[(size_t)best].window)))
          best = (int64_t)c;
      if (choice[(size_t)f] != best) { printf("choice: frame %d\n", f); return 2; }
      if (f < n_ref) continue;
      if (best >= 0 && (cands[(size_t)best].off < 0 || cands[(size_t)best].off + cands[(size_t)best].len > stage_bytes)) leaves = true;
      total += best < 0 ? 24 : cands[(size_t)best].len;
    }
    const int64_t cap = rnd() % 4 == 0 ? 0 : (rnd() % 4 == 0 ? total - 1 : total + (int64_t)(rnd() % 3));
    std::vector<uint8_t> out((size_t)std::max<int64_t>(cap, 0));   // exactly cap bytes: a store behind them is a report
    std::vector<int64_t> h_offs((size_t)n_frames + 1, -7);
    int64_t need = -1;
    const int64_t got = o4_best_copy(stage.data(), stage_bytes, cands.data(), choice.data(), n_frames, n_ref, out.data(),
                                     std::max<int64_t>(cap, 0), h_offs.data(), &need);
    if (leaves) {
      if (got != -2) { printf("copy: a candidate outside the staging gave %lld\n", (long long)got); return 3; }
      ++outside;
      continue;
    }
    if (total > std::max<int64_t>(cap, 0)) {
      if (got != -1 || need != total) { printf("copy: %lld bytes into %lld gave %lld\n", (long long)total, (long long)cap, (long long)got); return 4; }
      ++refused;
      continue;
    }
    if (got != total || h_offs[0] != 0 || h_offs[(size_t)n_frames] != total) { printf("copy: total\n"); return 5; }
    for (int f = 0; f < n_frames; ++f) {
      const int64_t len = h_offs[(size_t)f + 1] - h_offs[(size_t)f];
      const uint8_t* b = out.data() + h_offs[(size_t)f];
      if (f < n_ref) { if (len != 0) return 6; continue; }
      if (choice[(size_t)f] < 0) {
        if (len != 24 || b[0] != 'O' || b[1] != 2 || std::count(b + 2, b + 24, 0) != 22) return 7;
        continue;
      }
      const O4BestCand& c = cands[(size_t)choice[(size_t)f]];
      std::vector<uint8_t> want(stage.begin() + c.off, stage.begin() + c.off + c.len);
      if (c.window >= 1) want[3] = (uint8_t)(c.window - 1);
      if (len != c.len || memcmp(b, want.data(), (size_t)len) != 0) { printf("copy: frame %d\n", f); return 8; }
    }
    ++copied;
  }
  printf("fuzz: %d calls: %lld copied, %lld refused for capacity, %lld with a candidate outside the staging\n", iters, copied, refused, outside);
  return copied > 0 && refused > 0 && outside > 0 ? 0 : 9;
}
