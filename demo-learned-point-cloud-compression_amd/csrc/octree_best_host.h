// octree_best_host.h — the host side of pcc_octree_encode_frames_inter_best (octree2.hip; include/pcc.h has the rule):
// which window every frame of the call may try, which of a frame's candidates is written, and the copy of the winners
// from the staging into the caller's buffer.  No HIP and no library state: tests/fuzz/fuzz_octree_best.cpp builds it
// alone under the sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

constexpr int kO4BestEmptyBlob = 24;   // a frame without points: 'O' 2 and zeros (version 2's header)

// One candidate blob of a frame, as an encode batch left it in the staging: window 0 = version 2, W >= 1 = version 4
// against the union of the W frames in front of the frame.
struct O4BestCand {
  int32_t frame;     // of the call's keys (the reference frames included)
  int32_t window;
  int64_t off, len;  // in the staging
};

// The windows of a call.  offs[f] .. offs[f + 1] are frame f's keys (n_frames + 1 entries, not decreasing); the first
// n_ref_frames frames are references and get no blob.  wmax[f] = -1: no points (or a reference frame): no candidate;
// 0: a scheduled intra frame — coded frame g with g % intra_period == 0 (intra_period 0: frame 0 of the keys alone) —
// or a frame behind one without points: version 2 alone; W >= 1: version 2 and the windows 1 .. W, where W is what
// history = K gives the frame: up to K frames directly in front, not past a scheduled intra frame (which may be in
// it), not past a frame without points.  A version-2 blob written by choice cuts nothing.
inline void o4_best_windows(const int64_t* offs, int n_frames, int n_ref_frames, int intra_period, int history, std::vector<int>* wmax) {
  wmax->assign((size_t)(n_frames > 0 ? n_frames : 0), -1);
  std::vector<char> cut((size_t)(n_frames > 0 ? n_frames : 0), 0);   // frames no window reaches past
  for (int f = n_ref_frames > 0 ? n_ref_frames : 0; f < n_frames; ++f) {
    if (offs[f + 1] <= offs[f]) continue;
    const int g = f - n_ref_frames;
    const bool intra = intra_period > 0 ? g % intra_period == 0 : f == 0;
    const bool ref_points = f > 0 && offs[f] > offs[f - 1];
    if (intra || !ref_points) {
      (*wmax)[(size_t)f] = 0;
      cut[(size_t)f] = 1;
      continue;
    }
    int W = 1;
    while (W < history && !cut[(size_t)(f - W)] && f - W - 1 >= 0 && offs[f - W] > offs[f - W - 1]) ++W;
    (*wmax)[(size_t)f] = W;
  }
}

// choice[f] = the candidate frame f is written as (-1: none of the candidates is its own): the shortest; of equal
// lengths version 2, then the smaller window.  A candidate of a frame outside [0, n_frames) or of a negative length is
// nobody's.
inline void o4_best_choose(const O4BestCand* cands, int64_t n_cands, int n_frames, std::vector<int64_t>* choice) {
  choice->assign((size_t)(n_frames > 0 ? n_frames : 0), -1);
  for (int64_t c = 0; c < n_cands; ++c) {
    const O4BestCand& k = cands[c];
    if (k.frame < 0 || k.frame >= n_frames || k.len < 0 || k.window < 0) continue;
    int64_t& best = (*choice)[(size_t)k.frame];
    if (best < 0 || k.len < cands[best].len || (k.len == cands[best].len && k.window < cands[best].window)) best = c;
  }
}

// The blobs of the call into h_out[0, cap): frame f's at h_offsets[f] .. h_offsets[f + 1] — nothing for the first
// n_ref_frames frames, the chosen candidate's bytes (byte 3 = window - 1 for a version-4 blob), the 24-byte empty blob
// for a frame without a choice.  Returns the bytes written, -1 where they exceed cap (nothing is written then; *need
// receives them), -2 where a chosen candidate does not lie inside the staging or is shorter than a blob's head.
inline int64_t o4_best_copy(const uint8_t* stage, int64_t stage_bytes, const O4BestCand* cands, const int64_t* choice, int n_frames,
                            int n_ref_frames, uint8_t* h_out, int64_t cap, int64_t* h_offsets, int64_t* need) {
  int64_t total = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (f < n_ref_frames) continue;
    if (choice[f] < 0) {
      total += kO4BestEmptyBlob;
      continue;
    }
    const O4BestCand& k = cands[choice[f]];
    if (k.len < kO4BestEmptyBlob || k.off < 0 || k.off > stage_bytes || k.len > stage_bytes - k.off) return -2;
    total += k.len;
  }
  if (need) *need = total;
  if (total > cap) return -1;
  h_offsets[0] = 0;
  for (int f = 0; f < n_frames; ++f) {
    int64_t len = 0;
    if (f >= n_ref_frames) {
      uint8_t* dst = h_out + h_offsets[f];
      if (choice[f] < 0) {
        len = kO4BestEmptyBlob;
        memset(dst, 0, (size_t)len);
        dst[0] = 'O';
        dst[1] = 2;
      } else {
        const O4BestCand& k = cands[choice[f]];
        len = k.len;
        memcpy(dst, stage + k.off, (size_t)len);
        if (k.window >= 1) dst[3] = (uint8_t)(k.window - 1);
      }
    }
    h_offsets[f + 1] = h_offsets[f] + len;
  }
  return total;
}
