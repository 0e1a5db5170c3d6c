// attr_nbr.h — the kernels of attribute blob versions 25, 26, 28 and 31 (attr_blob.h states the rules).  25 / 26: lossless
// values in version 2's introduction order, each predicted from up to three Morton-first points of the coarser cells
// around it; 28 / 31, at the end of this comment, their bounded-error forms.
// Included by attr.hip behind its own kernels, whose frame rows (AFrame, ADFrame, A2Order), order stage (k_a2_size,
// k_a2_scan) and value accessors (a_load, a_store) it uses; nothing in here is launched for another kind.
//
// Encoder: k_an_place behind k_a2_size / k_a2_scan, in the shape of k_a2_place<true>: one thread per point, up to 27
// bounded lower bounds over the frame's keys, the three best kept in three registers, the residual stored to its place.
// Every merged value is known, so there is no order among the points.
// Decoder: k_an_plan behind the same order stage (the Morton index of every place, and every point's choice, 3 words),
// k_a_dec<true> (and k_ax_inv), then k_an_recon once per size of introduction 16 .. 0 that holds a point in any frame of
// the call, over that size's range of the introduction order: a point's candidates are all of larger sizes, so every
// value it reads was written by an earlier launch.  Every wait is a kernel boundary.
//
// Versions 28 and 31, their bounded-error forms (a closed loop: the predictor runs over decoded values).  Encoder:
// k_anl_plan behind the order stage keeps every point's choice as k_an_plan does, then k_anl_quant once per size of
// introduction, 16 down to 0, quantises that size against the reconstructions of the larger sizes and writes its own.
// Decoder: the launches of 25 / 26 with k_anl_recon, k_an_recon's body with the index scaled and the sum clamped.
#pragma once

namespace {

constexpr uint32_t kANone = 0xFFFFFFFFu;   // a slot without a candidate
constexpr int kANIndexBits = 27;           // a choice: Morton index (a frame has fewer than 2^27 points) | d << 27, d in 1 .. 27

// The choice of point i > 0 of size s among the frame's n sorted keys.  ksh: the bits of a key below its cell (the
// encoder's key_shift; 0 for the decoder's cell keys); lbits: the lattice's bits per axis, 16 - the level of the cells.
// pick[0 .. 3): the up to three candidates with the smallest (d, Morton index), kANone behind them.  Every index is the
// result of a search in [0, n) that was checked against the cell it was meant to find, so it is below n.
__device__ __forceinline__ void an_choose(const uint64_t* __restrict__ keys, int64_t n, int64_t i, int s, int ksh, int lbits,
                                          uint32_t (&pick)[3]) {
  constexpr uint64_t kLow48 = 0xFFFFFFFFFFFFull;
  const uint64_t own = keys[i], top = own & ~kLow48, key = (own & kLow48) >> ksh;
  const int sb = std::min(3 * (s + 1) + ksh, 48);   // the bits of a key below a candidate cell
  const int ux = (int)(pcc_compact3(key >> 2) >> s), uy = (int)(pcc_compact3(key >> 1) >> s), uz = (int)(pcc_compact3(key) >> s);
  const int cx = ux >> 1, cy = uy >> 1, cz = uz >> 1;
  const int lim = s + 1 >= lbits ? 1 : 1 << (lbits - s - 1);   // candidate cells per axis of the lattice
  uint64_t r0 = ~0ull, r1 = ~0ull, r2 = ~0ull;                 // d << 32 | Morton index, ascending
#pragma unroll 1
  for (int t = 0; t < 27; ++t) {
    const int qx = cx + t / 9 - 1, qy = cy + (t / 3) % 3 - 1, qz = cz + t % 3 - 1;
    if (qx < 0 || qy < 0 || qz < 0 || qx >= lim || qy >= lim || qz >= lim) continue;
    const uint64_t ck = (pcc_spread3((uint32_t)qx) << 2) | (pcc_spread3((uint32_t)qy) << 1) | pcc_spread3((uint32_t)qz);
    const uint64_t target = top | (sb >= 48 ? 0ull : ck << sb);
    int64_t lo = 0, hi = t == 13 ? i : n;   // o = 0: first(i), which lies in front of i
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    if (lo >= n || lo == i) continue;
    const uint64_t kj = keys[lo];
    if ((kj >> sb) != (target >> sb)) continue;   // the cell is empty
    const uint64_t cj = (kj & kLow48) >> ksh;
    const int dx = (int)(pcc_compact3(cj >> 2) >> s) - ux, dy = (int)(pcc_compact3(cj >> 1) >> s) - uy,
              dz = (int)(pcc_compact3(cj) >> s) - uz;
    const uint32_t d = (uint32_t)(dx * dx + dy * dy + dz * dz);
    if (d == 0 || d > 27) continue;   // cannot happen: i and lo are the first points of different cells of side 2^s
    const uint64_t r = ((uint64_t)d << 32) | (uint64_t)lo;
    if (r < r2) {
      r2 = r;
      if (r2 < r1) { const uint64_t x = r1; r1 = r2; r2 = x; }
      if (r1 < r0) { const uint64_t x = r0; r0 = r1; r1 = x; }
    }
  }
  const auto slot = [](uint64_t r) { return r == ~0ull ? kANone : (uint32_t)r | ((uint32_t)(r >> 32) << kANIndexBits); };
  pick[0] = slot(r0);
  pick[1] = slot(r1);
  pick[2] = slot(r2);
}

// p[ch] = floor((2 sum(w v_j) + sum(w)) / (2 sum(w))) over the slots of a choice, w = floor(65536 / d), in 64 bits; 0
// without a candidate (point 0).  load(j, ch): value ch of Morton index j
template <typename Load>
__device__ __forceinline__ void an_predict(const uint32_t (&pick)[3], int c, Load load, uint32_t (&p)[4]) {
  uint64_t num[4] = {0, 0, 0, 0};
  uint64_t sw = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (pick[k] == kANone) continue;
    const uint32_t d = pick[k] >> kANIndexBits, j = pick[k] & ((1u << kANIndexBits) - 1u);
    const uint64_t w = 65536u / (d ? d : 1u);
    sw += w;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < c) num[ch] += w * (uint64_t)load(j, ch);
  }
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) p[ch] = sw && ch < c ? (uint32_t)((2 * num[ch] + sw) / (2 * sw)) : 0u;
}

// Encoder: the place of every point in the introduction order (as k_a2_place finds it) and the residual of its merged
// value against the predictor of its choice, to that place of resid ([n][c] per frame at val_off, wrapped to the value
// width).  Frame f owns blocks [blk0, blk0 + ceil(n / 256))
__global__ __launch_bounds__(256) void k_an_place(const uint64_t* __restrict__ keys_all, const A2Order* __restrict__ tab, int nf,
                                                  const uint16_t* __restrict__ packed, const uint32_t* __restrict__ hist,
                                                  const uint32_t* __restrict__ bins, const AFrame* __restrict__ ftab,
                                                  const uint16_t* __restrict__ merged, uint16_t* __restrict__ resid) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const uint32_t pk = packed[h.pt0 + i];
  const int s = (int)(pk >> 8);
  const int64_t r = (int64_t)bins[f * kA2Bins + s] + hist[(int64_t)blockIdx.x * kA2Bins + s] + (pk & 255u);
  if (r >= h.n) return;   // cannot happen: the places are a permutation of the frame's points
  const AFrame& a = ftab[f];
  const int c = a.c;
  const uint32_t mask = (1u << (8 * a.bpv)) - 1u;
  const uint16_t* v = merged + a.val_off;
  uint32_t pick[3] = {kANone, kANone, kANone}, p[4];
  if (i > 0) an_choose(keys_all + h.pt0, h.n, i, s, h.shift, 16 - h.shift / 3, pick);
  an_predict(pick, c, [&](uint32_t j, int ch) { return (uint32_t)v[(int64_t)j * c + ch]; }, p);
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
    if (ch < c) resid[a.val_off + r * c + ch] = (uint16_t)(((uint32_t)v[i * c + ch] - p[ch]) & mask);
}

// Decoder, over the keys of the cells: inv[pt0 + r] = the Morton index of place r of the introduction order, and the
// choice of every cell, picks[3 (pt0 + i) + k].  Nothing of it depends on the attribute stream
__global__ __launch_bounds__(256) void k_an_plan(const uint64_t* __restrict__ keys_all, const A2Order* __restrict__ tab, int nf,
                                                 const uint16_t* __restrict__ packed, const uint32_t* __restrict__ hist,
                                                 const uint32_t* __restrict__ bins, uint32_t* __restrict__ inv,
                                                 uint32_t* __restrict__ picks) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const uint32_t pk = packed[h.pt0 + i];
  const int s = (int)(pk >> 8);
  const int64_t r = (int64_t)bins[f * kA2Bins + s] + hist[(int64_t)blockIdx.x * kA2Bins + s] + (pk & 255u);
  if (r < h.n) inv[h.pt0 + r] = (uint32_t)i;
  uint32_t pick[3] = {kANone, kANone, kANone};
  if (i > 0) an_choose(keys_all + h.pt0, h.n, i, s, 0, 16 - h.shift, pick);
  uint32_t* o = picks + 3 * (h.pt0 + i);
  o[0] = pick[0];
  o[1] = pick[1];
  o[2] = pick[2];
}

// Decoder, size s of the introduction order: frame = blockIdx.y, one thread per place of the frame's range [bins[17 f +
// s], bins[17 f + s - 1]) (size 0: up to its m values), both from the order stage on the device, whatever count the
// host sized the grid from.  value = (predictor of the kept choice over the values written so far + residual) & mask,
// to the cell's row of out.  resid_all / out_all: the frames' [m][c] values of bpv bytes at out_off, residuals in
// introduction order / values in Morton order.  status |= 8 where an index is outside the frame
//
// NL (versions 28 / 31): resid_all holds the indices j, sign-extended from the value width; the predictor runs over the
// clamped values written so far, value = clip(p + j q, 0, mask) with the sum in 64 bits (|j| <= 2^15 and q < 2^16: a
// damaged stream reaches 2^31), clamped as k_a2_walk<true> clamps; status |= 16 where the sum lies outside [-e, mask + e],
// which no encoder's reconstruction does
template <bool NL>
__device__ __forceinline__ void an_recon(const A2Order* __restrict__ tab, const ADFrame* __restrict__ ftab,
                                         const uint32_t* __restrict__ bins, int s, const uint32_t* __restrict__ inv,
                                         const uint32_t* __restrict__ picks, const uint8_t* __restrict__ resid_all,
                                         uint8_t* __restrict__ out_all, int32_t* __restrict__ status_all) {
  const int f = blockIdx.y;
  const A2Order& h = tab[f];
  const ADFrame& a = ftab[f];
  const int64_t start = bins[f * kA2Bins + s], end = std::min<int64_t>(s > 0 ? (int64_t)bins[f * kA2Bins + s - 1] : h.n, h.n);
  const int64_t r = start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= end) return;
  const uint32_t i = inv[h.pt0 + r];
  if (i >= h.n) {
    atomicOr(status_all + f, 8);
    return;
  }
  const int c = a.c, bpv = a.bpv;
  const uint32_t mask = (1u << (8 * bpv)) - 1u;
  uint32_t pick[3], p[4];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pick[k] = picks[3 * (h.pt0 + i) + k];
    if (pick[k] != kANone && (int64_t)(pick[k] & ((1u << kANIndexBits) - 1u)) >= h.n) {
      bad = true;
      pick[k] = kANone;
    }
  }
  if (bad) atomicOr(status_all + f, 8);
  uint8_t* out = out_all + a.out_off;
  an_predict(pick, c, [&](uint32_t j, int ch) { return a_load(out + (int64_t)j * c * bpv, bpv, ch); }, p);
  const uint8_t* x = resid_all + a.out_off + r * c * bpv;
  uint8_t* o = out + (int64_t)i * c * bpv;
  if constexpr (!NL) {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < c) a_store(o, bpv, (p[ch] + a_load(x, bpv, ch)) & mask, ch);
  } else {
    const int64_t e = a.max_error, q = 2 * e + 1;
    bool far = false;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < c) {
        const int64_t y = (int64_t)p[ch] + (int64_t)a_load_s(x, bpv, ch) * q;
        far |= y < -e || y > (int64_t)mask + e;
        a_store(o, bpv, (uint32_t)(y < 0 ? 0 : (y > (int64_t)mask ? (int64_t)mask : y)), ch);
      }
    if (far) atomicOr(status_all + f, 16);
  }
}

__global__ __launch_bounds__(256) void k_an_recon(const A2Order* __restrict__ tab, const ADFrame* __restrict__ ftab,
                                                  const uint32_t* __restrict__ bins, int s, const uint32_t* __restrict__ inv,
                                                  const uint32_t* __restrict__ picks, const uint8_t* __restrict__ resid_all,
                                                  uint8_t* __restrict__ out_all, int32_t* __restrict__ status_all) {
  an_recon<false>(tab, ftab, bins, s, inv, picks, resid_all, out_all, status_all);
}
__global__ __launch_bounds__(256) void k_anl_recon(const A2Order* __restrict__ tab, const ADFrame* __restrict__ ftab,
                                                   const uint32_t* __restrict__ bins, int s, const uint32_t* __restrict__ inv,
                                                   const uint32_t* __restrict__ picks, const uint8_t* __restrict__ resid_all,
                                                   uint8_t* __restrict__ out_all, int32_t* __restrict__ status_all) {
  an_recon<true>(tab, ftab, bins, s, inv, picks, resid_all, out_all, status_all);
}

// ---- versions 28 and 31: the encoder's closed loop ------------------------------------------------------------------
// Encoder, over the call's keys, behind the order stage: k_an_plan's two arrays from the encoder's keys (ksh = key_shift).
// The 27 searches of every point run here, once, at full occupancy; the launches below only gather
__global__ __launch_bounds__(256) void k_anl_plan(const uint64_t* __restrict__ keys_all, const A2Order* __restrict__ tab, int nf,
                                                  const uint16_t* __restrict__ packed, const uint32_t* __restrict__ hist,
                                                  const uint32_t* __restrict__ bins, uint32_t* __restrict__ inv,
                                                  uint32_t* __restrict__ picks) {
  const int f = o2_find(nf, blockIdx.x, [&](int i) { return (int64_t)tab[i].blk0; });
  const A2Order& h = tab[f];
  const int64_t i = ((int64_t)blockIdx.x - h.blk0) * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const uint32_t pk = packed[h.pt0 + i];
  const int s = (int)(pk >> 8);
  const int64_t r = (int64_t)bins[f * kA2Bins + s] + hist[(int64_t)blockIdx.x * kA2Bins + s] + (pk & 255u);
  if (r < h.n) inv[h.pt0 + r] = (uint32_t)i;
  uint32_t pick[3] = {kANone, kANone, kANone};
  if (i > 0) an_choose(keys_all + h.pt0, h.n, i, s, h.shift, 16 - h.shift / 3, pick);
  uint32_t* o = picks + 3 * (h.pt0 + i);
  o[0] = pick[0];
  o[1] = pick[1];
  o[2] = pick[2];
}

// Encoder, size s of the introduction order, in k_an_recon's shape: frame = blockIdx.y, one thread per place of the
// frame's range of the order stage.  The point's predictor over the reconstructions of its kept choice (all of larger
// sizes: written by earlier launches), its index j = a_quant(v - p) to its place of idx, wrapped to the value width, and
// its own reconstruction clip(p + j q, 0, mask) to its Morton index of recon.  merged / recon / idx: uint16 [n][c] per
// frame at val_off; recon in Morton order, idx in introduction order.  |p + j q| < 2^18: int holds it
__global__ __launch_bounds__(256) void k_anl_quant(const A2Order* __restrict__ tab, const AFrame* __restrict__ ftab,
                                                   const uint32_t* __restrict__ bins, int s, const uint32_t* __restrict__ inv,
                                                   const uint32_t* __restrict__ picks, const uint16_t* __restrict__ merged,
                                                   uint16_t* __restrict__ recon, uint16_t* __restrict__ idx) {
  const int f = blockIdx.y;
  const A2Order& h = tab[f];
  const AFrame& a = ftab[f];
  const int64_t start = bins[f * kA2Bins + s], end = std::min<int64_t>(s > 0 ? (int64_t)bins[f * kA2Bins + s - 1] : h.n, h.n);
  const int64_t r = start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= end) return;
  const uint32_t i = inv[h.pt0 + r];
  if (i >= h.n) return;   // cannot happen: the places are a permutation of the frame's points
  const int c = a.c, e = a.e, q = 2 * e + 1;
  const int mask = (1 << (8 * a.bpv)) - 1;
  uint32_t pick[3], p[4];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pick[k] = picks[3 * (h.pt0 + i) + k];
    if (pick[k] != kANone && (int64_t)(pick[k] & ((1u << kANIndexBits) - 1u)) >= h.n) pick[k] = kANone;   // cannot happen (an_choose)
  }
  uint16_t* vh = recon + a.val_off;
  an_predict(pick, c, [&](uint32_t j, int ch) { return (uint32_t)vh[(int64_t)j * c + ch]; }, p);
  const uint16_t* v = merged + a.val_off + (int64_t)i * c;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
    if (ch < c) {
      const int j = a_quant((int)v[ch] - (int)p[ch], e, q);
      const int y = (int)p[ch] + j * q;
      idx[a.val_off + r * c + ch] = (uint16_t)((uint32_t)j & (uint32_t)mask);
      vh[(int64_t)i * c + ch] = (uint16_t)(y < 0 ? 0 : (y > mask ? mask : y));
    }
}

}  // namespace
