// octree4.hip — octree blob version 4: a frame of a sequence coded against the frame before it (a P-frame).
//
// The rule is version 2's (octree2.hip) with the context of every decision split in three by the node's REFERENCE BYTE:
// bit j of it says whether the reference — a set of distinct lattice points, for a sequence the decoded frame before —
// has a point inside the cube of the node's child octant j (include/pcc.h has the rule in full, octree4_blob.h the
// header).  About a fifth of a LiDAR sweep's geometry bytes go (DESIGN.md 6c-inter has the measurements).
//
// Encoder: the coder's three launches are octree2.hip's, instantiated with the reference byte (k_o2_stats / k_o2_enc /
// k_o2_pack <true>); this file adds the step in front of them, o4_ref_bytes_async — every node's cell from the child
// counts (one scan, one pass that links every child to its parent, a walk up the links), then one bounded binary
// search per child cube over the reference's sorted keys: a cube of the lattice is a contiguous range of Morton keys.
//
// Decoder: a context that depends on where a node lies cannot be formed before the levels above the node are decoded,
// so version 2's one launch over all nodes is not available.  A predicted frame is decoded level by level, every wait a
// kernel boundary, the launch sizes from the header's level table (no host synchronisation per level).  Per level L:
//   scan of the child counts of level L - 1 and k_o4_link   the (parent, octant) link of every node of level L
//   k_o4_ref                                                their cells (a walk up L links) and reference bytes
//   k_o4_dec                                                the entropy decode of the level's nodes: the chunks that
//                                                           hold nodes of the level, one wave each
// A lane whose run of S nodes straddles the boundary between two levels leaves its rANS state, its word position and
// its model in global memory and picks them up in the next launch (at most one lane per boundary; two slots used in
// turn, because the lane that picks up and the lane that leaves may differ).  Behind the last level one more scan and
// link give the leaves, and k_o4_points walks every leaf up to the root, as version 2 does.  The chain I P P .. decodes
// frame after frame on the stream: the keys of a decoded frame are the reference of the next.
//
// A window of several frames (history > 1; byte 3 of the head holds the frames of the window - 1): the reference is the
// union of the window's frames, formed on the device by a merge of their sorted distinct keys (k_o4_merge_flag, one
// scan, k_o4_merge_scatter; pcc_merge_keys) — for all predicted frames of an encode call in one go, and frame after
// frame in a decode call, which keeps the keys of the last frames it decoded.  Everything behind the merge sees a
// reference of more keys and nothing else.  pcc_octree_encode_frames_inter_best codes a frame against EVERY window
// 1 .. Wmax and keeps the shortest blob: its unions are nested, and one pass forms them all (k_o4_nest_scatter behind
// the merge's flags and scan; pcc_merge_keys_nested).
//
// A level of detail (lod = k > 0; octree4_blob.h has the plan): a prefix of the blob holds the levels above the cut
// Lc = max(depth - k, 0), and a node above the cut has child cubes of side >= 2^k, unions of whole lod-k cells, so its
// reference byte needs only the reference's CELLS at lod k.  pcc_octree_decode_frames_refs_lod keeps the keys of the
// cells' corners (k_o4_keys with a shift), decodes levels 0 .. Lc - 1 with arrays sized from N' and m, and k_o4_cells
// writes the m cells; the last lane of level Lc - 1 may stop in the middle of its run.  ref_n and ref_sum describe
// full-resolution points and are not compared at a cut.  The lod-0 entries queue what they queued before.
//
// What the stream announces is never trusted: every size comes from the header's checks (octree4_blob.h), every
// store is to an index below a bound the host sized the array from, every read of the stream is clamped to the chunk
// and to the words of it that are present (a prefix ends inside its last needed chunk).
#include "common.h"
#include "lanerans.h"
#include "octree2_blob.h"
#include "octree4.h"
#include "octree4_blob.h"

#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr int kC4 = kO4Ctx;
constexpr uint32_t kL = 1u << 16;
constexpr uint64_t kMask48 = ((uint64_t)1 << 48) - 1;
// the decoder's window of 16-bit words in LDS: 20 KB beside the 41.6 KB of models (325 rows x 64 lanes x 2 B).  It
// holds the runs of the lanes that decode in the launch; a span that does not fit is read from the stream in place
constexpr int kO4Win = 10240;

// the levels of one frame's tree and where its cubes lie
struct O4Tree {
  int64_t off[18];        // level L = nodes [off[L], off[L + 1]); off[depth] = nodes, off[depth + 1] = nodes + leaves
  int32_t depth;
  int32_t origin[3];      // of the root cube, in the units of the frame's points
  int32_t bias;           // reference key = Morton key of (point + bias) per axis
  int32_t key_shift;      // of the reference keys as they are stored
};

// the term of a point in ref_sum
__device__ __forceinline__ unsigned long long o4_sum_term(int x, int y, int z) {
  return ((unsigned long long)((uint32_t)x & 0xFFFFu) << 32) | ((unsigned long long)((uint32_t)y & 0xFFFFu) << 16) |
         (unsigned long long)((uint32_t)z & 0xFFFFu);
}
__device__ __forceinline__ void o4_sum_add(unsigned long long term, unsigned long long* sum) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) term += __shfl_xor(term, d, 64);
  if ((threadIdx.x & 63) == 0 && term) atomicAdd(sum, term);
}

// ref_sum of the reference keys[0 .. n) of an encode call (coordinates as a decoder returns them: the key's cell under
// the key shift, minus its bias)
__global__ __launch_bounds__(256) void k_o4_keysum(const uint64_t* __restrict__ keys, int64_t n, int shift, int bias,
                                                   unsigned long long* __restrict__ sum) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long term = 0;
  if (i < n) {
    const uint64_t k = (keys[i] & kMask48) >> shift;
    term = o4_sum_term((int)pcc_compact3(k >> 2) - bias, (int)pcc_compact3(k >> 1) - bias, (int)pcc_compact3(k) - bias);
  }
  o4_sum_add(term, sum);
}

// the keys (bias 32768) and ref_sum of decoded points, which must be distinct and in Morton order: status |= 32.  At a
// level of detail (lod > 0) the rows are cells, each in [-(32768 >> lod), (32768 >> lod) - 1], and a cell's key is that
// of its corner, the point cell << lod (the sum is then of the cells, and nobody reads it)
__global__ __launch_bounds__(256) void k_o4_keys(const int32_t* __restrict__ pts, int64_t n, int lod, uint64_t* __restrict__ keys,
                                                 unsigned long long* __restrict__ sum, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long term = 0;
  if (i < n) {
    const int x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    const int lim = 32768 >> lod;
    bool bad = x < -lim || x >= lim || y < -lim || y >= lim || z < -lim || z >= lim;
    // (a row out of range gives some key; the call is refused with status 32 whatever was decoded against it)
    auto key_of = [lod](int cx, int cy, int cz) {   // (shifts of the bit patterns: a row may hold anything)
      return pcc_morton(0, (int)((uint32_t)cx << lod), (int)((uint32_t)cy << lod), (int)((uint32_t)cz << lod));
    };
    const uint64_t k = key_of(x, y, z);
    if (i > 0) bad = bad || key_of(pts[3 * i - 3], pts[3 * i - 2], pts[3 * i - 1]) >= k;
    if (bad) atomicOr(status, 32);
    keys[i] = k;
    term = o4_sum_term(x, y, z);
  }
  o4_sum_add(term, sum);
}

// status |= 16 where the reference at hand is not the one the blob was coded against
__global__ void k_o4_refcheck(const unsigned long long* __restrict__ sum, unsigned long long want, int32_t* __restrict__ status) {
  if (*sum != want) atomicOr(status, 16);
}

// keys compared by (key & mask48) >> shift, under which they increase: the first of keys[lo, n) that is not below
// `target` (n: all are)
__device__ __forceinline__ int64_t o4_lower(const uint64_t* __restrict__ keys, int64_t n, uint64_t target, int shift,
                                            int64_t lo = 0) {
  int64_t hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (((keys[mid] & kMask48) >> shift) < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- the union of a window's key lists (history > 1): a merge, not a sort.  Element g of the call = element idx of
// list i of job j; what it is compared by is k_o4_ref's (key & mask48) >> shift, under which every list is strictly
// increasing.  An element is KEPT when no list in front of its own holds an equal key; the scan of the keep flags over
// all elements of the call gives, by differences, the kept elements below any place of any list, and a kept element's
// place in its union is the sum of those over the job's lists: no atomics, the same output every run.

// element g < total -> its job, list and index there (the jobs' bases increase from 0, every job has an element)
__device__ __forceinline__ void o4_mg_locate(const O4MergeDev* __restrict__ tab, int nj, int64_t g, int* job, int* list, int64_t* idx) {
  int lo = 0, hi = nj - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].base <= g) lo = mid; else hi = mid - 1;
  }
  const O4MergeDev& J = tab[lo];
  const int64_t e = g - J.base;
  int i = 0;
  while (i + 1 < J.nl && e >= J.off[i + 1]) ++i;
  *job = lo;
  *list = i;
  *idx = e - J.off[i];
}

// flags[g] = element g is kept; flags[total] = 0, so that the exclusive scan's entry `total` is the sum
__global__ __launch_bounds__(256) void k_o4_merge_flag(const O4MergeDev* __restrict__ tab, int nj, int64_t total, int shift,
                                                       uint32_t* __restrict__ flags) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > total) return;
  if (g == total) {
    flags[g] = 0u;
    return;
  }
  int job, i;
  int64_t idx;
  o4_mg_locate(tab, nj, g, &job, &i, &idx);
  const O4MergeDev& J = tab[job];
  const uint64_t k = (J.list[i][idx] & kMask48) >> shift;
  uint32_t keep = 1u;
  for (int l = 0; l < i; ++l) {
    const int64_t n = J.off[l + 1] - J.off[l];
    const int64_t at = o4_lower(J.list[l], n, k, shift);
    if (at < n && ((J.list[l][at] & kMask48) >> shift) == k) keep = 0u;
  }
  flags[g] = keep;
}

// excl: the exclusive scan of the flags, total + 1 entries.  A kept element goes to (kept elements with a smaller key,
// list by list); the first element of a job leaves the union's size
__global__ __launch_bounds__(256) void k_o4_merge_scatter(const O4MergeDev* __restrict__ tab, int nj, int64_t total, int shift,
                                                          const uint32_t* __restrict__ excl, uint32_t* __restrict__ counts) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  int job, i;
  int64_t idx;
  o4_mg_locate(tab, nj, g, &job, &i, &idx);
  const O4MergeDev& J = tab[job];
  if (g == J.base) counts[job] = excl[J.base + J.off[J.nl]] - excl[J.base];
  if (excl[g + 1] == excl[g]) return;
  const uint64_t key = J.list[i][idx];
  const uint64_t k = (key & kMask48) >> shift;
  int64_t pos = 0;
  for (int l = 0; l < J.nl; ++l) {
    const int64_t below = l == i ? idx : o4_lower(J.list[l], J.off[l + 1] - J.off[l], k, shift);
    const int64_t b = J.base + J.off[l];
    pos += (int64_t)(excl[b + below] - excl[b]);
  }
  J.out[pos] = key;   // pos < kept elements of the job <= its elements: the room the caller gave
}

// The nested unions of a job whose lists stand newest first (octree4.h): the flags and their scan are the merge's — a
// key is kept where no list in front of its own, a newer one, holds it — and a kept key of list i belongs to every
// union W > i.  Its place there is the kept keys below it in lists 0 .. W - 1, a running sum over the lists: one search
// per list for all unions, where a merge per union would search W lists each.  The first element of a job leaves the
// sizes: the kept keys of lists 0 .. W - 1, which lie in front of off[W].
__global__ __launch_bounds__(256) void k_o4_nest_scatter(const O4MergeDev* __restrict__ tab, const O4NestOut* __restrict__ outs, int nj,
                                                         int64_t total, int shift, const uint32_t* __restrict__ excl,
                                                         uint32_t* __restrict__ counts) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  int job, i;
  int64_t idx;
  o4_mg_locate(tab, nj, g, &job, &i, &idx);
  const O4MergeDev& J = tab[job];
  if (g == J.base)
    for (int W = 1; W <= kO4MaxWindow; ++W)
      counts[(int64_t)kO4MaxWindow * job + W - 1] = W <= J.nl ? excl[J.base + J.off[W]] - excl[J.base] : 0u;
  if (excl[g + 1] == excl[g]) return;
  const uint64_t key = J.list[i][idx];
  const uint64_t k = (key & kMask48) >> shift;
  int64_t pos = 0;
  for (int l = 0; l < J.nl; ++l) {
    const int64_t below = l == i ? idx : o4_lower(J.list[l], J.off[l + 1] - J.off[l], k, shift);
    const int64_t b = J.base + J.off[l];
    pos += (int64_t)(excl[b + below] - excl[b]);
    if (l < i) continue;
    uint64_t* o = outs[job].out[l];   // union l + 1
    if (o) o[pos] = key;              // pos < kept keys of lists 0 .. l <= their keys: the room the caller gave
  }
}

// status |= 16 where the union at hand has another size than the blob's ref_n
__global__ void k_o4_countcheck(const uint32_t* __restrict__ count, uint32_t want, int32_t* __restrict__ status) {
  if (*count != want) atomicOr(status, 16);
}

__global__ __launch_bounds__(256) void k_o4_popc(const uint8_t* __restrict__ occ, int64_t n, uint32_t* __restrict__ pc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pc[i] = (uint32_t)__popc((uint32_t)occ[i]);
}

// link[child] = parent << 3 | octant for the children of nodes [a, a + cnt): excl is the exclusive scan of their child
// counts, their children are the nodes (or leaves) from child_base on and must end at child_end exactly: status |= 8
__global__ __launch_bounds__(256) void k_o4_link(const uint8_t* __restrict__ occ, const uint32_t* __restrict__ excl, int64_t a,
                                                 int64_t cnt, int64_t child_base, int64_t child_end, uint32_t* __restrict__ link,
                                                 int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t byte = occ[a + i];
  const int64_t first = child_base + (int64_t)excl[i];
  if (i == cnt - 1 && first + __popc(byte) != child_end) atomicOr(status, 8);
  int k = 0;
  for (int j = 0; j < 8; ++j)
    if ((byte >> j) & 1u) {
      const int64_t child = first + k;
      if (child < child_end) link[child] = ((uint32_t)(a + i) << 3) | (uint32_t)j;
      ++k;
    }
}

// the reference byte of nodes [a, b): the node's cell from a walk up its links, then for every child octant whether
// the reference holds a key inside the child's cube — the cube of side 2^s at a corner that is a multiple of 2^s in
// biased coordinates is the key range [G, G + 8^s), so two lower bounds over the sorted keys answer a child.
// n_ref_dev (or nullptr): where a merge left the size of the union that the keys are, when the host cannot know it (a
// window at a level of detail); n_ref is then the room the keys have.
__global__ __launch_bounds__(256) void k_o4_ref(const uint32_t* __restrict__ link, O4Tree t, int64_t a, int64_t b,
                                                const uint64_t* __restrict__ ref_keys, int64_t n_ref,
                                                const uint32_t* __restrict__ n_ref_dev, uint8_t* __restrict__ rb) {
  const int64_t i = a + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b) return;
  if (n_ref_dev) n_ref = (int64_t)*n_ref_dev < n_ref ? (int64_t)*n_ref_dev : n_ref;
  int L = 0;
  while (L + 1 < t.depth && i >= t.off[L + 1]) ++L;
  uint64_t code = 0;
  uint32_t idx = (uint32_t)i;
  const uint32_t n_nodes = (uint32_t)t.off[t.depth];
  for (int d = 0; d < L; ++d) {
    const uint32_t l = link[idx < n_nodes ? idx : 0u];
    code |= (uint64_t)(l & 7u) << (3 * d);
    idx = l >> 3;
  }
  const int s = t.depth - L - 1;   // a child's cube has side 2^s
  const uint32_t cx = (pcc_compact3(code >> 2) << (s + 1)) + (uint32_t)(t.origin[0] + t.bias);
  const uint32_t cy = (pcc_compact3(code >> 1) << (s + 1)) + (uint32_t)(t.origin[1] + t.bias);
  const uint32_t cz = (pcc_compact3(code) << (s + 1)) + (uint32_t)(t.origin[2] + t.bias);
  const int shift = t.key_shift;
  // every child's own corner: a child's cube (s <= 15 - lod) is aligned under any bias that is a multiple of its side,
  // the node's own cube need not be (the root of a frame of cells under bias 32768), so the eight ranges are searched
  // one by one
  uint32_t byte = 0;
  for (int j = 0; j < 8; ++j) {
    const uint32_t jx = (uint32_t)((j >> 2) & 1) << s, jy = (uint32_t)((j >> 1) & 1) << s, jz = (uint32_t)(j & 1) << s;
    const uint64_t G = (pcc_spread3(cx + jx) << 2) | (pcc_spread3(cy + jy) << 1) | pcc_spread3(cz + jz);
    const int64_t lo = o4_lower(ref_keys, n_ref, G, shift), hi = o4_lower(ref_keys, n_ref, G + ((uint64_t)1 << (3 * s)), shift, lo);
    byte |= hi > lo ? 1u << j : 0u;
  }
  rb[i] = (uint8_t)byte;
}

// every leaf walks up its `depth` links: the octants on the way are its cell inside the root cube
__global__ __launch_bounds__(256) void k_o4_points(const uint32_t* __restrict__ link, O4Tree t, int32_t* __restrict__ points,
                                                   int32_t* __restrict__ status) {
  const int64_t n_nodes = t.off[t.depth], n_points = t.off[t.depth + 1] - n_nodes;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_points) return;
  uint64_t code = 0;
  uint32_t idx = (uint32_t)(n_nodes + e);
  for (int d = 0; d < t.depth; ++d) {
    const uint32_t l = link[idx];   // a link holds a node of the frame (or 0)
    code |= (uint64_t)(l & 7u) << (3 * d);
    idx = l >> 3;
  }
  if (idx != 0u) atomicOr(status, 8);
  points[3 * e] = (int32_t)pcc_compact3(code >> 2) + t.origin[0];
  points[3 * e + 1] = (int32_t)pcc_compact3(code >> 1) + t.origin[1];
  points[3 * e + 2] = (int32_t)pcc_compact3(code) + t.origin[2];
}

// At a cut (lod > 0): t.off[Lc] = N' nodes were decoded and t.off[Lc + 1] - N' cells hang below them.  Every cell walks
// up its Lc links; the octants on the way are its place among the cells of side 2^lod inside the root cube, whose
// corner is a multiple of 2^lod: the global cell index is ((cell << lod) + origin) >> lod, version 2's convention.
// Lc = 0: the one cell is the root cube's, origin >> lod.
__global__ __launch_bounds__(256) void k_o4_cells(const uint32_t* __restrict__ link, O4Tree t, int Lc, int lod,
                                                  int32_t* __restrict__ cells, int32_t* __restrict__ status) {
  const int64_t n_dec = t.off[Lc], m = t.off[Lc + 1] - n_dec;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  uint64_t code = 0;
  uint32_t idx = (uint32_t)(n_dec + e);
  for (int d = 0; d < Lc; ++d) {
    const uint32_t l = link[idx];   // a link holds one of the N' nodes (or 0)
    code |= (uint64_t)(l & 7u) << (3 * d);
    idx = l >> 3;
  }
  if (Lc > 0 && idx != 0u) atomicOr(status, 8);
  cells[3 * e] = (int32_t)(((int64_t)pcc_compact3(code >> 2) << lod) + t.origin[0]) >> lod;
  cells[3 * e + 1] = (int32_t)(((int64_t)pcc_compact3(code >> 1) << lod) + t.origin[1]) >> lod;
  cells[3 * e + 2] = (int32_t)(((int64_t)pcc_compact3(code) << lod) + t.origin[2]) >> lod;
}

// what k_o4_dec needs of a frame
struct O4Dec {
  int64_t table_off, payload_off;      // in the body (p0 | chunk table | payload)
  int64_t n_nodes, start_last, start_prev;
  int64_t words_here;                  // 16-bit words of the payload that are present (a prefix holds fewer than the table's sum)
  int32_t S;
};
constexpr int kCarryWords = 512;   // 32-bit words per slot: state, word position, 324 probabilities

// The nodes [a, b) of one level: block = chunk c_lo + blockIdx.x, every lane the part of its run of S nodes that lies in
// the level.  occ[node] receives the byte, pcl[node - a] its child count; status |= 1 words, 2 an empty node.
// carry: two slots; slot_in holds what the lane that began its run in an earlier level left, slot_out takes what the
// lane that goes on in a later level leaves.
__global__ __launch_bounds__(64) void k_o4_dec(const uint8_t* __restrict__ body, O4Dec d, int64_t a, int64_t b, int64_t c_lo,
                                               const uint8_t* __restrict__ rb, uint8_t* __restrict__ occ, uint32_t* __restrict__ pcl,
                                               uint32_t* __restrict__ carry, int slot_in, int slot_out,
                                               int32_t* __restrict__ status) {
  __shared__ uint16_t s_model[(kC4 + 1) * kLanes];   // [ctx][lane]; row kC4 takes the writes of decisions that are not coded
  __shared__ uint16_t s_words[kO4Win];
  const int lane = threadIdx.x;
  const int64_t c = c_lo + blockIdx.x;
  const uint16_t* p0 = reinterpret_cast<const uint16_t*>(body);
  const uint32_t* table = reinterpret_cast<const uint32_t*>(body + d.table_off);
  const uint16_t* payload = reinterpret_cast<const uint16_t*>(body + d.payload_off);
  const int S = d.S;
  const int64_t n_nodes = d.n_nodes;
  unsigned long long before = 0;
  for (int64_t j = lane; j < c; j += kLanes) before += table[j];
  for (int sh = 32; sh >= 1; sh >>= 1) before += __shfl_xor(before, sh, 64);
  const uint32_t cw = (uint32_t)__builtin_amdgcn_readfirstlane((int)table[c]);
  // The chunk table's sum is the payload's length (o4_parse_lod), and of a whole blob all of it is here.  Of a prefix
  // the last needed chunk is here as far as its lane l* (the host's plan): states and length table must be, and no word
  // is read behind the `here` that are
  if (cw < 3u * kLanes || before + 3ull * kLanes > (unsigned long long)d.words_here) {   // wave-uniform
    if (lane == 0) atomicOr(status, 1);
    return;
  }
  const uint16_t* p = payload + before;
  const unsigned long long left = (unsigned long long)d.words_here - before;
  const uint32_t here = left < (unsigned long long)cw ? (uint32_t)left : cw;
  const uint32_t my_len = p[2 * kLanes + lane];
  uint32_t incl = my_len;
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, sh, 64);
    incl += lane >= sh ? o : 0u;
  }
  if (3u * kLanes + (uint32_t)__shfl((int)incl, 63, 64) != cw) {   // wave-uniform
    if (lane == 0) atomicOr(status, 1);
    return;
  }
  const uint32_t rbase = 3u * kLanes + incl - my_len, rend = rbase + my_len;
  const int64_t node0 = (c * kLanes + lane) * S;
  const int64_t lo = node0 > a ? node0 : a, hi = node0 + S < b ? node0 + S : b;
  const bool active = lo < hi;
  const bool carry_in = active && lo > node0;                   // the run began in an earlier level
  const bool carry_out = active && hi < node0 + S && hi < n_nodes;   // and goes on in a later one
  const unsigned long long act_mask = __ballot(active);
  if (act_mask == 0ull) return;
  if (__ballot(active && rend > here) != 0ull) {   // a lane that decodes owns words that are not here (never a whole blob's)
    if (lane == 0) atomicOr(status, 1);
    return;
  }
  int bad = (node0 >= n_nodes && my_len != 0u) ? 1 : 0;   // a lane without nodes has no words
  // the model: the frame's initial probabilities, or what the lane left behind
  for (int ctx = 0; ctx < kC4; ++ctx) s_model[ctx * kLanes + lane] = p0[ctx];
  uint32_t x = (uint32_t)p[2 * lane] | ((uint32_t)p[2 * lane + 1] << 16);
  uint32_t pos = rbase;
  if (carry_in) {
    const uint32_t* cin = carry + (size_t)slot_in * kCarryWords;
    x = cin[0];
    pos = cin[1];
    for (int ctx = 0; ctx < kC4; ctx += 2) {
      const uint32_t v = cin[2 + (ctx >> 1)];
      s_model[ctx * kLanes + lane] = (uint16_t)v;
      s_model[(ctx + 1) * kLanes + lane] = (uint16_t)(v >> 16);
    }
  }
  // the words of the lanes that decode here, in LDS when they fit
  const int first_lane = (int)__builtin_ctzll(act_mask), last_lane = 63 - (int)__builtin_clzll(act_mask);
  const uint32_t w_lo = (uint32_t)__shfl((int)rbase, first_lane, 64), w_hi = (uint32_t)__shfl((int)rend, last_lane, 64);
  const bool in_lds = w_hi > w_lo && w_hi - w_lo <= (uint32_t)kO4Win;   // wave-uniform
  if (in_lds)
    for (uint32_t i = lane; i < w_hi - w_lo; i += kLanes) s_words[i] = p[w_lo + i];
  __syncthreads();
  auto word_at = [&](uint32_t i) -> uint32_t {
    if (in_lds) {
      const uint32_t ic = i < w_lo ? w_lo : (i >= w_hi ? w_hi - 1u : i);
      return s_words[ic - w_lo];
    }
    return p[i < here ? i : here - 1u];   // a lane at the end of its run looks one word too far: never used
  };
  uint32_t nextw = word_at(pos);
  // steps [s_lo, s_hi) of the runs: what some lane of the wave decodes
  int s_lo = active ? (int)(lo - node0) : S, s_hi = active ? (int)(hi - node0) : 0;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    s_lo = min(s_lo, __shfl_xor(s_lo, sh, 64));
    s_hi = max(s_hi, __shfl_xor(s_hi, sh, 64));
  }
  const int a_dummy = kC4 * kLanes + lane;
  // As in version 2's decoder, the model entry of the NEXT decision is requested before the current one is decoded —
  // both candidates (the ones so far, and one more) — so that the LDS round trip is not on the chain from state to
  // state; the reference byte of a node is requested two nodes ahead.  (Two decisions never share a model row: the
  // row is r, level class, bit position and ones so far.)
  auto rb_at = [&](int64_t node) -> uint32_t { return (active && node >= lo && node < hi) ? (uint32_t)rb[node] : 0u; };
  auto row0_of = [&](int64_t node, uint32_t rbyte) -> int {   // the row of a node's decision 0
    return (rbyte == 0u ? 0 : 108 * (1 + (int)(rbyte & 1u))) + (node >= d.start_last ? 0 : (node >= d.start_prev ? 1 : 2)) * 36;
  };
  uint32_t rbyte = rb_at(node0 + s_lo), rbyte_next = rb_at(node0 + s_lo + 1);
  uint32_t p_cur = s_model[row0_of(node0 + s_lo, rbyte) * kLanes + lane];
  for (int s = s_lo; s < s_hi; ++s) {
    const int64_t node = node0 + s;
    const bool valid = active && node >= lo && node < hi;
    const uint32_t rbyte_after = rb_at(node + 2);
    const int cbase = (node >= d.start_last ? 0 : (node >= d.start_prev ? 1 : 2)) * 36;
    int ones = 0;
    uint32_t byte = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = rbyte == 0u ? 0 : 1 + (int)((rbyte >> j) & 1u);
      const bool act = valid && !(j == 7 && ones == 0);
      const int at = act ? (r * 108 + cbase + j * (j + 1) / 2 + ones) * kLanes + lane : a_dummy;
      uint32_t c0, c1 = 0;
      if (j < 7) {
        const int rn = rbyte == 0u ? 0 : 1 + (int)((rbyte >> (j + 1)) & 1u);
        const int an = (rn * 108 + cbase + (j + 1) * (j + 2) / 2 + ones) * kLanes + lane;
        c0 = s_model[an];
        c1 = s_model[an + kLanes];
      } else {
        c0 = s_model[row0_of(node + 1, rbyte_next) * kLanes + lane];   // decision 0 of the next node
      }
      const uint32_t p1 = p_cur;
      const uint32_t cum = x & 4095u;
      const uint32_t dbit = cum >= 4096u - p1 ? 1u : 0u;
      const uint32_t start = dbit ? 4096u - p1 : 0u, freq = dbit ? p1 : 4096u - p1;
      const uint32_t xn = freq * (x >> 12) + cum - start;
      x = act ? xn : x;
      s_model[at] = (uint16_t)o2_adapt(p1, dbit);
      const uint32_t bit = act ? dbit : (valid ? 1u : 0u);   // else: the implied bit
      const bool need = act && x < kL;
      bad |= (need && pos >= rend) ? 1 : 0;
      x = need ? (x << 16) | nextw : x;
      pos += need ? 1u : 0u;
      nextw = word_at(pos);
      ones += (int)bit;
      byte |= bit << j;
      p_cur = (j < 7 && bit) ? c1 : c0;
    }
    rbyte = rbyte_next;
    rbyte_next = rbyte_after;
    if (valid) {   // node < b <= n_nodes: inside the arrays the host sized from the header
      bad |= byte == 0u ? 2 : 0;
      occ[node] = (uint8_t)byte;
      pcl[node - a] = (uint32_t)__popc(byte);
    }
  }
  if (carry_out) {
    uint32_t* cout = carry + (size_t)slot_out * kCarryWords;
    cout[0] = x;
    cout[1] = pos;
    for (int ctx = 0; ctx < kC4; ctx += 2)
      cout[2 + (ctx >> 1)] = (uint32_t)s_model[ctx * kLanes + lane] | ((uint32_t)s_model[(ctx + 1) * kLanes + lane] << 16);
  } else if (active && pos != rend) {
    bad |= 1;   // the run is complete: every word of it consumed
  }
  const unsigned long long b1 = __ballot((bad & 1) != 0), b2 = __ballot((bad & 2) != 0);
  if (lane == 0 && (b1 | b2) != 0ull) atomicOr(status, (b1 ? 1 : 0) | (b2 ? 2 : 0));
}

inline int64_t o4_round(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace

// ======================================================================== encoder: the reference bytes
size_t o4_ref_scratch_bytes(int64_t n_nodes, int64_t n_points) {
  return 2 * pcc_align((size_t)n_nodes * 4) + pcc_align((size_t)(n_nodes + n_points) * 4) + 1024;
}

int o4_ref_bytes_async(pcc_ctx* ctx, int key_shift, const O4RefJob* jobs, int nf, const uint8_t* occ,
                       uint8_t* rb, uint32_t* ref_n, unsigned long long* ref_sum, char* scratch, size_t scratch_b) {
  hipStream_t st = ctx->stream;
  for (int f = 0; f < nf; ++f) PCC_HIP(hipMemsetD32Async((hipDeviceptr_t)(ref_n + f), (int)(uint32_t)jobs[f].ref_n, 1, st));
  PCC_HIP(hipMemsetAsync(ref_sum, 0, (size_t)nf * 8, st));
  const int bias = 32768 >> (key_shift / 3);
  for (int f = 0; f < nf; ++f) {
    const O4RefJob& j = jobs[f];
    const int64_t N = j.off[j.depth];
    PCC_REQUIRE(o4_ref_scratch_bytes(N, j.n_points) <= scratch_b && j.ref_n >= 1, PCC_E_NOMEM,
                "octree blob v4: frame %d: scratch of the reference bytes", f);
    uint32_t* pc = (uint32_t*)scratch;
    uint32_t* excl = (uint32_t*)(scratch + pcc_align((size_t)N * 4));
    uint32_t* link = (uint32_t*)(scratch + 2 * pcc_align((size_t)N * 4));
    O4Tree t;
    for (int L = 0; L < 18; ++L) t.off[L] = L <= j.depth ? j.off[L] : N + j.n_points;
    t.depth = j.depth;
    for (int a = 0; a < 3; ++a) t.origin[a] = j.origin[a];
    t.bias = bias;
    t.key_shift = key_shift;
    const uint8_t* o = occ + j.occ_off;
    if (f == 0 || jobs[f - 1].occ_off != j.occ_off) {   // (else: the tree of the job before, its links still in the scratch)
      PCC_HIP(hipMemsetAsync(link, 0, 4, st));   // the root's link; every other node's is written
      hipLaunchKernelGGL(k_o4_popc, dim3(nblk(N, 256)), dim3(256), 0, st, o, N, pc);
      PCC_CHECK_LAUNCH();
      PCC_TRY(pcc_scan_exclusive_u32(ctx, pc, excl, N, nullptr));
      // the whole tree at once: the first child of node i is node 1 + (child counts in front of i); the encoder's own
      // bytes need no check, the status word is the scratch's tail
      int32_t* st_dummy = (int32_t*)(scratch + scratch_b - 256);
      hipLaunchKernelGGL(k_o4_link, dim3(nblk(N, 256)), dim3(256), 0, st, o, (const uint32_t*)excl, (int64_t)0, N, (int64_t)1,
                         N + j.n_points, link, st_dummy);
      PCC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_o4_ref, dim3(nblk(N, 256)), dim3(256), 0, st, (const uint32_t*)link, t, (int64_t)0, N, j.ref_keys,
                       j.ref_n, (const uint32_t*)nullptr, rb + j.rb_off);
    PCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_o4_keysum, dim3(nblk(j.ref_n, 256)), dim3(256), 0, st, j.ref_keys, j.ref_n, key_shift, bias,
                       ref_sum + f);
    PCC_CHECK_LAUNCH();
  }
  return PCC_OK;
}

// ======================================================================== the merged reference of a window
size_t o4_merge_scratch_bytes(int64_t total, int nj) {
  return pcc_align((size_t)(total + 1) * 4 + 16) + pcc_align((size_t)nj * sizeof(O4MergeDev)) + pcc_align((size_t)nj * 4);
}

int o4_merge_async(pcc_ctx* ctx, const O4MergeJob* jobs, int nj, int key_shift, char* scratch, size_t scratch_b, O4MergeDev* h_tab,
                   uint32_t** d_counts) {
  hipStream_t st = ctx->stream;
  int64_t total = 0;
  for (int j = 0; j < nj; ++j) {
    const O4MergeJob& g = jobs[j];
    O4MergeDev& d = h_tab[j];
    PCC_REQUIRE(g.nl >= 1 && g.nl <= kO4MaxWindow && g.out, PCC_E_ARG, "merge of key lists: job %d has %d lists", j, g.nl);
    d.base = total;
    d.out = g.out;
    d.nl = g.nl;
    int64_t run = 0;
    for (int i = 0; i <= kO4MaxWindow; ++i) {
      d.off[i] = run;
      if (i < kO4MaxWindow) d.list[i] = i < g.nl ? g.list[i] : nullptr;
      if (i < g.nl) {
        PCC_REQUIRE(g.n[i] >= 0 && (g.n[i] == 0 || g.list[i]), PCC_E_ARG, "merge of key lists: job %d, list %d", j, i);
        run += g.n[i];
      }
    }
    PCC_REQUIRE(run >= 1, PCC_E_ARG, "merge of key lists: job %d has no keys", j);
    total += run;
  }
  PCC_REQUIRE(nj >= 1 && total + 1 < ((int64_t)1 << 31) && o4_merge_scratch_bytes(total, nj) <= scratch_b, PCC_E_ARG,
              "merge of key lists: %lld keys in %d jobs", (long long)total, nj);
  uint32_t* flags = (uint32_t*)scratch;
  O4MergeDev* d_tab = (O4MergeDev*)(scratch + pcc_align((size_t)(total + 1) * 4 + 16));
  uint32_t* counts = (uint32_t*)((char*)d_tab + pcc_align((size_t)nj * sizeof(O4MergeDev)));
  PCC_TRY(pcc_arena_reserve(ctx, pcc_scan_scratch_bytes(total + 1) + 1024));
  PCC_HIP(hipMemcpyAsync(d_tab, h_tab, (size_t)nj * sizeof(O4MergeDev), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_o4_merge_flag, dim3(nblk(total + 1, 256)), dim3(256), 0, st, (const O4MergeDev*)d_tab, nj, total, key_shift, flags);
  PCC_CHECK_LAUNCH();
  PCC_TRY(pcc_scan_exclusive_u32(ctx, flags, flags, total + 1, nullptr));
  hipLaunchKernelGGL(k_o4_merge_scatter, dim3(nblk(total, 256)), dim3(256), 0, st, (const O4MergeDev*)d_tab, nj, total, key_shift,
                     (const uint32_t*)flags, counts);
  PCC_CHECK_LAUNCH();
  *d_counts = counts;
  return PCC_OK;
}

size_t o4_nest_scratch_bytes(int64_t total, int nj) {
  return o4_merge_scratch_bytes(total, nj) + pcc_align((size_t)nj * sizeof(O4NestOut)) + pcc_align((size_t)nj * kO4MaxWindow * 4);
}

int o4_nest_async(pcc_ctx* ctx, const O4NestJob* jobs, int nj, int key_shift, char* scratch, size_t scratch_b, O4MergeDev* h_tab,
                  O4NestOut* h_out, uint32_t** d_counts) {
  hipStream_t st = ctx->stream;
  int64_t total = 0;
  for (int j = 0; j < nj; ++j) {
    const O4NestJob& g = jobs[j];
    O4MergeDev& d = h_tab[j];
    PCC_REQUIRE(g.nl >= 1 && g.nl <= kO4MaxWindow, PCC_E_ARG, "nested unions of key lists: job %d has %d lists", j, g.nl);
    d.base = total;
    d.out = nullptr;
    d.nl = g.nl;
    int64_t run = 0;
    for (int i = 0; i <= kO4MaxWindow; ++i) {
      d.off[i] = run;
      if (i < kO4MaxWindow) {
        d.list[i] = i < g.nl ? g.list[i] : nullptr;
        h_out[j].out[i] = i < g.nl ? g.out[i] : nullptr;
      }
      if (i < g.nl) {
        PCC_REQUIRE(g.n[i] >= 0 && (g.n[i] == 0 || g.list[i]), PCC_E_ARG, "nested unions of key lists: job %d, list %d", j, i);
        run += g.n[i];
      }
    }
    PCC_REQUIRE(run >= 1, PCC_E_ARG, "nested unions of key lists: job %d has no keys", j);
    total += run;
  }
  PCC_REQUIRE(nj >= 1 && total + 1 < ((int64_t)1 << 31) && o4_nest_scratch_bytes(total, nj) <= scratch_b, PCC_E_ARG,
              "nested unions of key lists: %lld keys in %d jobs", (long long)total, nj);
  uint32_t* flags = (uint32_t*)scratch;
  O4MergeDev* d_tab = (O4MergeDev*)(scratch + pcc_align((size_t)(total + 1) * 4 + 16));
  O4NestOut* d_out = (O4NestOut*)(scratch + o4_merge_scratch_bytes(total, nj));
  uint32_t* counts = (uint32_t*)((char*)d_out + pcc_align((size_t)nj * sizeof(O4NestOut)));
  PCC_TRY(pcc_arena_reserve(ctx, pcc_scan_scratch_bytes(total + 1) + 1024));
  PCC_HIP(hipMemcpyAsync(d_tab, h_tab, (size_t)nj * sizeof(O4MergeDev), hipMemcpyHostToDevice, st));
  PCC_HIP(hipMemcpyAsync(d_out, h_out, (size_t)nj * sizeof(O4NestOut), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_o4_merge_flag, dim3(nblk(total + 1, 256)), dim3(256), 0, st, (const O4MergeDev*)d_tab, nj, total, key_shift, flags);
  PCC_CHECK_LAUNCH();
  PCC_TRY(pcc_scan_exclusive_u32(ctx, flags, flags, total + 1, nullptr));
  hipLaunchKernelGGL(k_o4_nest_scatter, dim3(nblk(total, 256)), dim3(256), 0, st, (const O4MergeDev*)d_tab, (const O4NestOut*)d_out, nj,
                     total, key_shift, (const uint32_t*)flags, counts);
  PCC_CHECK_LAUNCH();
  *d_counts = counts;
  return PCC_OK;
}

namespace {
// a block of the call's own, and host memory on its way to the device: both outlive what the stream still holds
struct O4Own {
  hipStream_t st;
  void* p = nullptr;
  std::vector<O4MergeDev> tab;
  explicit O4Own(hipStream_t s) : st(s) {}
  ~O4Own() {
    if (!tab.empty()) (void)hipStreamSynchronize(st);
    if (p) (void)hipFree(p);
  }
};
}  // namespace

extern "C" int pcc_merge_keys_nested(pcc_ctx* ctx, const uint64_t* const* d_lists, const int64_t* h_n, int n_lists, int key_shift,
                                     uint64_t* d_out, int64_t cap, int64_t* h_counts) {
  const char* who = "pcc_merge_keys_nested";
  PCC_REQUIRE(ctx && d_lists && h_n && h_counts && n_lists >= 1 && n_lists <= kO4MaxWindow && key_shift >= 0 && key_shift % 3 == 0 &&
                  key_shift <= 45 && cap >= 0,
              PCC_E_ARG, "%s: bad argument (n_lists=%d key_shift=%d)", who, n_lists, key_shift);
  O4NestJob job;
  int64_t total = 0, room = 0;
  for (int i = 0; i < n_lists; ++i) {
    PCC_REQUIRE(h_n[i] >= 0 && h_n[i] < ((int64_t)1 << 27) && (h_n[i] == 0 || d_lists[i]), PCC_E_ARG, "%s: list %d has %lld keys", who, i,
                (long long)h_n[i]);
    job.list[i] = d_lists[i];
    job.n[i] = h_n[i];
    job.out[i] = d_out ? d_out + room : nullptr;   // union i + 1: behind the rooms of the narrower ones
    total += h_n[i];
    room += total;
    h_counts[i] = 0;
  }
  job.nl = n_lists;
  if (total == 0) return PCC_OK;
  PCC_REQUIRE(total < ((int64_t)1 << 27), PCC_E_ARG, "%s: %lld keys in the lists", who, (long long)total);
  PCC_REQUIRE(d_out && cap >= room, PCC_E_NOMEM, "%s: the unions take room for %lld keys, %lld are given", who, (long long)room,
              (long long)cap);
  O4Own own(ctx->stream);
  const size_t scratch_b = o4_nest_scratch_bytes(total, 1);
  PCC_HIP(hipMalloc(&own.p, scratch_b));
  own.tab.resize(1);
  O4NestOut h_out;   // (on its way to the device until the synchronisation below, or own's)
  uint32_t* d_counts = nullptr;
  PCC_TRY(o4_nest_async(ctx, &job, 1, key_shift, (char*)own.p, scratch_b, own.tab.data(), &h_out, &d_counts));
  uint32_t counts[kO4MaxWindow];
  PCC_HIP(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  PCC_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < n_lists; ++i) h_counts[i] = (int64_t)counts[i];
  return PCC_OK;
}

extern "C" int pcc_merge_keys(pcc_ctx* ctx, const uint64_t* const* d_lists, const int64_t* h_n, int n_lists, int key_shift,
                              uint64_t* d_out, int64_t cap, int64_t* h_count) {
  const char* who = "pcc_merge_keys";
  PCC_REQUIRE(ctx && d_lists && h_n && h_count && n_lists >= 1 && n_lists <= kO4MaxWindow && key_shift >= 0 && key_shift % 3 == 0 &&
                  key_shift <= 45 && cap >= 0,
              PCC_E_ARG, "%s: bad argument (n_lists=%d key_shift=%d)", who, n_lists, key_shift);
  O4MergeJob job;
  int64_t total = 0;
  for (int i = 0; i < n_lists; ++i) {
    PCC_REQUIRE(h_n[i] >= 0 && h_n[i] < ((int64_t)1 << 27) && (h_n[i] == 0 || d_lists[i]), PCC_E_ARG, "%s: list %d has %lld keys", who, i,
                (long long)h_n[i]);
    job.list[i] = d_lists[i];
    job.n[i] = h_n[i];
    total += h_n[i];
  }
  job.nl = n_lists;
  job.out = d_out;
  *h_count = 0;
  if (total == 0) return PCC_OK;
  PCC_REQUIRE(d_out && cap >= total, PCC_E_NOMEM, "%s: %lld keys in the lists, room for %lld", who, (long long)total, (long long)cap);
  O4Own own(ctx->stream);
  const size_t scratch_b = o4_merge_scratch_bytes(total, 1);
  PCC_HIP(hipMalloc(&own.p, scratch_b));
  own.tab.resize(1);
  uint32_t* d_count = nullptr;
  PCC_TRY(o4_merge_async(ctx, &job, 1, key_shift, (char*)own.p, scratch_b, own.tab.data(), &d_count));
  uint32_t count = 0;
  PCC_HIP(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCC_HIP(hipStreamSynchronize(ctx->stream));
  *h_count = (int64_t)count;
  return PCC_OK;
}

// ======================================================================== decoder
// one predicted frame, queued on the stream: d_body = p0 | chunk table | payload of the blob as far as the plan's bytes
// (on the device), the reference's keys (bias 32768, sorted) and its sum as k_o4_keys left them -> the frame's points.
// At a cut (pl.lod > 0): levels 0 .. Lc - 1 alone, every array sized from N' and m, the keys those of the reference's
// cells' corners (d_ref_count: the size of a window's union, where the host does not know it) -> the frame's m cells;
// ref_sum is of full-resolution points and is not compared.  The arena is this frame's: reserved here.
static int o4_decode_one(pcc_ctx* ctx, const O4Info& o, const O4Plan& pl, const uint8_t* d_body, const uint64_t* d_ref_keys,
                         int64_t n_ref, const uint32_t* d_ref_count, const unsigned long long* d_ref_sum, int32_t* d_points,
                         int32_t* d_status) {
  hipStream_t st = ctx->stream;
  const int64_t N = pl.n_dec, n = pl.m;
  const int Lc = pl.Lc, lod = pl.lod;
  O4Tree t;
  int64_t run = 0;
  for (int L = 0; L < 18; ++L) {
    t.off[L] = run;
    if (L < Lc) run += o.level_n[L];
    else if (L == Lc) run += n;
  }
  t.depth = o.depth;
  for (int a = 0; a < 3; ++a) t.origin[a] = o.origin[a];
  t.bias = 32768;
  t.key_shift = 0;
  if (Lc == 0) {   // (lod >= depth) nothing to decode: the root cube is the one cell
    hipLaunchKernelGGL(k_o4_cells, dim3(1), dim3(256), 0, st, (const uint32_t*)nullptr, t, 0, lod, d_points, d_status);
    PCC_CHECK_LAUNCH();
    return PCC_OK;
  }
  int64_t max_level = 1;
  size_t scan_b = 0;
  for (int L = 0; L < Lc; ++L) {
    max_level = std::max(max_level, o.level_n[L]);
    scan_b += pcc_scan_scratch_bytes(o.level_n[L]) + 512;
  }
  PCC_TRY(pcc_arena_reserve(ctx, 2 * pcc_align((size_t)N + 16) + 2 * pcc_align((size_t)max_level * 4 + 16) +
                                     pcc_align((size_t)(N + n) * 4) + pcc_align(2 * kCarryWords * 4) + scan_b + 8192));
  uint8_t* occ = (uint8_t*)pcc_arena_alloc(ctx, (size_t)N + 16);
  uint8_t* rb = (uint8_t*)pcc_arena_alloc(ctx, (size_t)N + 16);
  uint32_t* pcl = (uint32_t*)pcc_arena_alloc(ctx, (size_t)max_level * 4 + 16);
  uint32_t* excl = (uint32_t*)pcc_arena_alloc(ctx, (size_t)max_level * 4 + 16);
  uint32_t* link = (uint32_t*)pcc_arena_alloc(ctx, (size_t)(N + n) * 4);
  uint32_t* carry = (uint32_t*)pcc_arena_alloc(ctx, 2 * kCarryWords * 4);
  if (!occ || !rb || !pcl || !excl || !link || !carry) return PCC_E_NOMEM;
  O4Dec d;
  d.table_off = o.off_table - o.off_p0;
  d.payload_off = o.off_payload - o.off_p0;
  d.n_nodes = o.n_nodes;   // of the whole tree: the level classes and the lanes' runs are the whole tree's
  d.start_last = o.n_nodes - o.level_n[o.depth - 1];
  d.start_prev = o.depth >= 2 ? d.start_last - o.level_n[o.depth - 2] : 0;
  d.words_here = lod == 0 ? o.payload_words : pl.last_off + pl.last_words;
  d.S = (int32_t)o.S;
  if (lod == 0) {
    hipLaunchKernelGGL(k_o4_refcheck, dim3(1), dim3(1), 0, st, d_ref_sum, (unsigned long long)o.ref_sum, d_status);
    PCC_CHECK_LAUNCH();
  }
  PCC_HIP(hipMemsetAsync(link, 0, (size_t)(N + n) * 4, st));
  const int64_t per_chunk = (int64_t)kLanes * o.S;
  for (int L = 0; L <= Lc; ++L) {
    const int64_t a = t.off[L], b = t.off[L + 1];
    if (L > 0) {   // the links of this level's nodes (L == Lc: of the leaves, or cells) from the child counts of the level above
      const int64_t pa = t.off[L - 1], cnt = a - pa;
      PCC_TRY(pcc_scan_exclusive_u32(ctx, pcl, excl, cnt, nullptr));
      hipLaunchKernelGGL(k_o4_link, dim3(nblk(cnt, 256)), dim3(256), 0, st, (const uint8_t*)occ, (const uint32_t*)excl, pa, cnt, a, b,
                         link, d_status);
      PCC_CHECK_LAUNCH();
    }
    if (L == Lc) break;
    hipLaunchKernelGGL(k_o4_ref, dim3(nblk(b - a, 256)), dim3(256), 0, st, (const uint32_t*)link, t, a, b, d_ref_keys, n_ref,
                       d_ref_count, rb);
    PCC_CHECK_LAUNCH();
    // < nc: the header's check of S and nc; at a cut <= c*, and the last lane of level Lc - 1 may stop in the middle of
    // its run: it leaves a carry that nothing picks up
    const int64_t c_lo = a / per_chunk, c_hi = (b - 1) / per_chunk;
    hipLaunchKernelGGL(k_o4_dec, dim3((unsigned)(c_hi - c_lo + 1)), dim3(64), 0, st, d_body, d, a, b, c_lo, (const uint8_t*)rb, occ,
                       pcl, carry, (L + 1) & 1, L & 1, d_status);
    PCC_CHECK_LAUNCH();
  }
  if (lod == 0)
    hipLaunchKernelGGL(k_o4_points, dim3(nblk(n, 256)), dim3(256), 0, st, (const uint32_t*)link, t, d_points, d_status);
  else
    hipLaunchKernelGGL(k_o4_cells, dim3(nblk(n, 256)), dim3(256), 0, st, (const uint32_t*)link, t, Lc, lod, d_points, d_status);
  PCC_CHECK_LAUNCH();
  return PCC_OK;
}

static int o4_named(int rc, const char* who, int frame) {
  const std::string m = pcc_last_error();
  pcc_set_error("%s: frame %d: %s", who, frame, m.c_str());
  return rc;
}

// The frames of a decode call have positions: the caller's references (oldest first), then the blobs' frames.  A
// version-4 blob whose byte 3 holds W - 1 is coded against the union of the W frames in front of its own.
// lod > 0: blobs or prefixes of them, the references and every decoded frame the CELLS at that lod.  The keys the call
// keeps are those of the cells' corners, under which the range search and the merge run as they do at lod 0.  ref_n and
// ref_sum describe full-resolution points that nobody here holds: they are not compared, on the host or on the device
// (include/pcc.h says what a wrong reference then gives); every bound comes from the header's checks, the prefix's
// length and the rows at hand.  lod 0 queues what it queued before levels of detail.
static int o4_decode_frames(const char* who, pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                            const int32_t* const* d_refs, const int64_t* n_ref, int n_refs, int lod, int32_t* d_points,
                            int32_t* h_points, int64_t cap_points, int64_t* h_point_offsets) {
  const int nb = n_frames;
  std::vector<int> ver((size_t)nb);
  std::vector<O4Info> info((size_t)nb);
  std::vector<O4Plan> plan((size_t)nb);
  std::vector<int64_t> rows((size_t)nb);   // points, or cells, of every frame
  int64_t points = 0, bodies = 0, max_n = 0;
  for (int r = 0; r < n_refs; ++r) max_n = std::max(max_n, n_ref[r]);
  h_point_offsets[0] = 0;
  int max_w = 1;
  for (int f = 0; f < nb; ++f) {
    if (lod == 0) {
      const int v = pcc_octree_inter_info(h_blobs[f], h_lens[f], &ver[(size_t)f], &rows[(size_t)f], nullptr, nullptr);
      if (v != PCC_OK) return o4_named(v, who, f);
    } else if (h_blobs[f] && h_lens[f] >= kO2Header && h_blobs[f][0] == 'O' && h_blobs[f][1] == 2) {
      O2Info o2;
      O2Plan pl2;
      const int rc = o2_parse(h_blobs[f], h_lens[f], lod, true, &o2, &pl2);
      if (rc != PCC_OK) return o4_named(rc, who, f);
      ver[(size_t)f] = 2;
      rows[(size_t)f] = pl2.m;
    } else {
      ver[(size_t)f] = 4;   // or no blob of the two versions: o4_parse_lod's "bad header"
    }
    if (ver[(size_t)f] == 4) {
      const int rc = o4_parse_lod(h_blobs[f], h_lens[f], lod, true, &info[(size_t)f], &plan[(size_t)f]);
      if (rc != PCC_OK) return o4_named(rc, who, f);
      PCC_REQUIRE(info[(size_t)f].window <= kO4MaxWindow, PCC_E_STREAM, "%s: frame %d: octree blob v4: a window of %d frames (byte 3), at most %d",
                  who, f, info[(size_t)f].window, kO4MaxWindow);
      max_w = std::max(max_w, info[(size_t)f].window);
      rows[(size_t)f] = plan[(size_t)f].m;
      bodies += o4_round(plan[(size_t)f].bytes - info[(size_t)f].off_p0, 16);
    }
    points += rows[(size_t)f];
    max_n = std::max(max_n, rows[(size_t)f]);
    h_point_offsets[f + 1] = points;
  }
  PCC_REQUIRE(points < ((int64_t)1 << 31), PCC_E_ARG, "%s: the blobs announce %lld points in all", who, (long long)points);
  if (points == 0 || (!d_points && !h_points)) return PCC_OK;
  PCC_REQUIRE(cap_points >= points, PCC_E_NOMEM, "%s: %lld points, capacity %lld", who, (long long)points, (long long)cap_points);
  // what a predicted frame is coded against: the frames decoded before it, in front of blob 0 the caller's
  auto n_at = [&](int q) { return q < n_refs ? n_ref[q] : rows[(size_t)(q - n_refs)]; };
  int64_t max_window = 0;   // keys of the largest window of more than one frame
  for (int f = 0; f < nb; ++f) {
    if (ver[(size_t)f] != 4) continue;
    const O4Info& o = info[(size_t)f];
    const int p = n_refs + f, W = o.window;
    PCC_REQUIRE(p > 0 || W > 1, PCC_E_ARG, "%s: frame 0: a predicted frame (blob version 4) needs its reference", who);
    PCC_REQUIRE(W <= p, PCC_E_ARG, "%s: frame %d: a predicted frame (blob version 4) needs %d frames in front of it, %d are here", who, f,
                W, p);
    if (W == 1) {
      PCC_REQUIRE(lod > 0 || n_at(p - 1) == (int64_t)o.ref_n, PCC_E_ARG,
                  "%s: frame %d: the reference differs: it has %lld points, the blob was coded against %u", who, f,
                  (long long)n_at(p - 1), o.ref_n);
      PCC_REQUIRE(n_at(p - 1) >= 1, PCC_E_ARG, "%s: frame %d: the reference differs: it has no cells", who, f);
      continue;
    }
    int64_t most = 0, sum = 0;
    for (int q = p - W; q < p; ++q) {
      most = std::max(most, n_at(q));
      sum += n_at(q);
    }
    PCC_REQUIRE((lod > 0 ? most >= 1 : most <= (int64_t)o.ref_n && (int64_t)o.ref_n <= sum) && sum < ((int64_t)1 << 27), PCC_E_ARG,
                "%s: frame %d: the reference differs: the %d frames in front of it have %lld .. %lld distinct points, the blob was coded "
                "against %u",
                who, f, W, (long long)most, (long long)sum, o.ref_n);
    max_window = std::max(max_window, sum);
  }
  // the call's own block (the arena is each frame's in turn): points | keys of the last max_w frames | a window's union
  // and the merge's scratch | bodies | sums (per position, per blob) | status
  hipStream_t st = ctx->stream;
  O4Own own(st);
  const int npos = n_refs + nb;
  const size_t pts_b = d_points ? 0 : pcc_align((size_t)points * 12), slot_b = pcc_align((size_t)max_n * 8 + 16);
  const size_t keys_b = (size_t)max_w * slot_b, union_b = max_window ? pcc_align((size_t)max_window * 8 + 16) : 0;
  const size_t merge_b = max_window ? o4_merge_scratch_bytes(max_window, 1) : 0;
  const size_t bodies_b = pcc_align((size_t)bodies + 16), sums_b = pcc_align((size_t)(npos + nb) * 8), stat_b = pcc_align((size_t)nb * 4);
  PCC_HIP(hipMalloc(&own.p, pts_b + keys_b + union_b + merge_b + bodies_b + sums_b + stat_b));
  char* base = (char*)own.p;
  int32_t* pts = d_points ? d_points : (int32_t*)base;
  char* ring = base + pts_b;
  uint64_t* merged = (uint64_t*)(ring + keys_b);
  char* merge_scratch = ring + keys_b + union_b;
  uint8_t* d_bodies = (uint8_t*)(merge_scratch + merge_b);
  unsigned long long* sums = (unsigned long long*)((char*)d_bodies + bodies_b);   // [npos] of the frames, [nb] of the unions
  int32_t* status = (int32_t*)((char*)sums + sums_b);
  own.tab.reserve((size_t)nb);   // (the merges' tables stay where they are until the synchronisation)
  PccProfScope prof(ctx, "octree4_decode", points, nb, 0, 0);
  PCC_HIP(hipMemsetAsync(sums, 0, sums_b + stat_b, st));
  std::vector<char> keyed((size_t)npos, 0);
  int64_t body_at = 0;
  for (int f = 0; f < nb; ++f) {
    const O4Info& o = info[(size_t)f];
    const O4Plan& pl = plan[(size_t)f];
    int32_t* out = pts + 3 * h_point_offsets[f];
    if (rows[(size_t)f] == 0) continue;
    if (ver[(size_t)f] != 4) {   // an intra frame: version 2's decoder, to its place in the output
      int64_t offs2[2];
      const int rc = lod == 0 ? pcc_octree_decode_frames(ctx, h_blobs + f, h_lens + f, 1, out, nullptr, rows[(size_t)f], offs2)
                              : pcc_octree_decode_frames_lod(ctx, h_blobs + f, h_lens + f, 1, lod, out, nullptr, rows[(size_t)f], offs2);
      if (rc != PCC_OK) {
        const std::string m = pcc_last_error();
        pcc_set_error("%s: frame %d: %s", who, f, m.c_str());
        return rc;
      }
      continue;
    }
    const int p = n_refs + f, W = o.window;
    auto keys_of = [&](int q) { return (uint64_t*)(ring + (size_t)(q % max_w) * slot_b); };
    for (int q = p - W; q < p; ++q) {   // the keys of the window's frames, each formed once
      if (keyed[(size_t)q] || n_at(q) == 0) continue;
      const int32_t* src = q < n_refs ? d_refs[q] : pts + 3 * h_point_offsets[q - n_refs];
      hipLaunchKernelGGL(k_o4_keys, dim3(nblk(n_at(q), 256)), dim3(256), 0, st, src, n_at(q), lod, keys_of(q), sums + q, status + f);
      PCC_CHECK_LAUNCH();
      keyed[(size_t)q] = 1;
    }
    const uint64_t* ref_keys = keys_of(p - 1);
    const unsigned long long* ref_sum = sums + (p - 1);
    const uint32_t* ref_count = nullptr;
    int64_t rn = lod == 0 ? (int64_t)o.ref_n : n_at(p - 1);
    if (W > 1) {   // the union of the window: at lod 0 its size and its sum are compared on the device (status 16)
      O4MergeJob job;
      job.nl = W;
      job.out = merged;
      int64_t sum = 0;
      for (int i = 0; i < W; ++i) {
        job.list[i] = keys_of(p - W + i);
        job.n[i] = n_at(p - W + i);
        sum += job.n[i];
      }
      own.tab.emplace_back();
      uint32_t* d_count = nullptr;
      PCC_TRY(o4_merge_async(ctx, &job, 1, 0, merge_scratch, merge_b, &own.tab.back(), &d_count));
      if (lod == 0) {
        hipLaunchKernelGGL(k_o4_countcheck, dim3(1), dim3(1), 0, st, (const uint32_t*)d_count, o.ref_n, status + f);
        PCC_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_o4_keysum, dim3(nblk(rn, 256)), dim3(256), 0, st, (const uint64_t*)merged, rn, 0, 32768, sums + npos + f);
        PCC_CHECK_LAUNCH();
      } else {   // the union's size stays on the device: the search reads it there, below the room the union has
        ref_count = d_count;
        rn = sum;
      }
      ref_keys = merged;
      ref_sum = sums + npos + f;
    }
    const int64_t body_b = pl.bytes - o.off_p0;
    PCC_HIP(hipMemcpyAsync(d_bodies + body_at, h_blobs[f] + o.off_p0, (size_t)body_b, hipMemcpyHostToDevice, st));
    PCC_TRY(o4_decode_one(ctx, o, pl, d_bodies + body_at, ref_keys, rn, ref_count, ref_sum, out, status + f));
    body_at += o4_round(body_b, 16);
  }
  std::vector<int32_t> h_status((size_t)nb);
  PCC_HIP(hipMemcpyAsync(h_status.data(), status, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
  PCC_HIP(hipStreamSynchronize(st));
  for (int f = 0; f < nb; ++f) {
    const int32_t bad = h_status[(size_t)f];
    if (lod == 0)
      PCC_REQUIRE(!(bad & 32), PCC_E_ARG, "%s: frame %d: the reference is not a set of distinct int16 points in Morton order", who, f);
    else
      PCC_REQUIRE(!(bad & 32), PCC_E_ARG, "%s: frame %d: the reference is not a set of distinct cells of lod %d in Morton order", who, f, lod);
    PCC_REQUIRE(!(bad & 16), PCC_E_ARG, "%s: frame %d: the reference differs from the one the blob was coded against (ref_sum)", who, f);
    PCC_REQUIRE(bad == 0, PCC_E_STREAM, "%s: frame %d: octree blob v4: corrupt stream (status %d: 1 = words, 2 = empty node, 8 = counts)",
                who, f, bad);
  }
  if (h_points) {
    PCC_HIP(hipMemcpyAsync(h_points, pts, (size_t)points * 12, hipMemcpyDeviceToHost, st));
    PCC_HIP(hipStreamSynchronize(st));
  }
  return PCC_OK;
}

extern "C" int pcc_octree_decode_frames_refs(pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                                             const int32_t* const* d_ref_points, const int64_t* n_ref, int n_refs, int32_t* d_points,
                                             int32_t* h_points, int64_t cap_points, int64_t* h_point_offsets) {
  const char* who = "pcc_octree_decode_frames_refs";
  PCC_REQUIRE(ctx && h_blobs && h_lens && h_point_offsets && n_frames >= 1 && n_frames <= 65535 && n_refs >= 0 &&
                  n_refs <= kO4MaxWindow && (n_refs == 0 || (d_ref_points && n_ref)),
              PCC_E_ARG, "%s: bad argument (n_frames=%d n_refs=%d)", who, n_frames, n_refs);
  for (int r = 0; r < n_refs; ++r)
    PCC_REQUIRE(n_ref[r] >= 0 && n_ref[r] < ((int64_t)1 << 27) && (n_ref[r] == 0 || d_ref_points[r]), PCC_E_ARG,
                "%s: bad argument (reference %d: n_ref=%lld)", who, r, (long long)n_ref[r]);
  return o4_decode_frames(who, ctx, h_blobs, h_lens, n_frames, d_ref_points, n_ref, n_refs, 0, d_points, h_points, cap_points,
                          h_point_offsets);
}

// _decode_frames_refs at a level of detail: the references are CELLS at that lod (include/pcc.h has the rule)
extern "C" int pcc_octree_decode_frames_refs_lod(pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                                                 const int32_t* const* d_ref_cells, const int64_t* n_ref, int n_refs, int lod,
                                                 int32_t* d_points, int32_t* h_points, int64_t cap_points, int64_t* h_point_offsets) {
  const char* who = "pcc_octree_decode_frames_refs_lod";
  PCC_REQUIRE(ctx && h_blobs && h_lens && h_point_offsets && n_frames >= 1 && n_frames <= 65535 && n_refs >= 0 &&
                  n_refs <= kO4MaxWindow && (n_refs == 0 || (d_ref_cells && n_ref)),
              PCC_E_ARG, "%s: bad argument (n_frames=%d n_refs=%d)", who, n_frames, n_refs);
  PCC_REQUIRE(lod >= 0 && lod <= kO2MaxLod, PCC_E_ARG, "%s: level of detail %d outside 0 .. %d", who, lod, kO2MaxLod);
  for (int r = 0; r < n_refs; ++r)
    PCC_REQUIRE(n_ref[r] >= 0 && n_ref[r] < ((int64_t)1 << 27) && (n_ref[r] == 0 || d_ref_cells[r]), PCC_E_ARG,
                "%s: bad argument (reference %d: n_ref=%lld)", who, r, (long long)n_ref[r]);
  return o4_decode_frames(who, ctx, h_blobs, h_lens, n_frames, d_ref_cells, n_ref, n_refs, lod, d_points, h_points, cap_points,
                          h_point_offsets);
}

extern "C" int pcc_octree_decode_frames_ref(pcc_ctx* ctx, const uint8_t* const* h_blobs, const int64_t* h_lens, int n_frames,
                                            const int32_t* d_ref_points, int64_t n_ref, int32_t* d_points, int32_t* h_points,
                                            int64_t cap_points, int64_t* h_point_offsets) {
  const char* who = "pcc_octree_decode_frames_ref";
  PCC_REQUIRE(ctx && h_blobs && h_lens && h_point_offsets && n_frames >= 1 && n_frames <= 65535 && n_ref >= 0 &&
                  n_ref < ((int64_t)1 << 27) && (n_ref == 0 || d_ref_points),
              PCC_E_ARG, "%s: bad argument (n_frames=%d n_ref=%lld)", who, n_frames, (long long)n_ref);
  return o4_decode_frames(who, ctx, h_blobs, h_lens, n_frames, &d_ref_points, &n_ref, n_ref > 0 ? 1 : 0, 0, d_points, h_points,
                          cap_points, h_point_offsets);
}

// host only: what the head of a geometry blob of version 2 or 4 says
extern "C" int pcc_octree_inter_info(const uint8_t* h_in, int64_t len, int* version, int64_t* points, int* predicted,
                                     int64_t* ref_points) {
  if (!h_in || len < kO4Header || h_in[0] != 'O' || (h_in[1] != 2 && h_in[1] != 4)) {
    pcc_set_error("pcc_octree_inter_info: not an octree blob of version 2 or 4 (len=%lld)", (long long)len);
    return PCC_E_STREAM;
  }
  int64_t n = 0, rn = 0;
  if (h_in[1] == 2) {
    O2Info o;
    O2Plan pl;
    PCC_TRY(o2_parse(h_in, len, 0, true, &o, &pl));
    n = o.n;
  } else {
    // the whole blob, or exactly the prefix that pcc_octree_lod_info names for some level of detail
    O4Info o;
    O4Plan pl;
    const int64_t blob = kO4Header + (int64_t)o4_u32(h_in + 20);
    bool prefix = false;
    for (int k = 1; k <= kO2MaxLod && !prefix && len < blob; ++k)
      prefix = o4_parse_lod(h_in, len, k, true, &o, &pl) == PCC_OK && pl.bytes == len;
    if (!prefix) PCC_TRY(o4_parse(h_in, len, &o));
    n = o.n;
    rn = (int64_t)o.ref_n;
  }
  if (version) *version = h_in[1];
  if (points) *points = n;
  if (predicted) *predicted = h_in[1] == 4 ? 1 : 0;
  if (ref_points) *ref_points = rn;
  return PCC_OK;
}
