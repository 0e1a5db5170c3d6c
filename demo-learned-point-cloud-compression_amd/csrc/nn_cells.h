// nn_cells.h — distances on the biased lattice of the Morton keys, shared by the 1-NN walk (nn.hip) and the k-NN walk
// (knn.hip): point to point, and point to the cell of edge 2^L that holds a point.
#pragma once
#include "common.h"

#define NN_KEY48 0xFFFFFFFFFFFFull

__host__ __device__ static inline uint32_t nn_sq(uint32_t a, uint32_t b) {
  const uint32_t d = a > b ? a - b : b - a;      // at most 65535: the square fits 32 bits
  return d * d;
}
// the gap between coordinate q and the cell of edge 2^L that holds coordinate c, squared
__host__ __device__ static inline uint32_t nn_gap_sq(uint32_t q, uint32_t c, int L) {
  const uint32_t lo = (c >> L) << L, hi = lo | ((1u << L) - 1u);
  const uint32_t g = q < lo ? lo - q : (q > hi ? q - hi : 0u);
  return g * g;
}
__host__ __device__ static inline uint64_t nn_d2(uint32_t qx, uint32_t qy, uint32_t qz, uint64_t k) {
  return (uint64_t)nn_sq(qx, pcc_compact3(k >> 2)) + nn_sq(qy, pcc_compact3(k >> 1)) + nn_sq(qz, pcc_compact3(k));
}
