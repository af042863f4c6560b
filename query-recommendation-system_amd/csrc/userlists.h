// userlists.h -- what the kernels of the live user lists share (userlists.hip, userrows.hip): the reference's integer
// centring, the split of a row piece into scalar head, 16-byte vectors and scalar tail, and the list order as one word.
#pragma once
#include "idmap.h"

constexpr int UL_MAXK = 64;
typedef int32_t us_i32x4 __attribute__((ext_vector_type(4)));

// the reference's integer centring (users.hip, center_rows_kernel): zeros stay zero, float64 -> int truncates
__device__ static inline int32_t us_centre(int32_t x, double mean) { return x == 0 ? 0 : (int32_t)((double)x - mean); }

// the columns [0, len) of a row piece that starts at element p of the matrix: lanes below `head` and lanes 64 ..
// 64 + tail - 1 take the scalars before and behind the aligned middle, lane t its vectors t, t + 256, ...
struct UsPiece {
  int head, nvec, tail0, tail;
};
__device__ static inline UsPiece us_piece(int64_t elem0, int len) {
  UsPiece p;
  const int h = (int)((4 - (elem0 & 3)) & 3);
  p.head = h < len ? h : len;
  p.nvec = (len - p.head) >> 2;
  p.tail0 = p.head + 4 * p.nvec;
  p.tail = len - p.tail0;
  return p;
}

// list order as one unsigned word: larger = earlier (value descending, then id ascending); 0 = no entry (values are >= 1)
__device__ static inline uint64_t ul_key(int32_t milli, int64_t id) {
  return ((uint64_t)(uint32_t)milli << 32) | (uint32_t)(0x7FFFFFFF - (int32_t)id);
}
