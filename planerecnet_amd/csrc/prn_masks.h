// Reading byte masks: the one layer under every kernel that takes [H][W] uint8 masks, non-zero = set.
// What differs between the operators is the bit LAYOUT they build (flat 32-bit words for IoU, word-major words for NMS, row-aligned 64-bit
// words for morphology, none for CCL and RLE); how the bytes are read, and which mask of a ragged batch is read, is stated here once.
#pragma once
#include "prn_common.h"

// one bit per non-zero byte of v (bits 0..3)
__device__ __forceinline__ unsigned prn_nz4(unsigned v) {
  v |= v >> 4; v |= v >> 2; v |= v >> 1;
  v &= 0x01010101u;
  return (v & 1u) | ((v >> 7) & 2u) | ((v >> 14) & 4u) | ((v >> 21) & 8u);
}

// prn_mask_bits4 / 16 / 32 (p, avail): bit k = (p[k] != 0) for k < min(avail, width), higher bits 0; avail <= 0 reads nothing.
// THE RULE -- the one place where a mask kernel could read out of bounds: a byte at or past p + avail is never read, and a vector load (4 or
// 16 bytes) is issued only when its whole group is available AND its address is aligned to the load size; anything else is read as single
// bytes.  (An odd H * W puts every second mask of a tensor on an odd address, a sliced view any mask; W % 4 != 0 every second row.  The vector
// case is the usual one and is laid out first.)
__device__ __forceinline__ unsigned prn_mask_bits4(const unsigned char* __restrict__ p, int64_t avail) {
  if (__builtin_expect(avail >= 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0, 1)) return prn_nz4(*reinterpret_cast<const unsigned*>(p));
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < avail && p[k]) bits |= 1u << k;
  return bits;
}

__device__ __forceinline__ unsigned prn_nz16(uint4 v) { return prn_nz4(v.x) | (prn_nz4(v.y) << 4) | (prn_nz4(v.z) << 8) | (prn_nz4(v.w) << 12); }

__device__ __forceinline__ unsigned prn_mask_bits16(const unsigned char* __restrict__ p, int64_t avail) {
  if (__builtin_expect(avail >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0, 1)) return prn_nz16(*reinterpret_cast<const uint4*>(p));
  unsigned bits = 0;
#pragma clang loop unroll(disable)                                  // (the rare path: kept small, it sits inside the packers' unrolled loops)
  for (int k = 0; k < 16 && k < avail; ++k) bits |= p[k] ? (1u << k) : 0u;
  return bits;
}

// the 16-byte groups of N masks `stride` bytes apart (a thread that walks the masks of an image over its own pixels; stride < 0 walks down):
// where every group takes its vector load -- p and the stride both multiples of 16 -- the N loads are issued before the first is tested: one
// round trip for all of them, where a walk that tests a mask before it loads the next is a chain of N.  Anything else: group by group.
template <int N>
__device__ __forceinline__ void prn_mask_bits16_each(const unsigned char* p, int64_t stride, int64_t avail, unsigned (&bits)[N]) {
  if (__builtin_expect(avail >= 16 && ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)stride) & 15) == 0, 1)) {
    uint4 v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = *reinterpret_cast<const uint4*>(p + k * stride);
#pragma unroll
    for (int k = 0; k < N; ++k) bits[k] = prn_nz16(v[k]);
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) bits[k] = prn_mask_bits16(p + k * stride, avail);
  }
}

// two 16-byte groups, each under the rule on its own (p + 16 is aligned exactly when p is); where both take their vector load, the two loads
// are issued together
__device__ __forceinline__ unsigned prn_mask_bits32(const unsigned char* __restrict__ p, int64_t avail) {
  if (__builtin_expect(avail >= 32 && (reinterpret_cast<uintptr_t>(p) & 15) == 0, 1)) {
    const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
    return prn_nz16(lo) | (prn_nz16(hi) << 16);
  }
  return prn_mask_bits16(p, avail) | (prn_mask_bits16(p + 16, avail - 16) << 16);
}

// Where the masks of a launch come from: the caller's ragged batch -- masks[b] = the first mask of image b, which holds the global masks
// first[b] .. first[b+1]-1 -- or (flat != NULL) [N][H][W] bytes back to back.
struct prn_mask_src {
  const unsigned char* const* masks;
  const int* first;
  int B;
  const unsigned char* flat;
};

__device__ __forceinline__ const unsigned char* prn_mask_ptr(const prn_mask_src& s, int n, size_t HW) {
  if (s.flat) return s.flat + (size_t)n * HW;
  int lo = 0, hi = s.B - 1;
  while (lo < hi) {                                                 // the last b with first[b] <= n (empty images are skipped)
    const int mid = (lo + hi + 1) >> 1;
    if (s.first[mid] <= n) lo = mid; else hi = mid - 1;
  }
  return s.masks[lo] + (size_t)(n - s.first[lo]) * HW;
}
