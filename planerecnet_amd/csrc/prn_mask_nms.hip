// Greedy mask NMS (reference models/functions/nms.py:53-81) of a ragged batch on the device, three launches on the caller's stream.
//
// The reference walks the candidates of one image in descending score order; a candidate i that is still kept removes every later
// j of its label with union <= 0 or inter / union > thr, where inter = sum(mask_i * mask_j) and union = (sum_masks[i] + sum_masks[j])
// - inter in fp32 with the CALLER's sum_masks.  Which pairs WOULD suppress each other does not depend on the greedy order, so:
//
//   pack   every mask to one bit per pixel, WORD-MAJOR within its image: word w of candidate j of image b (first candidate s_b, n_b
//          candidates) sits at P[s_b * words + w * n_b + j].  A wave that puts one candidate per lane then loads word w of 64
//          neighbouring candidates as one coalesced 256-byte access.  The transposition goes through an LDS tile, so the byte reads
//          (64 threads over 2 KB of one mask, 32 bytes each: prn_masks.h) and the word writes (64 threads over 256 B of one word row) are both contiguous.
//   pairs  S[i][c], one 64-bit word per candidate i and block c of 64 columns: bit l = candidate j = 64 c + l is suppressed by i
//          (i < j < n_b, equal labels, the decision above).  One column per lane, the decision balloted into the word; a workgroup
//          takes 8 rows of one column block, its four waves a quarter of the mask words each, so a column word is loaded once for 8
//          rows.  Only c >= i / 64 exists (the rest of the matrix is below the diagonal): exactly those words are written, and the
//          sweep reads exactly those.
//   sweep  one workgroup per image.  Lane l of wave 0 holds word l of the removed set (64 lanes x 64 bits: the per-image limit of 4096).
//          Per block of 64 candidates the rows of S are staged in LDS (the next block's rows are already in flight in registers of all
//          four waves while wave 0 works); the 64 keep-or-not decisions inside a block depend only on the diagonal words, lane r holding
//          the one of row r: a chain of readlane / scalar steps without any memory access.  The surviving rows are then ORed into the
//          removed set from LDS.
#include "prn_masks.h"

namespace {
constexpr int MN_LIMIT = PRN_MASK_NMS_MAX;      // candidates per image: 64 lanes x 64 bits
constexpr int MN_ROWS = 8;                      // rows of S per workgroup of the pairs kernel

inline size_t mn_words(int64_t HW) { return (size_t)((HW + 31) / 32); }
// ws = the packed bits of all candidates | S.  Where S starts depends on the total number of candidates, which the entry point is not told:
// the kernels read it from the end of the segment table.
__device__ __forceinline__ size_t mn_s_offset(const int* __restrict__ seg, int n_img, int words) {
  return prn_align256((size_t)seg[n_img] * words * 4);
}

// grid (word tiles of 64, candidate tiles of 64, images)
__global__ __launch_bounds__(256) void mask_nms_pack_kernel(const unsigned char* __restrict__ masks, const int* __restrict__ seg, unsigned* __restrict__ bits,
                                                            int64_t HW, int words) {
  __shared__ unsigned tile[64][65];
  const int s = seg[blockIdx.z], nb = seg[blockIdx.z + 1] - s;
  const int m0 = blockIdx.y * 64, w0 = blockIdx.x * 64;
  if (m0 >= nb) return;                                       // (uniform: before any barrier)
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int e = threadIdx.x + 256 * q, ml = e >> 6, wl = e & 63;
    const int m = m0 + ml, w = w0 + wl;
    unsigned word = 0;
    if (m < nb && w < words) word = prn_mask_bits32(masks + (size_t)(s + m) * HW + (size_t)w * 32, HW - (int64_t)w * 32);
    tile[ml][wl] = word;
  }
  __syncthreads();
  unsigned* out = bits + (size_t)s * words;
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int e = threadIdx.x + 256 * q, wl = e >> 6, ml = e & 63;
    const int m = m0 + ml, w = w0 + wl;
    if (m < nb && w < words) out[(size_t)w * nb + m] = tile[ml][wl];
  }
}

// grid (groups of MN_ROWS rows, column blocks of 64, images); S: [N][wmax] 64-bit words
__global__ __launch_bounds__(256) void mask_nms_pairs_kernel(char* ws, const int64_t* __restrict__ labels, const float* __restrict__ sums,
                                                             const int* __restrict__ seg, int n_img, int words, int wmax, float thr) {
  __shared__ int part[4][MN_ROWS][64];
  const unsigned* bits = reinterpret_cast<const unsigned*>(ws);
  unsigned long long* S = reinterpret_cast<unsigned long long*>(ws + mn_s_offset(seg, n_img, words));
  const int s = seg[blockIdx.z], nb = seg[blockIdx.z + 1] - s;
  const int i0 = blockIdx.x * MN_ROWS, c = blockIdx.y;
  if (i0 >= nb || c * 64 >= nb || c < (i0 >> 6)) return;      // (uniform; a group of 8 rows lies in one block of 64: all of its rows need this word or none)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = c * 64 + lane;
  const bool col = j < nb;
  const int jc = col ? j : nb - 1;                            // lanes past the last column: its word, masked off (an unconditional load: the unrolled
  const unsigned cmask = col ? ~0u : 0u;                      // loop then has all its loads in flight at once)
  const unsigned* P = bits + (size_t)s * words;
  int row[MN_ROWS];                                           // rows past the image's last: its last (loaded again, never stored)
#pragma unroll
  for (int r = 0; r < MN_ROWS; ++r) row[r] = i0 + r < nb ? i0 + r : nb - 1;
  int inter[MN_ROWS];
#pragma unroll
  for (int r = 0; r < MN_ROWS; ++r) inter[r] = 0;
#pragma unroll 4
  for (int w = wave; w < words; w += 4) {
    const unsigned* pw = P + (size_t)w * nb;
    const unsigned cw = pw[jc] & cmask;
#pragma unroll
    for (int r = 0; r < MN_ROWS; ++r) inter[r] += __popc(cw & pw[row[r]]);
  }
#pragma unroll
  for (int r = 0; r < MN_ROWS; ++r) part[wave][r][lane] = inter[r];
  __syncthreads();
  // wave v decides rows 2 v and 2 v + 1
#pragma unroll
  for (int rr = 0; rr < MN_ROWS / 4; ++rr) {
    const int r = wave * (MN_ROWS / 4) + rr, i = i0 + r;
    if (i >= nb) break;                                       // (uniform)
    const int cnt = part[0][r][lane] + part[1][r][lane] + part[2][r][lane] + part[3][r][lane];
    bool hit = false;
    if (col && j > i && labels[s + j] == labels[s + i]) {
#pragma clang fp contract(off)
      const float in_f = (float)cnt;                          // (an integer < 2^24: exact)
      const float pair = sums[s + i] + sums[s + j];
      const float uni = pair - in_f;
      hit = (uni <= 0.f) || (in_f / uni > thr);
    }
    const unsigned long long word = __ballot(hit);
    if (lane == 0) S[(size_t)(s + i) * wmax + c] = word;
  }
}

// one workgroup per image
__global__ __launch_bounds__(256) void mask_nms_sweep_kernel(const char* __restrict__ ws, const int* __restrict__ seg, int n_img, unsigned char* __restrict__ keep,
                                                             int words, int wmax) {
  const unsigned long long* S = reinterpret_cast<const unsigned long long*>(ws + mn_s_offset(seg, n_img, words));
  __shared__ unsigned long long rows[64][64];                 // rows[r][c - k]: word c of row 64 k + r, c >= k
  __shared__ unsigned long long gone[64];
  const int s = seg[blockIdx.x], nb = seg[blockIdx.x + 1] - s;
  if (nb <= 0) return;
  const int W = (nb + 63) >> 6;                               // words of the removed set = blocks of 64 candidates
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned long long next[16];
  // block k's words into registers: element e = (r, c - k), 64 consecutive threads on 64 consecutive words of one row; what the pairs
  // kernel did not write (rows past the image's last, words past W) is not read and counts as 0
  auto fetch = [&](int k) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = (threadIdx.x >> 6) + 4 * q, cc = k + lane, i = 64 * k + r;
      next[q] = (i < nb && cc < W) ? S[(size_t)(s + i) * wmax + cc] : 0ull;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < 16; ++q) rows[(threadIdx.x >> 6) + 4 * q][lane] = next[q];
  };
  fetch(0);
  stage();
  __syncthreads();
  unsigned long long removed = 0;                             // wave 0, lane l: word l
  for (int k = 0; k < W; ++k) {
    if (k + 1 < W) fetch(k + 1);                              // in flight while wave 0 works on block k
    if (wave == 0) {
      const unsigned long long mine = __shfl(removed, k, 64);
      unsigned klo = __builtin_amdgcn_readfirstlane((unsigned)mine), khi = __builtin_amdgcn_readfirstlane((unsigned)(mine >> 32));
      unsigned long long kw = ((unsigned long long)khi << 32) | klo;      // removed candidates of this block so far (uniform)
      const unsigned long long diag = rows[lane][0];          // lane r: which later candidates of the block row r suppresses
      const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
#pragma unroll
      for (int r = 0; r < 64; ++r) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)dlo, r), hi = (unsigned)__builtin_amdgcn_readlane((int)dhi, r);      // (the builtin
        const unsigned long long d = ((unsigned long long)hi << 32) | lo;                                // returns int: no sign extension into the high word)
        kw |= ((kw >> r) & 1ull) ? 0ull : d;                  // a removed candidate suppresses nobody
      }
      // the block's survivors remove what their rows say, in every later word too (lane l: word l = column l - k of the staged rows)
      const unsigned long long kept = ~kw;                    // (rows past the image's last are staged as 0)
      const int cc = lane >= k ? lane - k : 0;
      unsigned long long acc = 0;
#pragma unroll 8
      for (int r = 0; r < 64; ++r) acc |= rows[r][cc] & (0ull - ((kept >> r) & 1ull));
      if (lane >= k && lane < W) removed |= acc;
    }
    __syncthreads();
    if (k + 1 < W) {
      stage();
      __syncthreads();
    }
  }
  if (wave == 0) gone[lane] = removed;
  __syncthreads();
  for (int j = threadIdx.x; j < nb; j += 256) keep[s + j] = (unsigned char)(((gone[j >> 6] >> (j & 63)) & 1ull) ? 0 : 1);
}

}  // namespace

extern "C" int64_t prn_mask_nms_ws_bytes(int n_total, int n_max, int64_t HW) {
  if (n_total <= 0 || n_max <= 0 || HW <= 0) return 256;
  return (int64_t)(prn_align256((size_t)n_total * mn_words(HW) * 4) + (size_t)n_total * (size_t)((n_max + 63) / 64) * 8);
}

extern "C" int prn_mask_nms(const unsigned char* masks, const int64_t* labels, const float* sum_masks, const int* seg, int n_img, int n_max, int64_t HW, float thr,
                            unsigned char* keep, void* ws, void* stream) {
  PRN_REQUIRE(masks && labels && sum_masks && seg && keep && ws, "prn_mask_nms: null pointer argument");
  PRN_REQUIRE(n_img >= 1 && n_img <= 65535, "prn_mask_nms: needs 1 <= n_img <= 65535 (got %d)", n_img);
  PRN_REQUIRE(n_max >= 1 && n_max <= MN_LIMIT, "prn_mask_nms: needs 1 <= n_max <= %d candidates per image (got %d)", MN_LIMIT, n_max);
  PRN_REQUIRE(HW > 0 && HW < (1LL << 24), "prn_mask_nms: needs 0 < H*W < 2^24 (fp32-exact intersections)");
  PRN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "prn_mask_nms: ws must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int words = (int)mn_words(HW), wmax = (n_max + 63) / 64, tiles = (n_max + 63) / 64;
  // (PRN_SKIPPED: the measurement aid of include/prn.h -- tools/mask_nms_bench.py times each stage alone on buffers a full call left)
  if (!PRN_SKIPPED(1 << 16)) hipLaunchKernelGGL(mask_nms_pack_kernel, dim3(cdiv(words, 64), tiles, n_img), dim3(256), 0, st, masks, seg, (unsigned*)ws, HW, words);
  PRN_CHECK_LAUNCH("prn_mask_nms/pack");
  if (!PRN_SKIPPED(1 << 17))
    hipLaunchKernelGGL(mask_nms_pairs_kernel, dim3(cdiv(n_max, MN_ROWS), tiles, n_img), dim3(256), 0, st, (char*)ws, labels, sum_masks, seg, n_img, words, wmax, thr);
  PRN_CHECK_LAUNCH("prn_mask_nms/pairs");
  if (!PRN_SKIPPED(1 << 18)) hipLaunchKernelGGL(mask_nms_sweep_kernel, dim3(n_img), dim3(256), 0, st, (const char*)ws, seg, n_img, keep, words, wmax);
  PRN_CHECK_LAUNCH("prn_mask_nms/sweep");
  return 0;
}
