// COCO run-length masks on the device (include/prn.h: prn_rle_*).  A mask [H][W] is walked column-major, p = x * H + y;
// its runs are what every COCO tool exchanges, as a delta-coded string of 6-bit characters.  The masks are N H W bytes in HBM and their strings a few
// kilobytes, so the coding runs where the masks are and only the strings travel.
//   encode  A run boundary sits at p exactly when m[y][x] differs from its column-major predecessor (m[y-1][x]; m[H-1][x-1] for y = 0; 0 for p = 0).
//           Boundaries are found row-major: adjacent lanes on adjacent columns (four columns per lane where W % 4 == 0; prn_masks.h reads them),
//           every lane walking down a segment of RLE_SEG rows with the pixel above carried in a register.  Only the RANK of a boundary needs the
//           column-major order; it comes from per-(mask, column, row segment) counts (launch 1) and an exclusive scan over them in (column,
//           segment) order (launch 2, one workgroup per mask).  Launch 3 repeats the walk and writes every boundary position at its rank.
//           The string: count i = E[i] - E[i-1] with E = the positions followed by H W; one thread per count forms the delta against count
//           i - 2, its character length, a scan of the lengths over the mask (one workgroup per mask, tiles of 256 counts with a carry) and
//           the characters.  Nothing is ordered by an atomic: there is none in this file.
//   decode  prn_rle_paint: out[n][y][x] = (number of run ends <= x * H + y) & 1.  A 128 x 8 tile needs only the ends between its lowest and
//           highest position; they are staged in LDS when they fit and searched there (binary search), else searched in place.
#include "prn_masks.h"

namespace {

constexpr int RLE_SEG = 32;                    // rows one lane walks
constexpr int RLE_LX = 64, RLE_LY = 4;         // lanes of a workgroup across columns (one wave: a row of a wave is one contiguous load) x row segments
constexpr int RLE_PW = 128, RLE_PH = 8;        // paint: pixels of one workgroup (32 lanes x 4 pixels wide, 8 rows)
constexpr int RLE_STAGE = 2048;                // paint: run ends of a tile that fit its LDS

// set bits of pixels (y, x .. x+CPL-1), bit k = column x + k; CPL == 4: x % 4 == 0 and the row holds all four
template <int CPL>
__device__ __forceinline__ unsigned row_bits(const unsigned char* __restrict__ m, int y, int x, int W) {
  return prn_mask_bits4(m + (size_t)y * W + x, CPL);
}

// The walk both encoder launches share: rows y0 .. y1-1 of columns x .. x+CPL-1, f(k, y) for every boundary at (y, x + k), top to bottom.
template <int CPL, class F>
__device__ __forceinline__ void rle_walk(const unsigned char* __restrict__ m, int H, int W, int x, int y0, int y1, F&& f) {
  unsigned prev;
  if (y0 > 0) {
    prev = row_bits<CPL>(m, y0 - 1, x, W);
  } else {                                                          // the predecessor of (0, x) is (H-1, x-1); of p = 0: a zero
    const unsigned left = x > 0 ? (m[(size_t)(H - 1) * W + x - 1] ? 1u : 0u) : 0u;
    prev = CPL == 1 ? left : (((row_bits<CPL>(m, H - 1, x, W) << 1) & 15u) | left);
  }
#pragma unroll 4
  for (int y = y0; y < y1; ++y) {
    const unsigned cur = row_bits<CPL>(m, y, x, W);
    const unsigned d = cur ^ prev;
    prev = cur;
    if (d) {
#pragma unroll
      for (int k = 0; k < CPL; ++k)
        if ((d >> k) & 1u) f(k, y);
    }
  }
}

// thread -> (instance n, first column x, row segment s); false: nothing to do
template <int CPL>
__device__ __forceinline__ bool rle_place(int W, int nseg, int colblocks, int& n, int& x, int& s) {
  n = blockIdx.x / colblocks;
  x = ((blockIdx.x - n * colblocks) * RLE_LX + threadIdx.x) * CPL;
  s = blockIdx.y * RLE_LY + threadIdx.y;
  return x < W && s < nseg;
}

// launch 1: cells[n][x * nseg + s] = boundaries of column x inside row segment s
template <int CPL>
__global__ __launch_bounds__(RLE_LX* RLE_LY) void rle_count_kernel(prn_mask_src src, int H, int W, int nseg, int colblocks,
                                                                   unsigned* __restrict__ cells) {
  int n, x, s;
  if (!rle_place<CPL>(W, nseg, colblocks, n, x, s)) return;
  const unsigned char* m = prn_mask_ptr(src, n, (size_t)H * W);
  unsigned c[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) c[k] = 0u;
  const int y0 = s * RLE_SEG, y1 = min(H, y0 + RLE_SEG);
  rle_walk<CPL>(m, H, W, x, y0, y1, [&](int k, int) { ++c[k]; });
  unsigned* o = cells + (size_t)n * W * nseg + (size_t)x * nseg + s;
#pragma unroll
  for (int k = 0; k < CPL; ++k) o[(size_t)k * nseg] = c[k];
}

// exclusive scan of v over the 256 threads of a workgroup (thread order), total = the sum; sm: 4 words
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned* sm, unsigned& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();                                                  // the previous tile's totals are no longer read
  if (lane == 63) sm[w] = incl;
  __syncthreads();
  unsigned base = 0u, tot = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned t = sm[i];
    if (i < w) base += t;
    tot += t;
  }
  total = tot;
  return base + incl - v;
}

// launch 2, one workgroup per mask: cells[n][.] <- its exclusive scan, totals[n] = boundaries of the mask
__global__ __launch_bounds__(256) void rle_scan_kernel(unsigned* __restrict__ cells, int ncell, int* __restrict__ totals) {
  __shared__ unsigned sm[4];
  unsigned* c = cells + (size_t)blockIdx.x * ncell;
  unsigned carry = 0u;
  for (int64_t i0 = 0; i0 < ncell; i0 += 256) {                      // (64-bit: ncell + 256 may pass 2^31)
    const int64_t i = i0 + threadIdx.x;
    const unsigned v = i < ncell ? c[i] : 0u;
    unsigned tot;
    const unsigned e = block_scan_excl(v, sm, tot);
    if (i < ncell) c[i] = carry + e;
    carry += tot;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = (int)carry;
}

// launch 3: the walk again, every boundary position to pos[pos_first[n] + rank]
template <int CPL>
__global__ __launch_bounds__(RLE_LX* RLE_LY) void rle_fill_kernel(prn_mask_src src, int H, int W, int nseg, int colblocks,
                                                                  const unsigned* __restrict__ cells, const int64_t* __restrict__ pos_first,
                                                                  unsigned* __restrict__ pos) {
  int n, x, s;
  if (!rle_place<CPL>(W, nseg, colblocks, n, x, s)) return;
  const unsigned char* m = prn_mask_ptr(src, n, (size_t)H * W);
  const unsigned* o = cells + (size_t)n * W * nseg + (size_t)x * nseg + s;
  const int64_t p0 = pos_first[n];
  const unsigned room = (unsigned)(pos_first[n + 1] - p0);          // a rank past the mask's own slots is never stored
  unsigned r[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) r[k] = o[(size_t)k * nseg];
  const int y0 = s * RLE_SEG, y1 = min(H, y0 + RLE_SEG);
  rle_walk<CPL>(m, H, W, x, y0, y1, [&](int k, int y) {
    const unsigned rank = r[k]++;
    if (rank < room) pos[p0 + rank] = (unsigned)(x + k) * (unsigned)H + (unsigned)y;
  });
}

// the delta-coded value of count i of a mask with K boundaries (K + 1 counts): E[j] = pos[j] (j < K), H W (j = K), 0 (j < 0)
__device__ __forceinline__ int rle_delta(const unsigned* __restrict__ pos, int K, unsigned HW, int i) {
  auto E = [&](int j) -> unsigned { return j < 0 ? 0u : (j < K ? pos[j] : HW); };
  const unsigned e1 = E(i - 1);
  int x = (int)(E(i) - e1);
  if (i > 2) x -= (int)(E(i - 2) - E(i - 3));
  return x;
}

__device__ __forceinline__ unsigned rle_chars(int x, unsigned char* out) {      // the characters of one value (out == nullptr: their number only)
  unsigned n = 0u;
  bool more;
  do {
    unsigned c = (unsigned)x & 0x1fu;
    x >>= 5;                                                        // arithmetic
    more = (c & 0x10u) ? (x != -1) : (x != 0);
    if (more) c |= 0x20u;
    if (out) out[n] = (unsigned char)(c + 48u);
    ++n;
  } while (more);
  return n;
}

// one workgroup per mask.  WRITE == false: str_len[n] = characters of the mask's string.  WRITE == true: the characters, at str_first[n].
template <bool WRITE>
__global__ __launch_bounds__(256) void rle_string_kernel(const unsigned* __restrict__ pos, const int64_t* __restrict__ pos_first, unsigned HW,
                                                         int64_t* __restrict__ str_len, const int64_t* __restrict__ str_first, unsigned char* __restrict__ out) {
  __shared__ unsigned sm[4];
  const int n = blockIdx.x;
  const int64_t p0 = pos_first[n];
  const int K = (int)(pos_first[n + 1] - p0);
  const unsigned* ps = pos + p0;
  const int64_t room = WRITE ? str_first[n + 1] - str_first[n] : 0;
  unsigned char* o = WRITE ? out + str_first[n] : nullptr;
  int64_t carry = 0;
  for (int64_t i0 = 0; i0 <= K; i0 += 256) {                         // K + 1 counts
    const bool live = i0 + threadIdx.x <= K;
    const int x = live ? rle_delta(ps, K, HW, (int)(i0 + threadIdx.x)) : 0;
    const unsigned len = live ? rle_chars(x, nullptr) : 0u;
    unsigned tot;
    const unsigned e = block_scan_excl(len, sm, tot);
    if (WRITE && live && carry + e + len <= room) rle_chars(x, o + carry + e);
    carry += tot;
  }
  if (!WRITE && threadIdx.x == 0) str_len[n] = carry;
}

// the number of ends[lo .. hi) that are <= p (ends ascending)
__device__ __forceinline__ int ends_le(const unsigned* e, int lo, int hi, unsigned p) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void rle_paint_kernel(const unsigned* __restrict__ ends, const int64_t* __restrict__ end_first, int H, int W,
                                                        unsigned char* __restrict__ out) {
  __shared__ unsigned s_e[RLE_STAGE];
  __shared__ int s_j[2];
  const int n = blockIdx.z;
  const unsigned* e = ends + end_first[n];
  const int R = (int)(end_first[n + 1] - end_first[n]);
  const int x0 = blockIdx.x * RLE_PW, y0 = blockIdx.y * RLE_PH;
  const int xl = min(W, x0 + RLE_PW) - 1, yl = min(H, y0 + RLE_PH) - 1;       // the tile's last column and row inside the image
  if (threadIdx.x < 2)                                              // runs of the tile's lowest and highest position
    s_j[threadIdx.x] = ends_le(e, 0, R, threadIdx.x == 0 ? (unsigned)x0 * H + y0 : (unsigned)xl * H + yl);
  __syncthreads();
  const int j0 = s_j[0], j1 = s_j[1];
  const bool staged = j1 - j0 <= RLE_STAGE;
  if (staged)
    for (int j = threadIdx.x; j < j1 - j0; j += 256) s_e[j] = e[j0 + j];
  __syncthreads();
  const int x = x0 + (threadIdx.x & 31) * 4, y = y0 + (threadIdx.x >> 5);
  if (x >= W || y >= H) return;
  unsigned v = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (x + k >= W) break;
    const unsigned p = (unsigned)(x + k) * H + y;
    const int idx = staged ? j0 + ends_le(s_e, 0, j1 - j0, p) : ends_le(e, j0, j1, p);
    v |= (unsigned)(idx & 1) << (8 * k);
  }
  unsigned char* o = out + ((size_t)n * H + y) * W + x;
  if (WIDE) {
    *reinterpret_cast<unsigned*>(o) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < W) o[k] = (unsigned char)(v >> (8 * k));
  }
}

int rle_sizes_ok(const char* what, int Ntot, int H, int W) {
  PRN_REQUIRE(H > 0 && W > 0 && Ntot > 0, "%s: sizes must be positive (Ntot=%d H=%d W=%d)", what, Ntot, H, W);
  PRN_REQUIRE((int64_t)H * W < (1LL << 31), "%s: H * W = %lld does not index in 31 bits", what, (long long)((int64_t)H * W));
  return 0;
}

struct rle_grid { int nseg, colblocks, cpl; dim3 grid; };
int rle_plan(const char* what, int Ntot, int H, int W, rle_grid& g) {
  if (int rc = rle_sizes_ok(what, Ntot, H, W)) return rc;
  g.cpl = W % 4 == 0 ? 4 : 1;
  g.nseg = cdiv(H, RLE_SEG);
  g.colblocks = cdiv(W / g.cpl, RLE_LX);
  const int64_t gx = (int64_t)Ntot * g.colblocks;
  const int gy = cdiv(g.nseg, RLE_LY);
  PRN_REQUIRE(gx < (1LL << 31) && gy <= 65535, "%s: too many workgroups (Ntot=%d H=%d W=%d)", what, Ntot, H, W);
  g.grid = dim3((unsigned)gx, (unsigned)gy, 1);
  return 0;
}

}  // namespace

extern "C" {

int64_t prn_rle_ws_bytes(int Ntot, int H, int W) {
  if (Ntot <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (1LL << 31)) return -1;
  return (int64_t)Ntot * W * cdiv(H, RLE_SEG) * 4;
}

int prn_rle_count(const unsigned char* const* masks_dev, const int* first_dev, int B, int Ntot, int H, int W, void* ws, int* totals, void* stream) {
  rle_grid g;
  if (int rc = rle_plan("prn_rle_count", Ntot, H, W, g)) return rc;
  PRN_REQUIRE(B > 0 && masks_dev && first_dev && ws && totals, "prn_rle_count: null argument or B=%d", B);
  PRN_REQUIRE(((uintptr_t)ws & 3u) == 0, "prn_rle_count: the workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned* cells = (unsigned*)ws;
  const dim3 blk(RLE_LX, RLE_LY);
  const prn_mask_src src = {masks_dev, first_dev, B, nullptr};
  if (g.cpl == 4) rle_count_kernel<4><<<g.grid, blk, 0, st>>>(src, H, W, g.nseg, g.colblocks, cells);
  else rle_count_kernel<1><<<g.grid, blk, 0, st>>>(src, H, W, g.nseg, g.colblocks, cells);
  PRN_CHECK_LAUNCH("prn_rle_count (count)");
  rle_scan_kernel<<<Ntot, 256, 0, st>>>(cells, W * g.nseg, totals);
  PRN_CHECK_LAUNCH("prn_rle_count (scan)");
  return 0;
}

int prn_rle_fill(const unsigned char* const* masks_dev, const int* first_dev, int B, int Ntot, int H, int W, const void* ws, const int64_t* pos_first,
                 unsigned* pos, void* stream) {
  rle_grid g;
  if (int rc = rle_plan("prn_rle_fill", Ntot, H, W, g)) return rc;
  PRN_REQUIRE(B > 0 && masks_dev && first_dev && ws && pos_first && pos, "prn_rle_fill: null argument or B=%d", B);
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(RLE_LX, RLE_LY);
  const prn_mask_src src = {masks_dev, first_dev, B, nullptr};
  if (g.cpl == 4) rle_fill_kernel<4><<<g.grid, blk, 0, st>>>(src, H, W, g.nseg, g.colblocks, (const unsigned*)ws, pos_first, pos);
  else rle_fill_kernel<1><<<g.grid, blk, 0, st>>>(src, H, W, g.nseg, g.colblocks, (const unsigned*)ws, pos_first, pos);
  PRN_CHECK_LAUNCH("prn_rle_fill");
  return 0;
}

int prn_rle_string_lengths(const unsigned* pos, const int64_t* pos_first, int Ntot, int H, int W, int64_t* str_len, void* stream) {
  if (int rc = rle_sizes_ok("prn_rle_string_lengths", Ntot, H, W)) return rc;
  PRN_REQUIRE(pos && pos_first && str_len, "prn_rle_string_lengths: null argument");
  rle_string_kernel<false><<<Ntot, 256, 0, (hipStream_t)stream>>>(pos, pos_first, (unsigned)H * (unsigned)W, str_len, nullptr, nullptr);
  PRN_CHECK_LAUNCH("prn_rle_string_lengths");
  return 0;
}

int prn_rle_strings(const unsigned* pos, const int64_t* pos_first, const int64_t* str_first, int Ntot, int H, int W, unsigned char* out, void* stream) {
  if (int rc = rle_sizes_ok("prn_rle_strings", Ntot, H, W)) return rc;
  PRN_REQUIRE(pos && pos_first && str_first && out, "prn_rle_strings: null argument");
  rle_string_kernel<true><<<Ntot, 256, 0, (hipStream_t)stream>>>(pos, pos_first, (unsigned)H * (unsigned)W, nullptr, str_first, out);
  PRN_CHECK_LAUNCH("prn_rle_strings");
  return 0;
}

int prn_rle_paint(const unsigned* ends, const int64_t* end_first, int Ntot, int H, int W, unsigned char* out, void* stream) {
  if (int rc = rle_sizes_ok("prn_rle_paint", Ntot, H, W)) return rc;
  PRN_REQUIRE(ends && end_first && out, "prn_rle_paint: null argument");
  PRN_REQUIRE(Ntot <= 65535 && cdiv(H, RLE_PH) <= 65535, "prn_rle_paint: at most 65535 masks and %d rows per call (Ntot=%d H=%d)", 65535 * RLE_PH, Ntot, H);
  const dim3 grid(cdiv(W, RLE_PW), cdiv(H, RLE_PH), Ntot);
  if (W % 4 == 0 && ((uintptr_t)out & 3u) == 0) rle_paint_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(ends, end_first, H, W, out);
  else rle_paint_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(ends, end_first, H, W, out);
  PRN_CHECK_LAUNCH("prn_rle_paint");
  return 0;
}

}  // extern "C"
