// Binary erosion / dilation / inner boundary of byte masks, and the boundary IoU matrix (include/prn.h: prn_morph*, prn_boundary_iou*;
// DESIGN.md section 18).
//
// Semantics (all integer, all exact).  The structuring element is the full (2r+1) x (2r+1) square (Chebyshev distance r = r iterations of
// the 3 x 3 all-ones element); pixels outside the image have the value `border`:
//   erode    a pixel is set iff every pixel of the square round it is set     (scipy.ndimage.binary_erosion, border_value = border)
//   dilate   a pixel is set iff any pixel of the square is set = ~erode(~m, r, 1 - border): the same code on complemented words
//   boundary m & ~erode(m, r, border = 0): the inner band of Boundary IoU (Cheng et al., CVPR 2021); the image edge counts as background
//
// A mask is worked on packed, one bit per pixel, every ROW starting on a 64-bit word (wpr = ceil(W / 64) words per row; bit i of word j of a
// row is column 64 j + i), so that rows shift independently and the column pass is a word-wise AND.  The square is separable:
//   pack     one thread per word: 64 mask bytes -> 64 bits, four groups of 16 inside the row (prn_masks.h).  Pad bits of a row's last word are 0.
//   row      one thread per word: R[y][x] = AND of the bits x-rx .. x+rx of row y, rx = min(r, W) (a window that long already covers the row
//            and both borders).  A window AND of length n <= 64 is taken on a 128-bit value by doubling (lengths 1, 2, 4, ... and one
//            overlapping step to n); a longer one is the AND of such 64-windows, 64 bits apart, plus one that ends at the window's end.  The
//            bits come from a funnel over two neighbouring words; left of column 0, right of column W-1 and in the pad bits they are `border`.
//   column   out[y] = AND of R[y-ry .. y+ry], ry = min(r, H); rows outside the image are all-`border`.  A workgroup owns 64 rows x 4 words;
//            for ry <= 32 it holds the rows and their halo in LDS (at most 128 x 4 words, twice: 8 KB, whatever the sizes) and doubles there;
//            beyond that every thread walks its column of R in the workspace (through L2; at most H steps).  The same launch complements
//            (dilate), takes the band (boundary), clears the pad bits, counts the set bits (wave sum, one integer atomic per wave) and writes
//            bytes (prn_morph) or leaves the words packed (prn_boundary_iou).
//   pairs    prn_boundary_iou: one workgroup per (a, b): two popcount sums (mask words, band words), fp32 quotients in the operation order of
//            prn_pairwise_iou's kernel.
// No workgroup waits for another, every loop is bounded by the sizes, the only atomics are integer adds: results are identical run to run and
// between a batched call and per-image calls.
#include "prn_masks.h"

namespace {

typedef unsigned long long u64;

constexpr int MO_ROWS = 64, MO_COLS = 4, MO_CSHIFT = 2;       // rows x words of a column-pass tile (PRN_MORPH_TILE_ROWS / _WORDS): 256 threads
constexpr int MO_HALO = 32;                      // the largest ry the LDS form takes (PRN_MORPH_LDS_RADIUS)
constexpr int MO_LROWS = MO_ROWS + 2 * MO_HALO;
static_assert(PRN_MORPH_TILE_ROWS == MO_ROWS && PRN_MORPH_TILE_WORDS == MO_COLS && PRN_MORPH_LDS_RADIUS == MO_HALO, "include/prn.h names the tile");
static_assert(MO_ROWS * MO_COLS == 256 && (1 << MO_CSHIFT) == MO_COLS, "one thread per word of the tile");

inline int mo_wpr(int W) { return (W + 63) >> 6; }

// the bits that exist in word j of a row
__device__ __forceinline__ u64 mo_valid(int j, int wpr, int W) { return (j == wpr - 1 && (W & 63)) ? ((1ull << (W & 63)) - 1ull) : ~0ull; }

// ---- pack ----
__global__ __launch_bounds__(256) void morph_pack_kernel(prn_mask_src src, int H, int W, int wpr, u64* __restrict__ bits, unsigned* __restrict__ area) {
  const int n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;        // word of the mask: y * wpr + j
  u64 word = 0;
  if (i < (int64_t)H * wpr) {
    const int y = (int)(i / wpr), j = (int)(i - (int64_t)y * wpr);
    const unsigned char* row = prn_mask_ptr(src, n, (size_t)H * W) + (size_t)y * W;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int x = 64 * j + 16 * g;
      if (x >= W) break;
      word |= (u64)prn_mask_bits16(row + x, W - x) << (16 * g);
    }
    bits[(size_t)n * H * wpr + (size_t)i] = word;
  }
  if (area) {                                                       // (uniform: every lane of the wave takes the shuffles)
    const int cnt = wave_sum_i(__popcll(word));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(area + n, (unsigned)cnt);
  }
}

// ---- row pass ----
struct mo_row {
  const u64* w;      // the row's wpr packed words
  int wpr, W;
  u64 flip;          // all ones: work on the complement (dilate)
  u64 fill;          // all ones: the border value (in the domain worked in) is 1
};

__device__ __forceinline__ u64 mo_get(const mo_row& r, int64_t j) {
  if (j < 0 || j >= r.wpr) return r.fill;
  const u64 valid = mo_valid((int)j, r.wpr, r.W);
  return ((r.w[j] ^ r.flip) & valid) | (r.fill & ~valid);
}

// the 64 bits from bit position p of the bordered row (p may be negative or past the end)
__device__ __forceinline__ u64 mo_bits_at(const mo_row& r, int64_t p) {
  const int64_t q = p >> 6;                                         // floor
  const int s = (int)(p & 63);
  const u64 lo = mo_get(r, q);
  if (s == 0) return lo;
  return (lo >> s) | (mo_get(r, q + 1) << (64 - s));
}

// bit i = AND of the n bits from position p + i, 1 <= n <= 64: doubling on the 128 bits from p (bit i needs the bits up to i + n - 1 <= 126)
__device__ __forceinline__ u64 mo_window(const mo_row& r, int64_t p, int n) {
  u64 lo = mo_bits_at(r, p), hi = mo_bits_at(r, p + 64);
  int L = 1;
  while (2 * L <= n) {                                              // (at most six steps)
    lo &= (lo >> L) | (hi << (64 - L));
    hi &= hi >> L;
    L *= 2;
  }
  if (L < n) {
    const int s = n - L;                                            // 1 <= s < L <= 32
    lo &= (lo >> s) | (hi << (64 - s));
  }
  return lo;
}

__global__ __launch_bounds__(256) void morph_row_kernel(const u64* __restrict__ bits, u64* __restrict__ rows, int H, int W, int wpr, int rx, int flip, int fill) {
  const int n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * wpr) return;
  const int y = (int)(i / wpr), j = (int)(i - (int64_t)y * wpr);
  const size_t base = (size_t)n * H * wpr;
  const mo_row r = {bits + base + (size_t)y * wpr, wpr, W, flip ? ~0ull : 0ull, fill ? ~0ull : 0ull};
  const int64_t p = 64 * (int64_t)j - rx;
  const int64_t nwin = 2 * (int64_t)rx + 1;                         // (odd: never a multiple of 64)
  u64 acc;
  if (nwin <= 64) {
    acc = mo_window(r, p, (int)nwin);
  } else {
    acc = mo_window(r, p + nwin - 64, 64);
    for (int64_t k = 0; 64 * (k + 1) <= nwin; ++k) acc &= mo_window(r, p + 64 * k, 64);      // (at most (2 W + 1) / 64 steps)
  }
  rows[base + (size_t)i] = acc;
}

// ---- column pass, the operation's last step, the area and the output ----
enum { OP_ERODE = 0, OP_DILATE = 1, OP_BOUNDARY = 2 };

__global__ __launch_bounds__(256) void morph_col_kernel(const u64* __restrict__ rows, const u64* __restrict__ bits, int H, int W, int wpr, int ry, int op, int fill,
                                                        int tiles_x, unsigned char* __restrict__ out_bytes, u64* __restrict__ out_bits, int* __restrict__ area) {
  __shared__ u64 sm[2][MO_LROWS][MO_COLS];
  const int n = blockIdx.y;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int tx = threadIdx.x & (MO_COLS - 1), ty = threadIdx.x >> MO_CSHIFT;
  const int y0 = tile_y * MO_ROWS, j0 = tile_x * MO_COLS;
  const int y = y0 + ty, j = j0 + tx;
  const size_t base = (size_t)n * H * wpr;
  const u64 fillw = fill ? ~0ull : 0ull;
  const bool live = y < H && j < wpr;
  u64 res = fillw;
  if (ry <= MO_HALO) {                                              // (uniform over the launch: every thread meets every barrier)
    const int nrows = MO_ROWS + 2 * ry, nwin = 2 * ry + 1;
    for (int i = threadIdx.x; i < nrows * MO_COLS; i += 256) {
      const int k = i >> MO_CSHIFT, c = i & (MO_COLS - 1);
      const int yy = y0 - ry + k, jj = j0 + c;
      sm[0][k][c] = (yy >= 0 && yy < H && jj < wpr) ? rows[base + (size_t)yy * wpr + jj] : fillw;
    }
    __syncthreads();
    int cur = 0, L = 1;
    while (2 * L <= nwin) {                                         // sm[cur][k] = AND of the rows k .. k + L - 1 (at most six steps)
      for (int i = threadIdx.x; i < nrows * MO_COLS; i += 256) {
        const int k = i >> MO_CSHIFT, c = i & (MO_COLS - 1);
        sm[cur ^ 1][k][c] = (k + L < nrows) ? (sm[cur][k][c] & sm[cur][k + L][c]) : sm[cur][k][c];
      }
      __syncthreads();
      cur ^= 1;
      L *= 2;
    }
    res = sm[cur][ty][tx] & sm[cur][ty + nwin - L][tx];             // rows ty .. ty + 2 ry of the tile's window = y - ry .. y + ry
  } else if (live) {
    const int64_t a = (int64_t)y - ry, b = (int64_t)y + ry;
    if (!fill && (a < 0 || b >= H)) {
      res = 0;
    } else {
      const int lo = a < 0 ? 0 : (int)a, hi = b >= H ? H - 1 : (int)b;
      res = ~0ull;
      for (int yy = lo; yy <= hi; ++yy) res &= rows[base + (size_t)yy * wpr + j];      // (at most H steps)
    }
  }
  int cnt = 0;
  if (live) {
    const u64 valid = mo_valid(j, wpr, W);
    if (op == OP_DILATE) res = ~res;
    res &= valid;
    if (op == OP_BOUNDARY) res = bits[base + (size_t)y * wpr + j] & ~res;
    cnt = __popcll(res);
    if (out_bits) out_bits[base + (size_t)y * wpr + j] = res;
    if (out_bytes) {
      unsigned char* o = out_bytes + ((size_t)n * H + y) * (size_t)W;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int x = 64 * j + 16 * g;
        if (x >= W) break;
        const unsigned b16 = (unsigned)(res >> (16 * g)) & 0xffffu;
        unsigned char* p = o + x;
        if (x + 16 <= W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
          uint4 q;
          unsigned* qq = reinterpret_cast<unsigned*>(&q);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const unsigned nib = (b16 >> (4 * k)) & 15u;
            qq[k] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
          }
          *reinterpret_cast<uint4*>(p) = q;
        } else {
          for (int k = 0; k < 16 && x + k < W; ++k) p[k] = (unsigned char)((b16 >> k) & 1u);
        }
      }
    }
  }
  if (area) {
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(area + n, cnt);
  }
}

// ---- pairs: mask IoU and boundary IoU of every (a, b) ----
__global__ __launch_bounds__(256) void boundary_pair_kernel(const u64* __restrict__ mask_a, const u64* __restrict__ mask_b, const u64* __restrict__ band_a,
                                                            const u64* __restrict__ band_b, const unsigned* __restrict__ marea_a,
                                                            const unsigned* __restrict__ marea_b, const unsigned* __restrict__ barea_a,
                                                            const unsigned* __restrict__ barea_b, float* __restrict__ mask_iou,
                                                            float* __restrict__ boundary_iou, int B, int64_t words) {
  const int a = blockIdx.y, b = blockIdx.x;
  const size_t oa = (size_t)a * words, ob = (size_t)b * words;
  int cm = 0, cb = 0;
  for (int64_t w = threadIdx.x; w < words; w += 256) {
    cm += __popcll(mask_a[oa + w] & mask_b[ob + w]);
    cb += __popcll(band_a[oa + w] & band_b[ob + w]);
  }
  cm = wave_sum_i(cm);
  cb = wave_sum_i(cb);
  __shared__ int sm[2][4];
  if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = cm; sm[1][threadIdx.x >> 6] = cb; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float im = (float)(sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3]);
    const float ib = (float)(sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3]);
    if (mask_iou) mask_iou[(size_t)a * B + b] = im / (((float)marea_a[a] + (float)marea_b[b]) - im);      // (integers < 2^24: exact sums)
    boundary_iou[(size_t)a * B + b] = ib / (((float)barea_a[a] + (float)barea_b[b]) - ib);                // (0 / 0 = NaN: an empty band is an empty mask)
  }
}

inline bool mo_sizes_ok(int64_t N, int H, int W, int radius) {
  return N > 0 && N <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) && radius >= 0;
}
inline size_t mo_words(int H, int W) { return (size_t)H * (size_t)mo_wpr(W); }

// pack, row and column launches over N masks (N <= 65535: the grid's y).  skip: the measurement aid of include/prn.h
int mo_engine(const char* who, const prn_mask_src& src, int N, int H, int W, int radius, int op, int border, u64* bits, u64* rows, unsigned* mask_area,
              unsigned char* out_bytes, u64* out_bits, int* out_area, hipStream_t st) {
  const int wpr = mo_wpr(W);
  const int64_t words = (int64_t)H * wpr;
  const int rx = radius < W ? radius : W, ry = radius < H ? radius : H;
  const int flip = op == OP_DILATE, fill = flip ? 1 - border : border;
  const int tiles_x = cdiv(wpr, MO_COLS), tiles_y = cdiv(H, MO_ROWS);
  if (!PRN_SKIPPED(1 << 25)) hipLaunchKernelGGL(morph_pack_kernel, dim3(cdiv(words, 256), N), dim3(256), 0, st, src, H, W, wpr, bits, mask_area);
  PRN_CHECK_LAUNCH(who);
  if (!PRN_SKIPPED(1 << 26)) hipLaunchKernelGGL(morph_row_kernel, dim3(cdiv(words, 256), N), dim3(256), 0, st, (const u64*)bits, rows, H, W, wpr, rx, flip, fill);
  PRN_CHECK_LAUNCH(who);
  if (!PRN_SKIPPED(1 << 27))
    hipLaunchKernelGGL(morph_col_kernel, dim3(tiles_x * tiles_y, N), dim3(256), 0, st, (const u64*)rows, (const u64*)bits, H, W, wpr, ry, op, fill, tiles_x, out_bytes,
                       out_bits, out_area);
  PRN_CHECK_LAUNCH(who);
  return 0;
}

}  // namespace

extern "C" int64_t prn_morph_ws_bytes(int Ntot, int H, int W, int radius) {
  if (!mo_sizes_ok(Ntot, H, W, radius)) return -1;
  return (int64_t)(2 * (size_t)Ntot * mo_words(H, W) * 8);
}

extern "C" int prn_morph(const unsigned char* const* masks_dev, const int* first_dev, int B, int Ntot, int H, int W, int op, int radius, int border,
                         unsigned char* out, int* area, void* ws, void* stream) {
  PRN_REQUIRE(masks_dev && first_dev && out && ws, "prn_morph: null pointer argument");
  PRN_REQUIRE(B >= 1 && H > 0 && W > 0 && Ntot > 0, "prn_morph: needs B >= 1, Ntot > 0, H > 0, W > 0 (got B=%d Ntot=%d H=%d W=%d)", B, Ntot, H, W);
  PRN_REQUIRE((int64_t)H * W < (1LL << 31), "prn_morph: needs H * W < 2^31 (got %d x %d)", H, W);
  PRN_REQUIRE(Ntot <= 65535, "prn_morph: needs Ntot <= 65535 masks per call (got %d)", Ntot);
  PRN_REQUIRE(op == OP_ERODE || op == OP_DILATE || op == OP_BOUNDARY, "prn_morph: op must be 0 (erode), 1 (dilate) or 2 (boundary) (got %d)", op);
  PRN_REQUIRE(radius >= 0, "prn_morph: radius must be >= 0 (got %d)", radius);
  PRN_REQUIRE(border == 0 || border == 1, "prn_morph: border must be 0 or 1 (got %d)", border);
  PRN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "prn_morph: ws must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (area) PRN_REQUIRE(hipMemsetAsync(area, 0, (size_t)Ntot * 4, st) == hipSuccess, "prn_morph: memset failed");
  u64* bits = (u64*)ws;
  u64* rows = bits + (size_t)Ntot * mo_words(H, W);
  const prn_mask_src src = {masks_dev, first_dev, B, nullptr};
  return mo_engine("prn_morph", src, Ntot, H, W, radius, op, op == OP_BOUNDARY ? 0 : border, bits, rows, nullptr, out, nullptr, area, st);
}

extern "C" int64_t prn_boundary_iou_ws_bytes(int A, int B, int H, int W) {
  if (A <= 0 || B <= 0 || A >= 65536 || B >= 65536 || H <= 0 || W <= 0 || (int64_t)H * W >= (1LL << 24)) return -1;
  return (int64_t)(prn_align256((size_t)(A + B) * 8) + 3 * (size_t)(A + B) * mo_words(H, W) * 8);
}

extern "C" int prn_boundary_iou(const unsigned char* masks_a, const unsigned char* masks_b, int A, int B, int H, int W, int radius, float* mask_iou,
                                float* boundary_iou, void* ws, void* stream) {
  PRN_REQUIRE(masks_a && masks_b && boundary_iou && ws, "prn_boundary_iou: null pointer argument (only mask_iou may be NULL)");
  PRN_REQUIRE(A > 0 && B > 0 && A < 65536 && B < 65536, "prn_boundary_iou: needs 1 <= A, B < 65536 (got %d, %d)", A, B);
  PRN_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1LL << 24), "prn_boundary_iou: needs H, W > 0 and H * W < 2^24 (fp32-exact areas; got %d x %d)", H, W);
  PRN_REQUIRE(radius >= 0, "prn_boundary_iou: radius must be >= 0 (got %d)", radius);
  PRN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "prn_boundary_iou: ws must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t words = mo_words(H, W), N = (size_t)A + B;
  unsigned* marea = (unsigned*)ws;                                  // [A + B] mask areas, then [A + B] band areas
  unsigned* barea = marea + N;
  u64* bits = (u64*)((char*)ws + prn_align256(N * 8));
  u64* rows = bits + N * words;
  u64* band = rows + N * words;
  PRN_REQUIRE(hipMemsetAsync(marea, 0, N * 8, st) == hipSuccess, "prn_boundary_iou: memset failed");
  const prn_mask_src sa = {nullptr, nullptr, 0, masks_a}, sb = {nullptr, nullptr, 0, masks_b};
  if (int rc = mo_engine("prn_boundary_iou/a", sa, A, H, W, radius, OP_BOUNDARY, 0, bits, rows, marea, nullptr, band, (int*)barea, st)) return rc;
  if (int rc = mo_engine("prn_boundary_iou/b", sb, B, H, W, radius, OP_BOUNDARY, 0, bits + A * words, rows + A * words, marea + A, nullptr, band + A * words,
                         (int*)barea + A, st))
    return rc;
  if (!PRN_SKIPPED(1 << 28))
    hipLaunchKernelGGL(boundary_pair_kernel, dim3(B, A), dim3(256), 0, st, (const u64*)bits, (const u64*)(bits + A * words), (const u64*)band,
                       (const u64*)(band + A * words), (const unsigned*)marea, (const unsigned*)(marea + A), (const unsigned*)barea, (const unsigned*)(barea + A),
                       mask_iou, boundary_iou, B, (int64_t)words);
  PRN_CHECK_LAUNCH("prn_boundary_iou/pairs");
  return 0;
}
