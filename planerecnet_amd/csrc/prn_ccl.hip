// Connected components of byte masks on the device (include/prn.h: prn_ccl_*).
//
// Semantics (all integer, all exact).  A mask is [H][W] bytes, non-zero = set; connectivity is 8 or 4.  A component is a maximal set of set
// pixels connected under the connectivity; components are numbered 1..K in ascending order of their smallest row-major index y * W + x
// (scipy.ndimage.label with the full 3x3 structure for 8, the cross for 4).  prn_ccl_clean, per mask: the component of maximal area (a tie:
// the lowest label; nothing if its area < min_area) or every component of area >= min_area is kept; with fill_holes every unset pixel of THAT
// selection becomes set unless unset pixels connect it to an unset pixel on the image border under the DUAL connectivity (4 for 8, 8 for 4:
// scipy.ndimage.binary_fill_holes with the cross / the full structure).
//
// One engine: "label the pixels whose value is v under connectivity c, then keep components by a rule".  prn_ccl_label: v = set.  The selection
// of prn_ccl_clean: v = set, rule "largest" or "area >= min_area".  Its hole pass: the same launches on the selected mask with v = unset, the
// dual connectivity and the rule "touches the border"; the output is the complement of what was kept.
//
// The forest lives in ONE int32 word per pixel of the workspace, P[n][i], i = y * W + x:
//     -1                       the pixel does not have the value v
//     p, 0 <= p <= i           its parent (p == i: a root).  A parent is never larger than its child, so every chain descends.
//   after the flatten launch a root's word is reused (a root needs no parent: its index is its position):
//     i + (area - 1)           in bits 0..30 -- every other pixel of the component has a larger index, so the value stays below H * W, and a word
//                              whose low bits are >= its own index is a root, one whose low bits are < its index a child
//     bit 31                   the component has a pixel on the image border (H * W < 2^31 keeps bit 31 free, and i + area - 1 <= H * W - 1 <
//                              2^31 - 1 keeps a flagged root apart from -1)
//   and after the rank launch of prn_ccl_label a root's word is bit 31 | its label.
// Launches (each on the caller's stream; the launch boundary is the only ordering between workgroups -- no flags, tickets or spins):
//   local    a workgroup owns one (mask, 32 x 64 tile): union-find over the tile in LDS (decision tree over the N / W / NW / NE neighbours,
//            unions by LDS atomic min), then P = the global index of every pixel's tile-local root.  Mask bytes come four at a time (prn_masks.h).
//   seam     one thread per pixel on a tile's left column / top row: union with its neighbours across the seam.  Reads are relaxed agent-scope
//            atomic loads, writes atomic mins: the smaller index becomes the parent.  A stale parent is still a member of the same set at a
//            larger index, so staleness costs steps, never correctness.
//   flatten  every pixel follows its chain to the root, stores it, adds 1 to the root's word and ORs the border bit into it; runs of
//            neighbouring pixels with one root add their length once (a wave shuffle and a ballot), or a large component serialises on one word.
//   reduce   per (mask, 2048-pixel chunk): the number of roots (kept per chunk for the rank launch), the key (area << 32 | ~root) maximised
//            (= maximal area, lowest root on a tie), the kept / border sums of the rule; wave reductions first, one atomic per wave.
//   rank     prn_ccl_label only: a root's label = 1 + roots before it = the chunk counts before its chunk + a scan inside the chunk.
//   write    labels, or the kept mask and the statistics.
// Every loop is bounded by H * W: a find follows strictly decreasing indices; a union retries only with the value its own atomic min returned,
// which is smaller than the index it tried (the sum of the two indices falls with every retry).  All atomics are integer min / add / or / max:
// the forest's final roots (the smallest index of each component), the areas and therefore every output byte are independent of arrival order.
#include "prn_masks.h"

namespace {

constexpr int CC_TH = 32, CC_TW = 64;            // tile rows x columns (PRN_CCL_TILE_H / _W)
constexpr int CC_TPIX = CC_TH * CC_TW;
constexpr int CC_CHUNK = 2048;                   // pixels per workgroup of the reduce / rank launches: 256 threads x 8 consecutive pixels
constexpr int CC_FLAT = 1024;                   // pixels per workgroup of the flatten launch
constexpr int CC_ACC = 8;                        // int32 words of per-mask accumulators
constexpr int CC_NONE = -1;
constexpr int CC_LOW = 0x7fffffff;
constexpr unsigned CC_FLAG = 0x80000000u;
enum { ACC_KEY = 0 /* 64 bits */, ACC_COUNT = 2, ACC_KEPT = 3, ACC_KEPT_AREA = 4, ACC_BORDER_AREA = 5 };
enum { RULE_NONE = 0, RULE_LARGEST = 1, RULE_MIN_AREA = 2, RULE_BORDER = 3 };
static_assert(PRN_CCL_TILE_H == CC_TH && PRN_CCL_TILE_W == CC_TW, "include/prn.h names the tile");

inline size_t cc_align8(size_t v) { return (v + 7) & ~(size_t)7; }
inline int cc_chunks(int64_t HW) { return (int)((HW + CC_CHUNK - 1) / CC_CHUNK); }

// ---- the forest in LDS (one tile) ----
__device__ __forceinline__ int lds_load(const int* L, int x) { return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(const int* L, int x) {
  for (;;) {                                                        // (strictly decreasing: at most x steps)
    const int p = lds_load(L, x);
    if (p >= x) return x;
    x = p;
  }
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  for (;;) {                                                        // (a + b falls with every retry)
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;                                           // a was a root and now hangs below b
    a = old;                                                        // a had a parent old < a, which min(old, b) may have displaced: unite old and b
  }
}

// ---- the forest in global memory (one mask; several workgroups write the same words) ----
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// from a pixel that has the value v: the root's index.  Root words may carry an area and the border bit (flatten launch): low bits >= index.
__device__ __forceinline__ int g_find(const int* P, int x) {
  for (;;) {                                                        // (strictly decreasing: at most x steps)
    const int p = g_load(P + x) & CC_LOW;
    if (p >= x) return x;
    x = p;
  }
}
__device__ __forceinline__ void g_union(int* P, int a, int b) {     // seam launch only: words are plain parents there
  for (;;) {                                                        // (a + b falls with every retry)
    a = g_find(P, a);
    b = g_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

// launch 1: grid (tiles, masks)
__global__ __launch_bounds__(256) void ccl_local_kernel(prn_mask_src src, int H, int W, int tiles_x, int vset, int conn8, int* __restrict__ P) {
  __shared__ int L[CC_TPIX];
  const int n = blockIdx.y, t = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * CC_TH, tx0 = (blockIdx.x % tiles_x) * CC_TW;
  const size_t HW = (size_t)H * W;
  const unsigned char* m = prn_mask_ptr(src, n, HW);
  // stage: 512 groups of four pixels; pixels outside the image (never read) count as "not v"
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = t + 256 * k, ly = q >> 4, lx = (q & 15) * 4;
    const int y = ty0 + ly, x = tx0 + lx;
    unsigned bits = 0;
    if (y < H && x < W) {
      const int left = W - x;
      bits = prn_mask_bits4(m + (size_t)y * W + x, left);
      const unsigned inside = left >= 4 ? 15u : ((1u << left) - 1u);
      if (!vset) bits = ~bits & inside;
    }
    const int l0 = ly * CC_TW + lx;
#pragma unroll
    for (int j = 0; j < 4; ++j) L[l0 + j] = ((bits >> j) & 1u) ? l0 + j : CC_NONE;
  }
  __syncthreads();
  // unions with the neighbours above and to the left inside the tile (a word's sign never changes: "has the value v" is stable)
  const int lx = t & 63;
#pragma unroll 2
  for (int k = 0; k < CC_TH / 4; ++k) {
    const int ly = (t >> 6) + 4 * k, p = ly * CC_TW + lx;
    if (lds_load(L, p) < 0) continue;
    const bool up = ly > 0, lf = lx > 0, rt = lx < CC_TW - 1;
    const bool north = up && lds_load(L, p - CC_TW) >= 0;
    if (conn8) {
      // north set: W, NW and NE are its neighbours and meet it through their own unions (induction over the rows)
      if (north) {
        lds_union(L, p, p - CC_TW);
      } else {
        if (lf && lds_load(L, p - 1) >= 0) lds_union(L, p, p - 1);                       // (west set: NW is west's north)
        else if (up && lf && lds_load(L, p - CC_TW - 1) >= 0) lds_union(L, p, p - CC_TW - 1);
        if (up && rt && lds_load(L, p - CC_TW + 1) >= 0) lds_union(L, p, p - CC_TW + 1);
      }
    } else {
      if (north) lds_union(L, p, p - CC_TW);
      if (lf && lds_load(L, p - 1) >= 0) lds_union(L, p, p - 1);
    }
  }
  __syncthreads();
  int* Pm = P + (size_t)n * HW;
#pragma unroll 2
  for (int k = 0; k < CC_TH / 4; ++k) {
    const int ly = (t >> 6) + 4 * k, p = ly * CC_TW + lx;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    int out = CC_NONE;
    if (lds_load(L, p) >= 0) {
      const int r = lds_find(L, p);                                 // tile order = image order inside a tile: the root is the component's first pixel
      out = (ty0 + (r >> 6)) * W + tx0 + (r & 63);
    }
    Pm[(size_t)y * W + x] = out;
  }
}

// launch 2: grid (seam pixels / 256, masks).  Left-column pixels of the tile columns 1.., then top-row pixels of the tile rows 1..
__global__ __launch_bounds__(256) void ccl_seam_kernel(int* __restrict__ P, int H, int W, int nvs, int nseam, int conn8) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nseam) return;
  int* Pm = P + (size_t)blockIdx.y * ((size_t)H * W);
  int y, x;
  const bool vert = idx < nvs * H;
  if (vert) {
    x = (idx / H + 1) * CC_TW; y = idx % H;
  } else {
    const int j = idx - nvs * H;
    y = (j / W + 1) * CC_TH; x = j % W;
  }
  const int i = y * W + x;
  if (g_load(Pm + i) < 0) return;
  auto join = [&](int qy, int qx) {
    if (qy < 0 || qy >= H || qx < 0 || qx >= W) return;
    const int q = qy * W + qx;
    if (g_load(Pm + q) < 0) return;
    g_union(Pm, i, q);
  };
  // every pair of neighbours in different tiles has a member in a left column whose partner is W / NW / SW of it, or in a top row with N / NW / NE
  if (vert) {
    join(y, x - 1);
    if (conn8) { join(y - 1, x - 1); join(y + 1, x - 1); }
  } else {
    join(y - 1, x);
    if (conn8) { join(y - 1, x - 1); join(y - 1, x + 1); }
  }
}

// launch 3: grid (pixels / 1024, masks); a thread takes four pixels 256 apart (a wave: 64 consecutive pixels at a time)
__global__ __launch_bounds__(256) void ccl_flatten_kernel(int* __restrict__ P, int H, int W, int border) {
  const int64_t HW = (int64_t)H * W, b0 = (int64_t)blockIdx.x * CC_FLAT + threadIdx.x;
  int* Pm = P + (size_t)blockIdx.y * (size_t)HW;
  const int lane = threadIdx.x & 63;
  int pend_r = -1, pend_c = 0;                                      // additions to one root collected over the thread's pixels
#pragma unroll
  for (int k = 0; k < CC_FLAT / 256; ++k) {
    const int64_t i64 = b0 + 256 * k;
    int key = -2 - lane;                                            // the root this pixel adds 1 to; negative and unlike its neighbours': none
    if (i64 < HW) {
      const int i = (int)i64, w = g_load(Pm + i);
      if (w != CC_NONE) {
        int r = i;
        if ((w & CC_LOW) < i) {                                     // a child (its word is written by this thread alone)
          r = g_find(Pm, w);
          if (r != w) __hip_atomic_store(Pm + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          key = r;
        }
        if (border) {
          const int y = i / W, x = i - y * W;
          if ((y == 0 || y == H - 1 || x == 0 || x == W - 1) && g_load(Pm + r) >= 0)      // (a stale "not yet" costs a redundant OR)
            __hip_atomic_fetch_or(reinterpret_cast<unsigned*>(Pm + r), CC_FLAG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    // Neighbouring pixels mostly share their root: the first lane of a run of equal roots adds the run's length (all 64 lanes arrive here).
    // A component of 10^5 pixels otherwise serialises 10^5 atomics on one word.
    const int prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    if (head && key >= 0) {
      const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
      const int len = above ? __ffsll(above) : 64 - lane;           // (the next run starts `len` lanes on)
      if (key == pend_r) {
        pend_c += len;
      } else {
        if (pend_c) __hip_atomic_fetch_add(Pm + pend_r, pend_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pend_r = key; pend_c = len;
      }
    }
  }
  if (pend_c) __hip_atomic_fetch_add(Pm + pend_r, pend_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool cc_is_root(int w, int i) { return w != CC_NONE && (w & CC_LOW) >= i; }

// launch 4: grid (chunks, masks)
__global__ __launch_bounds__(256) void ccl_reduce_kernel(const int* __restrict__ P, int64_t HW, int nchunk, int rule, int min_area, int* __restrict__ acc,
                                                         int* __restrict__ chunks) {
  __shared__ int part[4];
  const int n = blockIdx.y, c = blockIdx.x;
  const int* Pm = P + (size_t)n * (size_t)HW;
  const int64_t i0 = (int64_t)c * CC_CHUNK + threadIdx.x * 8;
  int cnt = 0, kept = 0, sum = 0;
  unsigned long long key = 0ull;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (i0 + j >= HW) break;
    const int i = (int)(i0 + j), w = Pm[i];
    if (!cc_is_root(w, i)) continue;
    const int area = (w & CC_LOW) - i + 1;
    ++cnt;
    const unsigned long long k = ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
    key = k > key ? k : key;
    if (rule == RULE_MIN_AREA && area >= min_area) { ++kept; sum += area; }
    if (rule == RULE_BORDER && w < 0) sum += area;
  }
  int* a = acc + (size_t)n * CC_ACC;
  const int wcnt = wave_sum_i(cnt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  const int lane = threadIdx.x & 63;
  if (rule == RULE_MIN_AREA || rule == RULE_BORDER) {
    kept = wave_sum_i(kept);
    sum = wave_sum_i(sum);
  }
  if (lane == 0) {
    part[threadIdx.x >> 6] = wcnt;
    if (wcnt) {
      atomicAdd(a + ACC_COUNT, wcnt);
      atomicMax(reinterpret_cast<unsigned long long*>(a + ACC_KEY), key);
      if (rule == RULE_MIN_AREA && kept) { atomicAdd(a + ACC_KEPT, kept); atomicAdd(a + ACC_KEPT_AREA, sum); }
      if (rule == RULE_BORDER && sum) atomicAdd(a + ACC_BORDER_AREA, sum);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) chunks[(size_t)n * nchunk + c] = part[0] + part[1] + part[2] + part[3];
}

// launch 5 (labels): grid (chunks, masks); a root's word becomes bit 31 | label
__global__ __launch_bounds__(256) void ccl_rank_kernel(int* __restrict__ P, int64_t HW, int nchunk, const int* __restrict__ chunks) {
  __shared__ int sm[8];
  const int n = blockIdx.y, c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* Pm = P + (size_t)n * (size_t)HW;
  int before = 0;
  for (int k = threadIdx.x; k < c; k += 256) before += chunks[(size_t)n * nchunk + k];
  before = wave_sum_i(before);
  const int64_t i0 = (int64_t)c * CC_CHUNK + threadIdx.x * 8;
  int w[8];
  unsigned roots = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    w[j] = CC_NONE;
    if (i0 + j < HW) w[j] = Pm[i0 + j];
    if (i0 + j < HW && cc_is_root(w[j], (int)(i0 + j))) roots |= 1u << j;
  }
  const int mine = __popc(roots);
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int tt = __shfl_up(incl, o, 64);
    if (lane >= o) incl += tt;
  }
  if (lane == 63) sm[wv] = incl;
  if (lane == 0) sm[4 + wv] = before;
  __syncthreads();
  int rank = sm[4] + sm[5] + sm[6] + sm[7] + incl - mine;
  for (int k = 0; k < wv; ++k) rank += sm[k];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if ((roots >> j) & 1u) Pm[i0 + j] = (int)(CC_FLAG | (unsigned)(++rank));
}

// launch 6 (labels): grid (pixels / 256, masks)
__global__ __launch_bounds__(256) void ccl_write_labels_kernel(const int* __restrict__ P, int64_t HW, const int* __restrict__ acc, int* __restrict__ labels,
                                                               int* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const int n = blockIdx.y;
  const int* Pm = P + (size_t)n * (size_t)HW;
  const int w = Pm[i];
  int lab = 0;
  if (w != CC_NONE) lab = (w < 0 ? w : Pm[w]) & CC_LOW;
  labels[(size_t)n * (size_t)HW + i] = lab;
  if (i == 0) count[n] = acc[(size_t)n * CC_ACC + ACC_COUNT];
}

// launch 5 (clean): the selected mask and the statistics
__global__ __launch_bounds__(256) void ccl_write_kept_kernel(const int* __restrict__ P, int64_t HW, const int* __restrict__ acc, int rule, int min_area,
                                                             unsigned char* __restrict__ out, int* __restrict__ count, int* __restrict__ kept,
                                                             int* __restrict__ largest, int* __restrict__ area) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= HW) return;
  const int n = blockIdx.y, i = (int)i64;
  const int* Pm = P + (size_t)n * (size_t)HW;
  const int* a = acc + (size_t)n * CC_ACC;
  const unsigned long long key = *reinterpret_cast<const unsigned long long*>(a + ACC_KEY);
  const int max_area = (int)(key >> 32), best = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
  const int w = Pm[i];
  unsigned char keep = 0;
  if (w != CC_NONE) {
    const bool root = (w & CC_LOW) >= i;
    const int r = root ? i : w, rw = root ? w : Pm[r];
    const int ar = (rw & CC_LOW) - r + 1;
    keep = rule == RULE_LARGEST ? (r == best && max_area >= min_area) : (ar >= min_area);
  }
  out[(size_t)n * (size_t)HW + i] = keep;
  if (i == 0) {
    const int cnt = a[ACC_COUNT];
    const int k = rule == RULE_LARGEST ? ((cnt > 0 && max_area >= min_area) ? 1 : 0) : a[ACC_KEPT];
    count[n] = cnt;
    largest[n] = max_area;
    kept[n] = k;
    area[n] = rule == RULE_LARGEST ? (k ? max_area : 0) : a[ACC_KEPT_AREA];
  }
}

// last launch of the hole pass: an unset pixel whose component does not touch the border becomes set
__global__ __launch_bounds__(256) void ccl_write_holes_kernel(const int* __restrict__ P, int64_t HW, const int* __restrict__ acc, unsigned char* __restrict__ out,
                                                              int* __restrict__ area) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= HW) return;
  const int n = blockIdx.y, i = (int)i64;
  const int* Pm = P + (size_t)n * (size_t)HW;
  const int w = Pm[i];
  if (w != CC_NONE) {
    const bool root = (w & CC_LOW) >= i;
    const int rw = root ? w : Pm[w];
    if (rw >= 0) out[(size_t)n * (size_t)HW + i] = 1;               // (bit 31 clear: no pixel of the component lies on the border)
  }
  if (i == 0) area[n] = (int)(HW - acc[(size_t)n * CC_ACC + ACC_BORDER_AREA]);
}

struct cc_ws {
  int* P;
  int* acc;
  int* chunks;
};
inline cc_ws cc_carve(void* ws, int Ntot, int64_t HW) {
  char* b = (char*)ws;
  cc_ws r;
  r.P = (int*)b;
  r.acc = (int*)(b + cc_align8((size_t)Ntot * (size_t)HW * 4));
  r.chunks = r.acc + (size_t)Ntot * CC_ACC;
  return r;
}

inline bool cc_sizes_ok(int Ntot, int H, int W) { return Ntot > 0 && Ntot <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (1LL << 31); }

// launches 1-4 of one pass.  skip: the measurement aid of include/prn.h (tools/components_bench.py times each launch alone)
int cc_engine(const char* who, const prn_mask_src& src, int Ntot, int H, int W, int vset, int conn8, int border, int rule, int min_area, const cc_ws& ws, hipStream_t st) {
  const int64_t HW = (int64_t)H * W;
  const int tiles_x = cdiv(W, CC_TW), tiles_y = cdiv(H, CC_TH), nchunk = cc_chunks(HW);
  const int nvs = tiles_x - 1, nhs = tiles_y - 1;
  const int64_t nseam = (int64_t)nvs * H + (int64_t)nhs * W;        // (< H W / 32)
  if (!PRN_SKIPPED(1 << 19)) hipLaunchKernelGGL(ccl_local_kernel, dim3(tiles_x * tiles_y, Ntot), dim3(256), 0, st, src, H, W, tiles_x, vset, conn8, ws.P);
  PRN_CHECK_LAUNCH(who);
  if (nseam > 0 && !PRN_SKIPPED(1 << 20)) hipLaunchKernelGGL(ccl_seam_kernel, dim3(cdiv(nseam, 256), Ntot), dim3(256), 0, st, ws.P, H, W, nvs, (int)nseam, conn8);
  PRN_CHECK_LAUNCH(who);
  if (!PRN_SKIPPED(1 << 21)) hipLaunchKernelGGL(ccl_flatten_kernel, dim3(cdiv(HW, CC_FLAT), Ntot), dim3(256), 0, st, ws.P, H, W, border);
  PRN_CHECK_LAUNCH(who);
  if (!PRN_SKIPPED(1 << 22)) hipLaunchKernelGGL(ccl_reduce_kernel, dim3(nchunk, Ntot), dim3(256), 0, st, (const int*)ws.P, HW, nchunk, rule, min_area, ws.acc, ws.chunks);
  PRN_CHECK_LAUNCH(who);
  return 0;
}

}  // namespace

extern "C" int64_t prn_ccl_ws_bytes(int Ntot, int H, int W) {
  if (!cc_sizes_ok(Ntot, H, W)) return -1;
  const int64_t HW = (int64_t)H * W;
  return (int64_t)(cc_align8((size_t)Ntot * (size_t)HW * 4) + (size_t)Ntot * CC_ACC * 4 + (size_t)Ntot * cc_chunks(HW) * 4);
}

#define CC_REQUIRE_SIZES(who)                                                                                                             \
  PRN_REQUIRE(B >= 1 && H > 0 && W > 0 && Ntot > 0, who ": needs B >= 1, Ntot > 0, H > 0, W > 0 (got B=%d Ntot=%d H=%d W=%d)", B, Ntot, H, W); \
  PRN_REQUIRE((int64_t)H * W < (1LL << 31), who ": needs H * W < 2^31 (got %d x %d)", H, W);                                              \
  PRN_REQUIRE(Ntot <= 65535, who ": needs Ntot <= 65535 masks per call (got %d)", Ntot);                                                  \
  PRN_REQUIRE(connectivity == 4 || connectivity == 8, who ": connectivity must be 4 or 8 (got %d)", connectivity);                        \
  PRN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, who ": ws must be 8-byte aligned")

extern "C" int prn_ccl_label(const unsigned char* const* masks_dev, const int* first_dev, int B, int Ntot, int H, int W, int connectivity, int* labels, int* count,
                             void* ws, void* stream) {
  PRN_REQUIRE(masks_dev && first_dev && labels && count && ws, "prn_ccl_label: null pointer argument");
  CC_REQUIRE_SIZES("prn_ccl_label");
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const cc_ws w = cc_carve(ws, Ntot, HW);
  PRN_REQUIRE(hipMemsetAsync(w.acc, 0, (size_t)Ntot * CC_ACC * 4, st) == hipSuccess, "prn_ccl_label: memset failed");
  const prn_mask_src src = {masks_dev, first_dev, B, nullptr};
  if (int rc = cc_engine("prn_ccl_label", src, Ntot, H, W, 1, connectivity == 8, 0, RULE_NONE, 0, w, st)) return rc;
  const int nchunk = cc_chunks(HW);
  if (!PRN_SKIPPED(1 << 23)) hipLaunchKernelGGL(ccl_rank_kernel, dim3(nchunk, Ntot), dim3(256), 0, st, w.P, HW, nchunk, (const int*)w.chunks);
  PRN_CHECK_LAUNCH("prn_ccl_label/rank");
  if (!PRN_SKIPPED(1 << 24))
    hipLaunchKernelGGL(ccl_write_labels_kernel, dim3(cdiv(HW, 256), Ntot), dim3(256), 0, st, (const int*)w.P, HW, (const int*)w.acc, labels, count);
  PRN_CHECK_LAUNCH("prn_ccl_label/write");
  return 0;
}

extern "C" int prn_ccl_clean(const unsigned char* const* masks_dev, const int* first_dev, int B, int Ntot, int H, int W, int connectivity, int keep_all,
                             int min_area, int fill_holes, unsigned char* out, int* count, int* kept, int* largest, int* area, void* ws, void* stream) {
  PRN_REQUIRE(masks_dev && first_dev && out && count && kept && largest && area && ws, "prn_ccl_clean: null pointer argument");
  CC_REQUIRE_SIZES("prn_ccl_clean");
  PRN_REQUIRE(min_area >= 0, "prn_ccl_clean: min_area must be >= 0 (got %d)", min_area);
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const cc_ws w = cc_carve(ws, Ntot, HW);
  PRN_REQUIRE(hipMemsetAsync(w.acc, 0, (size_t)Ntot * CC_ACC * 4, st) == hipSuccess, "prn_ccl_clean: memset failed");
  const prn_mask_src src = {masks_dev, first_dev, B, nullptr};
  const int rule = keep_all ? RULE_MIN_AREA : RULE_LARGEST, conn8 = connectivity == 8;
  if (int rc = cc_engine("prn_ccl_clean", src, Ntot, H, W, 1, conn8, 0, rule, min_area, w, st)) return rc;
  if (!PRN_SKIPPED(1 << 24))
    hipLaunchKernelGGL(ccl_write_kept_kernel, dim3(cdiv(HW, 256), Ntot), dim3(256), 0, st, (const int*)w.P, HW, (const int*)w.acc, rule, min_area, out, count, kept,
                       largest, area);
  PRN_CHECK_LAUNCH("prn_ccl_clean/write");
  if (fill_holes) {
    // the same engine on the selection: v = unset, the dual connectivity, rule "touches the border" (its own accumulator word)
    const prn_mask_src sel = {nullptr, nullptr, 0, out};
    if (int rc = cc_engine("prn_ccl_clean/holes", sel, Ntot, H, W, 0, !conn8, 1, RULE_BORDER, 0, w, st)) return rc;
    if (!PRN_SKIPPED(1 << 24))
      hipLaunchKernelGGL(ccl_write_holes_kernel, dim3(cdiv(HW, 256), Ntot), dim3(256), 0, st, (const int*)w.P, HW, (const int*)w.acc, out, area);
    PRN_CHECK_LAUNCH("prn_ccl_clean/holes/write");
  }
  return 0;
}
