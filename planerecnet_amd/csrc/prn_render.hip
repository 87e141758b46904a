// What a user looks at, drawn on the device (include/prn.h: prn_render_*): the inference overlay (instance masks
// blended over the frame, optional one-pixel mask outlines, box outlines) and the depth picture (1 % / 99 % limits without a sort, a
// 256-entry colour table or a 16-bit gray image).  simple_inference.py did all of it on the host: N full-frame float passes per image.
//   overlay   ONE launch, grid (W / 128, H / 8), 256 threads, four adjacent pixels per thread.  Box and colour tables go through LDS in
//             chunks of 128 instances, highest chunk first (the blend runs from the last instance down, and the highest box index wins).
//             Without outlines every thread reads its own four mask bytes of sixteen instances at a time (one 4-byte load each, all in
//             flight together); with outlines sixteen instances' tiles plus a one-pixel halo are staged in LDS once and the five words of
//             the 4-neighbourhood are LDS reads.  Blend arithmetic: two rounded multiplies and one rounded add, contraction off.
//   limits    radix select on the order-preserving integer key of the fp32 pattern, 8 bits per pass, six order statistics together (the
//             four percentile neighbours, the minimum, the maximum); integer histograms only, so the result does not depend on scheduling.
//   colours   one pass, four pixels per thread.
// A scalar path (bytes / single floats, bounds checked per pixel) covers widths that are no multiple of four and unaligned pointers; it
// runs the same arithmetic per pixel and writes the same bytes.
#include "prn_masks.h"

namespace {

constexpr int RD_TW = 128, RD_TH = 8;          // pixels of one workgroup: 32 threads x 4 pixels wide, 8 rows
constexpr int RD_TAB = 128;                    // instances per chunk of the box / colour tables in LDS
constexpr int RD_G = 16;                       // instances whose mask words are fetched together
constexpr int RD_LW = RD_TW / 4 + 2;           // outline mode: words of a staged row (one halo word on each side)
constexpr int RD_LH = RD_TH + 2;               //               rows of a staged tile (one halo row above and below)

// the mask bytes of pixels (y, x .. x+3) of one instance as a word, x a multiple of 4 (-4 and >= W occur in the halo); outside the image: 0
template <bool WIDE>
__device__ __forceinline__ unsigned mask_word(const unsigned char* __restrict__ m, int y, int x, int H, int W) {
  if (y < 0 || y >= H || x < 0 || x >= W) return 0u;
  const unsigned char* p = m + (size_t)y * W + x;
  if (WIDE) return *reinterpret_cast<const unsigned*>(p);         // W % 4 == 0 and m 4-byte aligned: the word lies inside the row
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (x + k < W) v |= (unsigned)p[k] << (8 * k);
  return v;
}

// v <- fl(fl(v * oma) + ca) on the pixels of `bits`; ca = fl(colour * alpha)
__device__ __forceinline__ void blend4(float (&v)[4][3], unsigned bits, const float* ca, float oma) {
#pragma clang fp contract(off)
  const float c0 = ca[0], c1 = ca[1], c2 = ca[2];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((bits >> k) & 1u) {
      v[k][0] = v[k][0] * oma + c0;                               // (contraction is off: a multiply and an add, each rounded)
      v[k][1] = v[k][1] * oma + c1;
      v[k][2] = v[k][2] * oma + c2;
    }
}

__device__ __forceinline__ unsigned trunc_u8(float f) {             // toward zero, saturated to [0, 255]; NaN -> 0
  return (unsigned)(int)fminf(fmaxf(f, 0.f), 255.f);
}

template <bool WIDE, bool CONTOUR>
__global__ __launch_bounds__(256) void render_overlay_kernel(const float* __restrict__ frame, const unsigned char* __restrict__ masks,
                                                             const unsigned char* __restrict__ colors, const int* __restrict__ boxes, int N, int H, int W,
                                                             float alpha, float oma, int layers, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ int4 s_box[RD_TAB];
  __shared__ float s_ca[RD_TAB][3];
  __shared__ unsigned s_col[RD_TAB];
  __shared__ unsigned s_m[CONTOUR ? RD_G * RD_LH * RD_LW : 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int x0 = blockIdx.x * RD_TW, y0 = blockIdx.y * RD_TH;
  const int x = x0 + tx * 4, y = y0 + ty;
  const bool live = x < W && y < H;
  const size_t HW = (size_t)H * W;
  const bool do_mask = (layers & PRN_RENDER_MASKS) != 0, do_box = (layers & PRN_RENDER_BOXES) != 0;

  float v[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k][0] = v[k][1] = v[k][2] = 0.f;
  if (live) {
    const float* f = frame + ((size_t)y * W + x) * 3;
    if (WIDE) {                                                   // W % 4 == 0 and frame 16-byte aligned: 48 contiguous aligned bytes
      const float4 a = reinterpret_cast<const float4*>(f)[0], b = reinterpret_cast<const float4*>(f)[1], c = reinterpret_cast<const float4*>(f)[2];
      v[0][0] = a.x; v[0][1] = a.y; v[0][2] = a.z; v[1][0] = a.w; v[1][1] = b.x; v[1][2] = b.y;
      v[2][0] = b.z; v[2][1] = b.w; v[2][2] = c.x; v[3][0] = c.y; v[3][1] = c.z; v[3][2] = c.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) { v[k][0] = f[3 * k]; v[k][1] = f[3 * k + 1]; v[k][2] = f[3 * k + 2]; }
    }
  }
  unsigned cont = 0u, boxed = 0u;                                  // per pixel (bits 0..3): on some mask's outline / box colour found
  unsigned boxcol[4] = {0u, 0u, 0u, 0u};

  for (int cb = N > 0 ? (N - 1) / RD_TAB * RD_TAB : -1; cb >= 0; cb -= RD_TAB) {
    const int nc = N - cb < RD_TAB ? N - cb : RD_TAB;
    __syncthreads();                                              // the previous chunk's tables are no longer read
    for (int j = threadIdx.x; j < nc; j += 256) {
      const int i = cb + j;
      if (layers & (PRN_RENDER_MASKS | PRN_RENDER_BOXES)) {
        const unsigned b = colors[3 * i], g = colors[3 * i + 1], r = colors[3 * i + 2];
        s_ca[j][0] = (float)b * alpha; s_ca[j][1] = (float)g * alpha; s_ca[j][2] = (float)r * alpha;
        s_col[j] = b | (g << 8) | (r << 16);
      }
      if (do_box) s_box[j] = make_int4(boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3]);
    }
    __syncthreads();

    if (CONTOUR) {
      for (int jt = nc - 1; jt >= 0; jt -= RD_G) {                 // instances cb + jt, cb + jt - 1, ... in slots 0, 1, ...
        __syncthreads();                                          // the previous group's words are no longer read
        for (int idx = threadIdx.x; idx < RD_G * RD_LH * RD_LW; idx += 256) {
          const int g = idx / (RD_LH * RD_LW), rem = idx - g * (RD_LH * RD_LW), r = rem / RD_LW, c = rem - r * RD_LW;
          const int j = jt - g;
          s_m[idx] = j >= 0 ? mask_word<WIDE>(masks + (size_t)(cb + j) * HW, y0 - 1 + r, x0 - 4 + 4 * c, H, W) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < RD_G; ++g) {
          const int j = jt - g;
          if (j < 0) break;
          const unsigned* t = s_m + g * (RD_LH * RD_LW) + (ty + 1) * RD_LW + tx + 1;
          const unsigned C = prn_nz4(t[0]);
          if (C == 0u) continue;
          const unsigned U = prn_nz4(t[-RD_LW]), D = prn_nz4(t[RD_LW]);
          const unsigned L = ((C << 1) & 15u) | (t[-1] >> 24 ? 1u : 0u), R = (C >> 1) | (t[1] & 255u ? 8u : 0u);
          cont |= C & ~(U & D & L & R);                           // set, and a 4-neighbour is not (outside the image counts as not set)
          if (do_mask) blend4(v, C, s_ca[j], oma);
        }
      }
    } else if (do_mask) {
      const unsigned char* mp = masks + (size_t)cb * HW;
      for (int jt = nc - 1; jt >= 0; jt -= RD_G) {
        unsigned w[RD_G];
#pragma unroll
        for (int g = 0; g < RD_G; ++g) w[g] = (live && jt - g >= 0) ? mask_word<WIDE>(mp + (size_t)(jt - g) * HW, y, x, H, W) : 0u;
#pragma unroll
        for (int g = 0; g < RD_G; ++g)
          if (w[g] != 0u) blend4(v, prn_nz4(w[g]), s_ca[jt - g], oma);
      }
    }

    if (do_box && live) {
      for (int j = nc - 1; j >= 0 && boxed != 15u; --j) {          // chunks and j descend: the first hit is the highest index
        const int4 b = s_box[j];                                  // x0 y0 x1 y1
        if (y < b.y || y > b.w) continue;
        const bool edge_row = y == b.y || y == b.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int xx = x + k;
          const bool hit = edge_row ? (xx >= b.x && xx <= b.z) : (xx == b.x || xx == b.z);
          if (hit && !((boxed >> k) & 1u)) { boxed |= 1u << k; boxcol[k] = s_col[j]; }
        }
      }
    }
  }

  if (!live) return;
  unsigned px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    px[k] = trunc_u8(v[k][0]) | (trunc_u8(v[k][1]) << 8) | (trunc_u8(v[k][2]) << 16);
    if ((cont >> k) & 1u) px[k] = 0x00FFFFFFu;
    if ((boxed >> k) & 1u) px[k] = boxcol[k];
  }
  unsigned char* o = out + ((size_t)y * W + x) * 3;
  if (WIDE) {                                                     // W % 4 == 0 and out 4-byte aligned: 12 aligned bytes
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
    o4[0] = px[0] | (px[1] << 24);
    o4[1] = (px[1] >> 8) | (px[2] << 16);
    o4[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < W) { o[3 * k] = px[k] & 255u; o[3 * k + 1] = (px[k] >> 8) & 255u; o[3 * k + 2] = (px[k] >> 16) & 255u; }
  }
}

// ---- depth limits: radix select ----------------------------------------------------------------------------------------------------
constexpr int RL_R = 6;                        // order statistics selected together: lo floor / ceil, hi floor / ceil, minimum, maximum
constexpr int RL_PASSES = 4;                   // 8 bits of the key per pass
constexpr int RL_MAX_BLOCKS = 1024;

__device__ __forceinline__ unsigned f32_key(float f) {              // a < b (as floats, -0 < +0)  <=>  key(a) < key(b) (as unsigned)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// virtual index (cnt - 1) * q in fp64 -> its floor and the fraction above it
__device__ __forceinline__ void virtual_index(unsigned cnt, double q, unsigned& below, double& frac) {
#pragma clang fp contract(off)
  const double vi = (double)(cnt - 1u) * q, f = floor(vi);
  below = (unsigned)f;
  frac = vi - f;
}

__device__ __forceinline__ unsigned rank_of(int r, unsigned cnt, double q_lo, double q_hi) {
  if (cnt == 0u) return 0u;
  if (r == 4) return 0u;
  if (r == 5) return cnt - 1u;
  unsigned below;
  double frac;
  virtual_index(cnt, r < 2 ? q_lo : q_hi, below, frac);
  return (r & 1) ? (below + 1u < cnt ? below + 1u : cnt - 1u) : below;
}

// The whole workgroup (256 threads): from the histograms of passes 0 .. np-1, every rank's key prefix (its top 8 np bits) and its rank
// among the elements that share the prefix -> s_pref / s_rank [RL_R], the non-NaN count -> *s_cnt.  hist [RL_PASSES][RL_R][256]; pass 0
// has no prefix to tell the ranks apart and fills slot [0][0] only.  One wave per rank: four bins per lane, a prefix sum over the lanes.
__device__ void select_resolve(const unsigned* __restrict__ hist, int np, double q_lo, double q_hi, unsigned* s_pref, unsigned* s_rank, unsigned* s_cnt) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint4 h0 = reinterpret_cast<const uint4*>(hist)[lane];
  unsigned cnt = h0.x + h0.y + h0.z + h0.w;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
  for (int r = wave; r < RL_R; r += 4) {                          // wave-uniform
    unsigned rank = rank_of(r, cnt, q_lo, q_hi), pref = 0u;
    for (int p = 0; p < np; ++p) {
      const uint4 h = reinterpret_cast<const uint4*>(hist + (size_t)(p == 0 ? 0 : p * RL_R + r) * 256)[lane];
      const unsigned s = h.x + h.y + h.z + h.w;
      unsigned inc = s;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
      }
      const unsigned exc = inc - s;
      const bool mine = rank >= exc && rank < inc;                // at most one lane
      unsigned digit = 0u, below = 0u;
      if (mine) {
        unsigned c = exc;
        if (rank < c + h.x) { digit = 4 * lane; below = c; }
        else if (rank < (c += h.x) + h.y) { digit = 4 * lane + 1; below = c; }
        else if (rank < (c += h.y) + h.z) { digit = 4 * lane + 2; below = c; }
        else { c += h.z; digit = 4 * lane + 3; below = c; }
      }
      const unsigned long long bal = __ballot(mine);
      const int src = bal ? __ffsll((long long)bal) - 1 : 0;      // no lane (an empty map): digit 0, nothing below
      digit = __shfl(digit, src);
      below = __shfl(below, src);
      pref = (pref << 8) | digit;
      rank -= below;
    }
    if (lane == 0) { s_pref[r] = pref; s_rank[r] = rank; }
  }
  if (threadIdx.x == 0) *s_cnt = cnt;
  __syncthreads();
}

// pass p: among the non-NaN elements whose key starts with rank r's prefix, a histogram of the next 8 bits (LDS, then integer adds to hist)
__global__ __launch_bounds__(256) void render_select_hist_kernel(const float* __restrict__ d, unsigned n, int wide, int pass, double q_lo, double q_hi,
                                                                 unsigned* __restrict__ hist) {
  __shared__ unsigned s_h[RL_R * 256];
  __shared__ unsigned s_pref[RL_R], s_rank[RL_R], s_cnt;
  const int nr = pass == 0 ? 1 : RL_R;
  for (int k = threadIdx.x; k < nr * 256; k += 256) s_h[k] = 0u;
  if (pass > 0) select_resolve(hist, pass, q_lo, q_hi, s_pref, s_rank, &s_cnt);
  else __syncthreads();
  unsigned pref[RL_R];
#pragma unroll
  for (int r = 0; r < RL_R; ++r) pref[r] = pass > 0 ? s_pref[r] : 0u;
  const int shift = 24 - 8 * pass;
  for (size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < n; i0 += (size_t)gridDim.x * 1024) {
    float f[4];
    if (wide && i0 + 4 <= n) {
      const float4 q = *reinterpret_cast<const float4*>(d + i0);
      f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) f[k] = i0 + k < n ? d[i0 + k] : __builtin_nanf("");
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (f[k] != f[k]) continue;
      const unsigned key = f32_key(f[k]);
      if (pass == 0) {
        atomicAdd(&s_h[key >> 24], 1u);
      } else {
        const unsigned top = key >> (shift + 8), digit = (key >> shift) & 255u;
#pragma unroll
        for (int r = 0; r < RL_R; ++r)
          if (top == pref[r]) atomicAdd(&s_h[r * 256 + digit], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* gh = hist + (size_t)pass * RL_R * 256;
  for (int k = threadIdx.x; k < nr * 256; k += 256)
    if (s_h[k]) atomicAdd(&gh[k], s_h[k]);
}

// one workgroup: the six keys are complete -> out [8] = vmin, vmax, the two neighbours of each, minimum, maximum
__global__ __launch_bounds__(256) void render_select_final_kernel(const unsigned* __restrict__ hist, double q_lo, double q_hi, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ unsigned s_pref[RL_R], s_rank[RL_R], s_cnt;
  select_resolve(hist, RL_PASSES, q_lo, q_hi, s_pref, s_rank, &s_cnt);
  if (threadIdx.x != 0) return;
  const unsigned cnt = s_cnt;
  if (cnt == 0u) {                                                // nothing but NaN
    for (int k = 0; k < 8; ++k) out[k] = 0.f;
    return;
  }
  float s[RL_R];
  for (int r = 0; r < RL_R; ++r) s[r] = key_f32(s_pref[r]);
  unsigned below;
  double g_lo, g_hi;
  virtual_index(cnt, q_lo, below, g_lo);
  virtual_index(cnt, q_hi, below, g_hi);
  out[0] = (float)((double)s[0] + ((double)s[1] - (double)s[0]) * g_lo);
  out[1] = (float)((double)s[2] + ((double)s[3] - (double)s[2]) * g_hi);
  out[2] = s[0]; out[3] = s[1]; out[4] = s[2]; out[5] = s[3]; out[6] = s[4]; out[7] = s[5];
}

// ---- depth -> colours / 16-bit gray ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void render_depth_colors_kernel(const float* __restrict__ d, unsigned n, int wide, const float* __restrict__ lim,
                                                                  const unsigned char* __restrict__ lut, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ unsigned s_lut[256];
  for (int k = threadIdx.x; k < 256; k += 256) s_lut[k] = lut[3 * k] | ((unsigned)lut[3 * k + 1] << 8) | ((unsigned)lut[3 * k + 2] << 16);
  const float vmin = lim[0], vmax = lim[1];
  const float lo = fminf(fmaxf(lim[6], vmin), vmax), hi = fminf(fmaxf(lim[7], vmin), vmax);      // the extremes of the clipped map
  const float span = hi - lo, den = 1e-12f > span ? 1e-12f : span;
  __syncthreads();
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  float f[4];
  const bool full = wide && i0 + 4 <= n;
  if (full) {
    const float4 q = *reinterpret_cast<const float4*>(d + i0);
    f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = i0 + k < n ? d[i0 + k] : 0.f;
  }
  unsigned px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned level = 0u;
    if (f[k] == f[k]) {
      const float c = fminf(fmaxf(f[k], vmin), vmax);
      level = trunc_u8((c - lo) / den * 255.f);              // the division: correctly rounded (hipcc's default for fp32)
    }
    px[k] = s_lut[level];
  }
  unsigned char* o = out + i0 * 3;
  if (full) {                                                     // out 4-byte aligned (checked by the caller of the wide path)
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
    o4[0] = px[0] | (px[1] << 24);
    o4[1] = (px[1] >> 8) | (px[2] << 16);
    o4[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < n) { o[3 * k] = px[k] & 255u; o[3 * k + 1] = (px[k] >> 8) & 255u; o[3 * k + 2] = (px[k] >> 16) & 255u; }
  }
}

__global__ __launch_bounds__(256) void render_depth_gray_kernel(const float* __restrict__ d, unsigned n, float shift, unsigned short* __restrict__ out) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float t = d[i] * shift;
  out[i] = (unsigned short)(int)fminf(fmaxf(t, 0.f), 65535.f);     // toward zero, saturated; NaN -> 0
}

bool map_ok(int64_t n) { return n > 0 && n < (1LL << 31); }
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int prn_render_overlay(const float* frame, const unsigned char* masks, const unsigned char* colors, const int* boxes, int N, int H, int W,
                                  float alpha, float one_minus_alpha, int layers, unsigned char* out, void* stream) {
  PRN_REQUIRE(N >= 0 && H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) && cdiv(H, RD_TH) <= 65535, "prn_render_overlay: bad sizes (N=%d H=%d W=%d)", N, H, W);
  PRN_REQUIRE((layers & ~(PRN_RENDER_MASKS | PRN_RENDER_CONTOURS | PRN_RENDER_BOXES)) == 0, "prn_render_overlay: unknown layer flags 0x%x", layers);
  PRN_REQUIRE(frame && out, "prn_render_overlay: null frame / output");
  PRN_REQUIRE((const void*)out != (const void*)frame, "prn_render_overlay: the output must not alias the frame");
  const bool need_masks = N > 0 && (layers & (PRN_RENDER_MASKS | PRN_RENDER_CONTOURS)), need_boxes = N > 0 && (layers & PRN_RENDER_BOXES);
  const bool need_colors = N > 0 && (layers & (PRN_RENDER_MASKS | PRN_RENDER_BOXES));
  PRN_REQUIRE(!need_masks || masks, "prn_render_overlay: null masks");
  PRN_REQUIRE(!need_colors || colors, "prn_render_overlay: null colour table");
  PRN_REQUIRE(!need_boxes || boxes, "prn_render_overlay: null boxes");
  const bool wide = W % 4 == 0 && aligned(frame, 16) && aligned(out, 4) && (!need_masks || aligned(masks, 4));
  const bool contour = need_masks && (layers & PRN_RENDER_CONTOURS);
  const dim3 grid(cdiv(W, RD_TW), cdiv(H, RD_TH)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (!need_masks) layers &= ~(PRN_RENDER_MASKS | PRN_RENDER_CONTOURS);
#define PRN_RENDER_LAUNCH(WIDE_, CONT_) \
  hipLaunchKernelGGL((render_overlay_kernel<WIDE_, CONT_>), grid, block, 0, st, frame, masks, colors, boxes, N, H, W, alpha, one_minus_alpha, layers, out)
  if (wide) {
    if (contour) PRN_RENDER_LAUNCH(true, true); else PRN_RENDER_LAUNCH(true, false);
  } else {
    if (contour) PRN_RENDER_LAUNCH(false, true); else PRN_RENDER_LAUNCH(false, false);
  }
#undef PRN_RENDER_LAUNCH
  PRN_CHECK_LAUNCH("prn_render_overlay");
  return 0;
}

extern "C" int64_t prn_render_limits_ws_bytes(void) { return (int64_t)RL_PASSES * RL_R * 256 * (int64_t)sizeof(unsigned); }

extern "C" int prn_render_depth_limits(const float* depth, int64_t n, double q_lo, double q_hi, float* limits, void* ws, void* stream) {
  PRN_REQUIRE(map_ok(n), "prn_render_depth_limits: bad size (n=%lld)", (long long)n);
  PRN_REQUIRE(q_lo >= 0.0 && q_lo <= 1.0 && q_hi >= 0.0 && q_hi <= 1.0, "prn_render_depth_limits: quantiles outside [0, 1] (%g, %g)", q_lo, q_hi);
  PRN_REQUIRE(depth && limits && ws, "prn_render_depth_limits: null depth / limits / workspace");
  PRN_REQUIRE(aligned(ws, 16) && aligned(limits, 4), "prn_render_depth_limits: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned* hist = static_cast<unsigned*>(ws);
  if (hipMemsetAsync(hist, 0, (size_t)prn_render_limits_ws_bytes(), st) != hipSuccess) {
    prn_set_error("prn_render_depth_limits: clearing the workspace failed");
    return 1;
  }
  const int blocks = cdiv(n, 1024) < RL_MAX_BLOCKS ? cdiv(n, 1024) : RL_MAX_BLOCKS;
  const int wide = aligned(depth, 16) ? 1 : 0;
  for (int pass = 0; pass < RL_PASSES; ++pass) {
    hipLaunchKernelGGL(render_select_hist_kernel, dim3(blocks), dim3(256), 0, st, depth, (unsigned)n, wide, pass, q_lo, q_hi, hist);
    PRN_CHECK_LAUNCH("prn_render_depth_limits/hist");
  }
  hipLaunchKernelGGL(render_select_final_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)hist, q_lo, q_hi, limits);
  PRN_CHECK_LAUNCH("prn_render_depth_limits/final");
  return 0;
}

extern "C" int prn_render_depth_colors(const float* depth, int64_t n, const float* limits, const unsigned char* lut, unsigned char* out, void* stream) {
  PRN_REQUIRE(map_ok(n), "prn_render_depth_colors: bad size (n=%lld)", (long long)n);
  PRN_REQUIRE(depth && limits && lut && out, "prn_render_depth_colors: null depth / limits / table / output");
  const int wide = aligned(depth, 16) && aligned(out, 4) ? 1 : 0;
  hipLaunchKernelGGL(render_depth_colors_kernel, dim3(cdiv(n, 1024)), dim3(256), 0, (hipStream_t)stream, depth, (unsigned)n, wide, limits, lut, out);
  PRN_CHECK_LAUNCH("prn_render_depth_colors");
  return 0;
}

extern "C" int prn_render_depth_gray(const float* depth, int64_t n, float shift, unsigned short* out, void* stream) {
  PRN_REQUIRE(map_ok(n), "prn_render_depth_gray: bad size (n=%lld)", (long long)n);
  PRN_REQUIRE(depth && out, "prn_render_depth_gray: null depth / output");
  PRN_REQUIRE(aligned(out, 2), "prn_render_depth_gray: the output must be 2-byte aligned");
  hipLaunchKernelGGL(render_depth_gray_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, depth, (unsigned)n, shift, out);
  PRN_CHECK_LAUNCH("prn_render_depth_gray");
  return 0;
}
