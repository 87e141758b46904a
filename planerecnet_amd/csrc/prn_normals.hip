// Surface normals of a depth map and the angular error of two normal maps (include/prn.h: prn_normals, prn_normal_error).
//   normals   one workgroup per NRM_PX consecutive pixels (row-major) of one image, a thread takes one pixel: its depth and label and those of
//             its four neighbours `step` away (L1 / L2 hits: the rows above and below were some workgroup's own pixels), up to five back-projected
//             points in fp64, two tangents, their cross product and its length.  Every fp64 product and difference is rounded on its own (fp
//             contraction off in each device function: the file-level pragma does not reach them), so numpy restates the output bit for bit.
//             The 12-byte records and 3-byte colours are staged in LDS at the thread's slot and leave as whole dwords, consecutive lanes on
//             consecutive dwords.  No atomics.
//   error     one workgroup per ERR_PX consecutive pixels of one image pair: a uint32 histogram of the chord |a - b| in 16 KB of LDS (LDS
//             integer atomics), flushed where non-zero with 64-bit global integer atomics; the threshold and pixel counts are popcounts of wave
//             ballots, summed per wave in registers.  Integer sums in any order are the same sum: identical run to run.
// The image is the grid's y, so a batch costs the launch of one image.  Nothing is allocated or synchronised, inputs are only read.
#include "prn_common.h"

namespace {

typedef unsigned long long u64;

constexpr int NRM_PX = 256;                      // pixels (= threads) of one workgroup
constexpr int ERR_BINS = 4096;                   // chord bins over [0, 2]
constexpr int ERR_TH = 256;                      // threads of an error workgroup
constexpr int ERR_PX = 4096;                     // pixels of an error workgroup (ERR_PX / ERR_TH a thread)
static_assert(NRM_PX == 256 && ERR_TH == 256, "four waves a workgroup");

struct nrm_in {
  const float* depth;                            // [B][H][W]
  const int* labels;                             // [B][H][W] or NULL
  const double* k;                               // [B][9]
  int H, W, HW, step;
  float lo, hi, gap;
  int flags;
};

struct d3 { double x, y, z; };

__device__ __forceinline__ bool nrm_valid(const nrm_in& m, float z) { return __builtin_isfinite(z) && m.lo < z && z < m.hi; }

// a valid centre (zc, lc) and a neighbour inside the image: valid, of the centre's label (if asked) and close in depth, every operation rounded to
// fp32 on its own
__device__ __forceinline__ bool nrm_usable(const nrm_in& m, float zc, int lc, float zq, int lq) {
  if (!nrm_valid(m, zq)) return false;
  if ((m.flags & PRN_NORMALS_SAME_LABEL) && lq != lc) return false;
  const float zmax = fmaxf(zc, zq), zmin = fminf(zc, zq);
  const float bound = (m.flags & PRN_NORMALS_RELATIVE) ? __fmul_rn(m.gap, zmin) : m.gap;
  return __fsub_rn(zmax, zmin) <= bound;
}

__device__ __forceinline__ d3 nrm_point(int u, int v, float z, double fx, double fy, double cx, double cy) {
#pragma clang fp contract(off)
  d3 p;
  p.x = ((double)u - cx) * (double)z / fx;
  p.y = ((double)v - cy) * (double)z / fy;
  p.z = (double)z;
  return p;
}

__device__ __forceinline__ d3 nrm_sub(const d3& a, const d3& b) {
#pragma clang fp contract(off)
  d3 r;
  r.x = a.x - b.x;
  r.y = a.y - b.y;
  r.z = a.z - b.z;
  return r;
}

// the tangent along one axis: plus / minus = the neighbours at +step / -step (ok_*: usable), c = the centre
__device__ __forceinline__ d3 nrm_tangent(bool ok_plus, bool ok_minus, const d3& plus, const d3& minus, const d3& c) {
  return nrm_sub(ok_plus ? plus : c, ok_minus ? minus : c);
}

// tv x tu and its squared length, nothing fused
__device__ __forceinline__ d3 nrm_cross(const d3& tv, const d3& tu, double& l2) {
#pragma clang fp contract(off)
  d3 n;
  const double a0 = tv.y * tu.z, a1 = tv.z * tu.y, b0 = tv.z * tu.x, b1 = tv.x * tu.z, c0 = tv.x * tu.y, c1 = tv.y * tu.x;
  n.x = a0 - a1;
  n.y = b0 - b1;
  n.z = c0 - c1;
  const double xx = n.x * n.x, yy = n.y * n.y, zz = n.z * n.z;
  const double s = xx + yy;
  l2 = s + zz;
  return n;
}

__device__ __forceinline__ unsigned char nrm_byte(float c) {
#pragma clang fp contract(off)
  const double h = (double)c * 0.5;
  const double s = h + 0.5;
  return (unsigned char)(int)rint(s * 255.0);
}

// n dwords of LDS to o, consecutive lanes on consecutive dwords
__device__ __forceinline__ void nrm_store_words(float* __restrict__ o, const float* s, unsigned n) {
  for (unsigned i = threadIdx.x; i < n; i += NRM_PX) o[i] = s[i];
}

__global__ __launch_bounds__(NRM_PX) void normals_kernel(nrm_in m, float* __restrict__ normals, unsigned char* __restrict__ valid, unsigned char* __restrict__ image) {
#pragma clang fp contract(off)
  __shared__ float s_n[3 * NRM_PX];
  __shared__ unsigned char s_col[3 * NRM_PX];
  const int img = blockIdx.y;
  const size_t at = (size_t)img * m.HW;
  const int base = (int)(blockIdx.x * NRM_PX);                       // (< HW < 2^24)
  const int p = base + (int)threadIdx.x;
  const float* __restrict__ d = m.depth + at;
  const int* __restrict__ l = m.labels ? m.labels + at : nullptr;
  float ox = 0.f, oy = 0.f, oz = 0.f;
  bool ok = false;
  if (p < m.HW) {
    const float zc = d[p];
    if (nrm_valid(m, zc)) {
      const int lc = l ? l[p] : 0;
      const int v = p / m.W, u = p - v * m.W, st = m.step;
      const bool in_e = st < m.W - u, in_w = u >= st, in_s = st < m.H - v, in_n = v >= st;       // (no u + step: step may be near 2^31)
      const int pe = in_e ? p + st : p, pw = in_w ? p - st : p, ps = in_s ? p + st * m.W : p, pn = in_n ? p - st * m.W : p;
      const float ze = in_e ? d[pe] : 0.f, zw = in_w ? d[pw] : 0.f, zs = in_s ? d[ps] : 0.f, zn = in_n ? d[pn] : 0.f;
      const int le = (l && in_e) ? l[pe] : 0, lw = (l && in_w) ? l[pw] : 0, ls = (l && in_s) ? l[ps] : 0, ln = (l && in_n) ? l[pn] : 0;
      const bool ue = in_e && nrm_usable(m, zc, lc, ze, le), uw = in_w && nrm_usable(m, zc, lc, zw, lw);
      const bool us = in_s && nrm_usable(m, zc, lc, zs, ls), un = in_n && nrm_usable(m, zc, lc, zn, ln);
      if ((ue || uw) && (us || un)) {
        const double* k = m.k + 9 * img;
        const double fx = k[0], fy = k[4], cx = k[2], cy = k[5];
        const d3 c = nrm_point(u, v, zc, fx, fy, cx, cy);
        const d3 e = ue ? nrm_point(u + st, v, ze, fx, fy, cx, cy) : c, w = uw ? nrm_point(u - st, v, zw, fx, fy, cx, cy) : c;
        const d3 s = us ? nrm_point(u, v + st, zs, fx, fy, cx, cy) : c, n = un ? nrm_point(u, v - st, zn, fx, fy, cx, cy) : c;
        const d3 tu = nrm_tangent(ue, uw, e, w, c), tv = nrm_tangent(us, un, s, n, c);
        double l2;
        const d3 r = nrm_cross(tv, tu, l2);
        if (__builtin_isfinite(l2) && l2 > 0.0) {
          const double len = sqrt(l2);
          ox = (float)(r.x / len);
          oy = (float)(r.y / len);
          oz = (float)(r.z / len);
          if (m.flags & PRN_NORMALS_PLANE_SIGN) { ox = -ox; oy = -oy; oz = -oz; }
          ok = true;
        }
      }
    }
    valid[at + p] = ok ? 1 : 0;                                      // (a wave: 64 consecutive bytes)
  }
  const unsigned t = threadIdx.x;
  s_n[3 * t] = ox;
  s_n[3 * t + 1] = oy;
  s_n[3 * t + 2] = oz;
  if (image) {
    s_col[3 * t] = ok ? nrm_byte(oz) : 0;
    s_col[3 * t + 1] = ok ? nrm_byte(oy) : 0;
    s_col[3 * t + 2] = ok ? nrm_byte(ox) : 0;
  }
  __syncthreads();
  const unsigned cnt = (unsigned)min(NRM_PX, m.HW - base);           // (>= 1: the grid has cdiv(HW, NRM_PX) workgroups)
  nrm_store_words(normals + (at + base) * 3, s_n, 3u * cnt);
  if (image) {
    unsigned char* o = image + (at + base) * 3;
    const unsigned nb = 3u * cnt;
    const unsigned head = min(nb, (unsigned)((4u - (unsigned)(reinterpret_cast<uintptr_t>(o) & 3u)) & 3u));    // bytes before the first 4-byte boundary
    const unsigned words = (nb - head) >> 2, tail = head + 4u * words;
    if (t < head) o[t] = s_col[t];
    unsigned* ow = reinterpret_cast<unsigned*>(o + head);
    for (unsigned i = t; i < words; i += NRM_PX) {
      const unsigned char* s = s_col + head + 4u * i;
      ow[i] = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    }
    if (t < nb - tail) o[tail + t] = s_col[tail + t];
  }
}

struct err_thr { double v[PRN_NORMAL_ERROR_MAX_T]; };

__device__ __forceinline__ double err_d2(const float* __restrict__ a, const float* __restrict__ b) {
#pragma clang fp contract(off)
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double s = xx + yy;
  return s + zz;
}

__device__ __forceinline__ int err_bin(double d2) {
#pragma clang fp contract(off)
  const double t = floor(sqrt(d2) * (double)(ERR_BINS / 2));
  return t < (double)(ERR_BINS - 1) ? (int)t : ERR_BINS - 1;       // (a NaN lands in the last bin; t >= 0)
}

__global__ __launch_bounds__(ERR_TH) void normal_error_kernel(const float* __restrict__ a, const unsigned char* __restrict__ va, const float* __restrict__ b,
                                                              const unsigned char* __restrict__ vb, int64_t n, err_thr thr, int T, u64* __restrict__ hist,
                                                              u64* __restrict__ within, u64* __restrict__ count) {
  __shared__ unsigned s_h[ERR_BINS];
  __shared__ unsigned s_c[4][PRN_NORMAL_ERROR_MAX_T + 1];
  const int img = blockIdx.y;
  const int64_t at = (int64_t)img * n;
  for (int i = threadIdx.x; i < ERR_BINS; i += ERR_TH) s_h[i] = 0u;
  __syncthreads();
  unsigned c[PRN_NORMAL_ERROR_MAX_T + 1];                           // wave-uniform: the wave's pixels within each threshold, [MAX_T]: its pixels
#pragma unroll
  for (int t = 0; t <= PRN_NORMAL_ERROR_MAX_T; ++t) c[t] = 0u;
  const int64_t p0 = (int64_t)blockIdx.x * ERR_PX;
#pragma unroll 4
  for (int j = 0; j < ERR_PX / ERR_TH; ++j) {
    const int64_t p = p0 + j * ERR_TH + threadIdx.x;
    const bool both = p < n && va[at + p] != 0 && vb[at + p] != 0;
    double d2 = 0.0;
    if (both) {
      d2 = err_d2(a + (at + p) * 3, b + (at + p) * 3);
      atomicAdd(&s_h[err_bin(d2)], 1u);
    }
    c[PRN_NORMAL_ERROR_MAX_T] += (unsigned)__popcll(__ballot(both));
#pragma unroll
    for (int t = 0; t < PRN_NORMAL_ERROR_MAX_T; ++t)
      if (t < T) c[t] += (unsigned)__popcll(__ballot(both && d2 <= thr.v[t]));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int t = 0; t <= PRN_NORMAL_ERROR_MAX_T; ++t) s_c[threadIdx.x >> 6][t] = c[t];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ERR_BINS; i += ERR_TH) {
    const unsigned h = s_h[i];
    if (h) atomicAdd(&hist[(size_t)img * ERR_BINS + i], (u64)h);
  }
  if (threadIdx.x <= PRN_NORMAL_ERROR_MAX_T) {
    const int t = threadIdx.x;
    const unsigned s = s_c[0][t] + s_c[1][t] + s_c[2][t] + s_c[3][t];
    if (s) {
      if (t == PRN_NORMAL_ERROR_MAX_T) atomicAdd(&count[img], (u64)s);
      else if (t < T) atomicAdd(&within[(size_t)img * T + t], (u64)s);
    }
  }
}

}  // namespace

extern "C" {

int prn_normals_block_pixels(void) { return NRM_PX; }
int prn_normal_error_bins(void) { return ERR_BINS; }

int prn_normals(const float* depth, const int* labels, const double* k, int B, int H, int W, int step, float lo, float hi, float max_gap, int flags,
                float* normals, unsigned char* valid, unsigned char* image, void* stream) {
  PRN_REQUIRE(H > 0 && W > 0 && B > 0 && B <= 65535, "prn_normals: sizes must be positive and B <= 65535 (B=%d H=%d W=%d)", B, H, W);
  PRN_REQUIRE((int64_t)H * W < (1LL << 24), "prn_normals: H * W = %lld must be below 2^24", (long long)((int64_t)H * W));
  PRN_REQUIRE(step >= 1, "prn_normals: step must be >= 1, got %d", step);
  PRN_REQUIRE(max_gap >= 0.f && max_gap <= 3.402823466e38f, "prn_normals: max_gap must be finite and >= 0, got %g", (double)max_gap);
  PRN_REQUIRE((flags & ~(PRN_NORMALS_RELATIVE | PRN_NORMALS_SAME_LABEL | PRN_NORMALS_PLANE_SIGN)) == 0, "prn_normals: unknown flags 0x%x", flags);
  PRN_REQUIRE(depth && k && normals && valid, "prn_normals: null argument");
  const nrm_in m = {depth, labels, k, H, W, H * W, step, lo, hi, max_gap, flags};
  normals_kernel<<<dim3(cdiv((int64_t)H * W, NRM_PX), B), NRM_PX, 0, (hipStream_t)stream>>>(m, normals, valid, image);
  PRN_CHECK_LAUNCH("prn_normals");
  return 0;
}

int prn_normal_error(const float* a, const unsigned char* valid_a, const float* b, const unsigned char* valid_b, int B, int64_t n, const double* thr2, int T,
                     int64_t* hist, int64_t* within, int64_t* count, void* stream) {
  PRN_REQUIRE(B > 0 && B <= 65535, "prn_normal_error: B must be in [1, 65535], got %d", B);
  PRN_REQUIRE(n > 0 && n < (1LL << 31), "prn_normal_error: n = %lld pixels an image must be in [1, 2^31)", (long long)n);
  PRN_REQUIRE(T >= 0 && T <= PRN_NORMAL_ERROR_MAX_T, "prn_normal_error: T must be in [0, %d], got %d", PRN_NORMAL_ERROR_MAX_T, T);
  PRN_REQUIRE(T == 0 || (thr2 && within), "prn_normal_error: T = %d thresholds without thr2 or within", T);
  PRN_REQUIRE(a && valid_a && b && valid_b && hist && count, "prn_normal_error: null argument");
  err_thr thr;
  for (int t = 0; t < PRN_NORMAL_ERROR_MAX_T; ++t) thr.v[t] = t < T ? thr2[t] : 0.0;
  normal_error_kernel<<<dim3(cdiv(n, ERR_PX), B), ERR_TH, 0, (hipStream_t)stream>>>(a, valid_a, b, valid_b, n, thr, T, (u64*)hist, (u64*)within, (u64*)count);
  PRN_CHECK_LAUNCH("prn_normal_error");
  return 0;
}

}  // extern "C"
