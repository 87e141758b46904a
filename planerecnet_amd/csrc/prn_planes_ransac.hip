// Robust plane fit of detected instances: RANSAC hypotheses scored per mask, least-squares refit on the inliers (include/prn.h:
// prn_planes_ransac_*).  The least-squares plane of prn_planes.hip takes every pixel under a mask; a mask that
// runs over a depth discontinuity tilts it.  Here every instance draws `hypotheses` three-point planes from its own mask, every
// hypothesis is tested against every pixel of the mask, and the existing moments + solve passes refit the inliers of the best one.
//   count    one lane per 16 mask bytes: set pixels per (instance, 64-pixel segment); also writes the pointer table of the inlier masks
//   scan     one workgroup per instance: exclusive prefix of its segment counts (rank -> segment by binary search)
//   sample   one lane per (instance, hypothesis): Philox4x32-10 -> three ranks -> three pixels -> the plane through them, or NaN
//   score    grid (64 x 16 pixel blocks, B, hypothesis chunks): the lane's 16 points stay in fp64 registers, the four waves take the
//            image's instances round robin; per hypothesis three FMAs and one compare per point, the compare masks are counted on the
//            scalar side; lane j keeps the count of hypothesis j of the chunk: ONE vector integer atomic per 64 hypotheses
//   select   one wave per instance: largest score, lowest index
//   classify the score kernel's shape with one plane per instance: writes the inlier bytes
//   refit    prn_planes_fit on the inlier masks (through the device-written pointer table), then classify + refit per refinement
//   finish   invalid instances: inlier mask zeroed, inliers 0, hypothesis -1, centroid NaN
// Integer atomics only; nothing depends on scheduling: bit-identical run to run and between a batched call and per-image calls (the
// draws are keyed by the instance's index within its image, the tile grid is per image).
#include <math.h>
#include "prn_masks.h"

namespace {

constexpr int RS_PX = 16;                     // pixels per lane: one 16-byte mask load
constexpr int RS_TILE = PRN_WAVE * RS_PX;     // pixels per workgroup tile
constexpr int RS_WAVES = 4;                   // waves per workgroup (instances round robin)
constexpr int RS_SEG = 64;                    // pixels per counted segment
constexpr int RS_CHUNK = 64;                  // hypotheses per chunk: one per lane of the atomic
constexpr int RS_MAX_HYP = 4096, RS_MAX_REFINE = 8;

// the last b with first[b] <= n (empty images are skipped)
__device__ __forceinline__ int image_of(const int* __restrict__ first, int B, int n) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= n) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Philox4x32-10 (Salmon et al., SC'11), as in prn_targets.hip: counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ void philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// byte k of p = bit k of bits for k < min(avail, 16); a byte at or past p + avail is never written, one 16-byte store only where the whole
// group is available and aligned (the writing counterpart of prn_mask_bits16)
__device__ __forceinline__ unsigned spread4(unsigned b) { return (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21); }
__device__ __forceinline__ void store_bits16(unsigned char* __restrict__ p, int64_t avail, unsigned bits) {
  if (__builtin_expect(avail >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0, 1)) {
    *reinterpret_cast<uint4*>(p) = make_uint4(spread4(bits), spread4(bits >> 4), spread4(bits >> 8), spread4(bits >> 12));
    return;
  }
#pragma clang loop unroll(disable)
  for (int k = 0; k < 16 && k < avail; ++k) p[k] = (unsigned char)((bits >> k) & 1u);
}

// grid (cdiv(cdiv(HW, 16), 256), min(Ntot, 65535)), 256 threads: segcnt [Ntot][nseg] = set pixels of each 64-pixel segment (four lanes each)
__global__ __launch_bounds__(256) void ransac_count_kernel(prn_mask_src src, int Ntot, int HW, int nseg, unsigned char* __restrict__ segcnt,
                                                           unsigned char** __restrict__ tab, unsigned char* inl) {
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int b = threadIdx.x; b < src.B; b += 256) tab[b] = inl + (size_t)src.first[b] * HW;      // image b's inlier masks, for the refit
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int64_t off = (int64_t)g * 16;
  for (int inst = blockIdx.y; inst < Ntot; inst += gridDim.y) {
    const unsigned char* m = prn_mask_ptr(src, inst, (size_t)HW);
    int c = off < HW ? __popc(prn_mask_bits16(m + off, HW - off)) : 0;
    c += __shfl_xor(c, 1);
    c += __shfl_xor(c, 2);
    if ((threadIdx.x & 3) == 0 && (g >> 2) < nseg) segcnt[(size_t)inst * nseg + (g >> 2)] = (unsigned char)c;
  }
}

// one workgroup per instance: segstart[inst][0 .. nseg] = exclusive prefix of segcnt[inst][.]
__global__ __launch_bounds__(256) void ransac_scan_kernel(const unsigned char* __restrict__ segcnt, int nseg, int* __restrict__ segstart) {
  const unsigned char* c = segcnt + (size_t)blockIdx.x * nseg;
  int* out = segstart + (size_t)blockIdx.x * (nseg + 1);
  const int per = (nseg + 255) / 256, beg = min(threadIdx.x * per, nseg), end = min(beg + per, nseg);
  int sum = 0;
  for (int i = beg; i < end; ++i) sum += c[i];
  __shared__ int sm[256];
  sm[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                           // inclusive scan of the 256 partial sums
    const int v = (int)threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
    __syncthreads();
    sm[threadIdx.x] += v;
    __syncthreads();
  }
  int run = sm[threadIdx.x] - sum;
  for (int i = beg; i < end; ++i) { out[i] = run; run += c[i]; }
  if (threadIdx.x == 255) out[nseg] = sm[255];
}

// one lane per (instance, hypothesis): hyp [Ntot][nhyp][4] = (nx, ny, nz, d) or NaN (degenerate)
__global__ __launch_bounds__(256) void ransac_sample_kernel(const float* __restrict__ depth, const unsigned char* const* __restrict__ masks,
                                                            const int* __restrict__ first, const double* __restrict__ K, const int* __restrict__ segstart,
                                                            int B, int Ntot, int nhyp, int W, int HW, int nseg, unsigned long long seed,
                                                            double* __restrict__ hyp) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)Ntot * nhyp) return;
  const int inst = (int)(t / nhyp), h = (int)(t - (int64_t)inst * nhyp);
  const int b = image_of(first, B, inst), local = inst - first[b];
  const unsigned char* m = masks[b] + (size_t)local * HW;
  const float* db = depth + (size_t)b * HW;
  const double* Kb = K + 9 * b;
  const double fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
  const int* st = segstart + (size_t)inst * (nseg + 1);
  const int count = st[nseg];
  double* out = hyp + t * 4;
  const double nan = __builtin_nan("");
  double P[3][3];
  bool ok = count > 0;
  if (ok) {
    unsigned rnd[4];
    philox((unsigned)h, 0u, (unsigned)local, 0u, (unsigned)seed, (unsigned)(seed >> 32), rnd);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int rank = (int)(((unsigned long long)rnd[j] * (unsigned long long)count) >> 32);      // < count
      int lo = 0, hi = nseg - 1;
      while (lo < hi) {                                         // the last segment whose first rank is <= rank (it holds a set pixel)
        const int mid = (lo + hi + 1) >> 1;
        if (st[mid] <= rank) lo = mid; else hi = mid - 1;
      }
      const int64_t s0 = (int64_t)lo * RS_SEG;
      unsigned long long bits = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) bits |= (unsigned long long)prn_mask_bits16(m + s0 + q * 16, HW - (s0 + q * 16)) << (q * 16);
      for (int k = rank - st[lo]; k > 0; --k) bits &= bits - 1;                                     // drop the k lower set bits
      int p = (int)s0 + __ffsll((long long)bits) - 1;
      p = p < 0 ? 0 : (p >= HW ? HW - 1 : p);                   // (never taken: the prefix and the bytes agree)
      const double z = (double)db[p];
      const int v = p / W, u = p - v * W;
      P[j][0] = ((double)u - cx) * z / fx;
      P[j][1] = ((double)v - cy) * z / fy;
      P[j][2] = z;
    }
  }
  double nx = nan, ny = nan, nz = nan, d = nan;
  if (ok) {
    const double ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
    const double bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
    const double qx = ay * bz - az * by, qy = az * bx - ax * bz, qz = ax * by - ay * bx;
    const double cc = qx * qx + qy * qy + qz * qz, aa = ax * ax + ay * ay + az * az, bb = bx * bx + by * by + bz * bz;
    if (cc > 1e-12 * (aa * bb)) {                               // (false on NaN: repeated / collinear draws, non-finite depth)
      const double len = sqrt(cc);
      nx = qx / len; ny = qy / len; nz = qz / len;
      d = nx * P[0][0] + ny * P[0][1] + nz * P[0][2];
    }
  }
  out[0] = nx; out[1] = ny; out[2] = nz; out[3] = d;
}

// the lane's 16 points, the arithmetic of planes_moments_kernel; bit k of the result = pixel k exists and has a finite depth
__device__ __forceinline__ unsigned load_points(const float* __restrict__ db, const double* __restrict__ Kb, int W, int HW, int p0, double (&X)[RS_PX],
                                                double (&Y)[RS_PX], double (&Z)[RS_PX]) {
  const double fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
  unsigned fin = 0;
#pragma unroll
  for (int k = 0; k < RS_PX; ++k) {
    const int p = p0 + k < HW ? p0 + k : HW - 1;
    const float zf = db[p];
    const double z = (double)zf;
    const int v = p / W, u = p - v * W;
    X[k] = ((double)u - cx) * z / fx;
    Y[k] = ((double)v - cy) * z / fy;
    Z[k] = z;
    if (p0 + k < HW && fabsf(zf) < INFINITY) fin |= 1u << k;
  }
  return fin;
}

// The score kernel's tile is a 64 x 16 pixel BLOCK of the image, not 1024 pixels in raster order: a hypothesis costs the same for every non-empty
// (tile, instance) pair, however few of the tile's pixels the mask holds, and a compact mask fills blocks several times better than row runs
// (measured on the bench input: 5.3 tests issued per test needed in raster tiles).  A lane holds 16 consecutive pixels of one row (x = 16 * (lane & 3),
// row = lane >> 2): the same 16-byte mask reads, 64 contiguous bytes per row.  Same arithmetic per point as load_points.
constexpr int RS_TW = 64, RS_TH = 16;
__device__ __forceinline__ unsigned load_points_block(const float* __restrict__ db, const double* __restrict__ Kb, int W, int H, int x, int y, double (&X)[RS_PX],
                                                      double (&Y)[RS_PX], double (&Z)[RS_PX]) {
  const double fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
  unsigned fin = 0;
#pragma unroll
  for (int k = 0; k < RS_PX; ++k) {
    const bool in = y < H && x + k < W;
    const float zf = db[in ? (size_t)y * W + x + k : 0];          // (outside the image: pixel 0, never counted)
    const double z = (double)zf;
    X[k] = ((double)(x + k) - cx) * z / fx;
    Y[k] = ((double)y - cy) * z / fy;
    Z[k] = z;
    if (in && fabsf(zf) < INFINITY) fin |= 1u << k;
  }
  return fin;
}

// grid (tiles_x * tiles_y, B, zsplit), 256 threads.  score [Ntot][nhyp] zeroed by the caller.  The instance index and the hypothesis index are
// wave-uniform: the plane comes through scalar loads, the next one in flight; the 16 compare masks are ANDed with the instance's ballots and counted
// in SGPRs.
template <bool REL>
__global__ __launch_bounds__(256) void ransac_score_kernel(const float* __restrict__ depth, const unsigned char* const* __restrict__ masks,
                                                           const int* __restrict__ first, const double* __restrict__ K, const double* __restrict__ hyp,
                                                           int W, int H, int tiles_x, int nhyp, int nchunks, double thr, int* __restrict__ score) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i0 = first[b], nb = first[b + 1] - i0;
  if (wave >= nb) return;
  const unsigned char* mb = masks[b];
  const int HW = H * W, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * RS_TW + (lane & 3) * RS_PX, y = ty * RS_TH + (lane >> 2);
  const int avail = y < H ? W - x : 0;                            // bytes of the lane's row segment inside the image (<= 0: none, nothing is read)
  const int p0 = avail > 0 ? y * W + x : 0;
  double X[RS_PX], Y[RS_PX], Z[RS_PX];
  // (back-projecting only at a wave's first non-empty pair was tried: the conditional initialisation costs 97 more VGPRs and an occupancy step,
  //  score kernel 1232 -> 2173 us at B = 8)
  const unsigned fin = load_points_block(depth + (size_t)b * HW, K + 9 * b, W, H, x, y, X, Y, Z);
  unsigned cur = prn_mask_bits16(mb + (size_t)wave * HW + p0, avail);
  for (int i = wave; i < nb; i += RS_WAVES) {
    const unsigned bits = cur & fin;                              // a pixel without a finite depth is never an inlier
    cur = i + RS_WAVES < nb ? prn_mask_bits16(mb + (size_t)(i + RS_WAVES) * HW + p0, avail) : 0u;      // next instance's bytes in flight
    if (!__any(bits != 0u)) continue;                             // wave-uniform: nothing of this instance in the tile
    unsigned long long bm[RS_PX];
#pragma unroll
    for (int k = 0; k < RS_PX; ++k) bm[k] = __ballot((bits >> k) & 1u);
    for (int c = blockIdx.z; c < nchunks; c += gridDim.z) {
      const int h0 = c * RS_CHUNK, nh = min(RS_CHUNK, nhyp - h0);
      const double* hp = hyp + ((size_t)(i0 + i) * nhyp + h0) * 4;
      double nx = hp[0], ny = hp[1], nz = hp[2], d = hp[3];
      int mine = 0;
      for (int j = 0; j < nh; ++j) {
        const double* hn = hp + 4 * (j + 1 < nh ? j + 1 : j);     // the next plane, loaded under this one's tests
        const double ax = hn[0], ay = hn[1], az = hn[2], ad = hn[3];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < RS_PX; ++k) {
          const double r = fma(nz, Z[k], fma(ny, Y[k], fma(nx, X[k], -d)));
          const double t = REL ? thr * Z[k] : thr;
          cnt += __popcll(__ballot(fabs(r) <= t) & bm[k]);
        }
        if (lane == j) mine = cnt;
        nx = ax; ny = ay; nz = az; d = ad;
      }
      if (lane < nh && mine > 0) atomicAdd(score + (size_t)(i0 + i) * nhyp + h0 + lane, mine);    // integers: order-independent
    }
  }
}

// grid cdiv(Ntot, 4), 256 threads: one wave per instance.  The chosen plane goes to planes[] (what classify reads), the mask's pixel count to count[].
__global__ __launch_bounds__(256) void ransac_select_kernel(const int* __restrict__ score, const double* __restrict__ hyp, const int* __restrict__ segstart,
                                                            int Ntot, int nhyp, int nseg, double* __restrict__ planes, int* __restrict__ hypothesis,
                                                            long long* __restrict__ count) {
  const int inst = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (inst >= Ntot) return;                                       // wave-uniform
  int best = -1, bh = 0x7fffffff;
  for (int h = lane; h < nhyp; h += PRN_WAVE) {
    const int s = score[(size_t)inst * nhyp + h];
    if (s > best) { best = s; bh = h; }                           // ascending h: the lowest index of the lane's largest score
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int ob = __shfl_xor(best, off), oh = __shfl_xor(bh, off);
    if (ob > best || (ob == best && oh < bh)) { best = ob; bh = oh; }
  }
  if (lane != 0) return;
  const bool ok = best >= 3;
  const double nan = __builtin_nan("");
  const double* q = hyp + ((size_t)inst * nhyp + (ok ? bh : 0)) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) planes[4 * (size_t)inst + k] = ok ? q[k] : nan;
  hypothesis[inst] = ok ? bh : -1;
  count[inst] = segstart[(size_t)inst * (nseg + 1) + nseg];
}

// grid (ntiles, B), 256 threads: inl [Ntot][HW] = 1 where the pixel is in the mask and within t of planes[instance] (a NaN plane: all zero)
template <bool REL>
__global__ __launch_bounds__(256) void ransac_classify_kernel(const float* __restrict__ depth, const unsigned char* const* __restrict__ masks,
                                                              const int* __restrict__ first, const double* __restrict__ K, const double* __restrict__ planes,
                                                              int W, int HW, double thr, unsigned char* __restrict__ inl) {
  const int b = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i0 = first[b], nb = first[b + 1] - i0;
  if (wave >= nb) return;
  const unsigned char* mb = masks[b];
  const int p0 = tile * RS_TILE + lane * RS_PX;
  double X[RS_PX], Y[RS_PX], Z[RS_PX];
  const unsigned fin = load_points(depth + (size_t)b * HW, K + 9 * b, W, HW, p0, X, Y, Z);
  unsigned cur = prn_mask_bits16(mb + (size_t)wave * HW + p0, HW - p0);
  for (int i = wave; i < nb; i += RS_WAVES) {
    const unsigned bits = cur & fin;
    cur = i + RS_WAVES < nb ? prn_mask_bits16(mb + (size_t)(i + RS_WAVES) * HW + p0, HW - p0) : 0u;
    unsigned in = 0;
    if (__any(bits != 0u)) {
      const double* pl = planes + 4 * (size_t)(i0 + i);
      const double nx = pl[0], ny = pl[1], nz = pl[2], d = pl[3];
#pragma unroll
      for (int k = 0; k < RS_PX; ++k) {
        const double r = fma(nz, Z[k], fma(ny, Y[k], fma(nx, X[k], -d)));
        const double t = REL ? thr * Z[k] : thr;
        in |= (fabs(r) <= t ? 1u : 0u) << k;
      }
      in &= bits;
    }
    store_bits16(inl + (size_t)(i0 + i) * HW + p0, (int64_t)HW - p0, in);
  }
}

// grid (cdiv(cdiv(HW, 16), 256), min(Ntot, 65535)), 256 threads: the outputs of invalid instances
__global__ __launch_bounds__(256) void ransac_finish_kernel(const unsigned char* __restrict__ valid, int Ntot, int HW, unsigned char* __restrict__ inl,
                                                            long long* __restrict__ inliers, int* __restrict__ hypothesis, double* __restrict__ centroid) {
  const int64_t off = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  for (int inst = blockIdx.y; inst < Ntot; inst += gridDim.y) {
    if (valid[inst]) continue;
    if (off < HW) store_bits16(inl + (size_t)inst * HW + off, HW - off, 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const double nan = __builtin_nan("");
      inliers[inst] = 0;
      hypothesis[inst] = -1;
      centroid[3 * (size_t)inst + 0] = nan; centroid[3 * (size_t)inst + 1] = nan; centroid[3 * (size_t)inst + 2] = nan;
    }
  }
}

bool ransac_sizes_ok(int B, int Ntot, int H, int W, int hypotheses) {
  return hypotheses >= 1 && hypotheses <= RS_MAX_HYP && Ntot >= 0 && H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) - 2 * RS_TILE &&
         (int64_t)Ntot * hypotheses < (1LL << 31) && prn_planes_ws_bytes(B, Ntot, H, W) >= 0;
}

// ws = segment counts | their prefixes | hypotheses | scores | pointer table of the inlier masks | the refit's prn_planes_fit workspace
struct Layout {
  int64_t segcnt, segstart, hyp, score, tab, fit, total;
};

Layout layout(int B, int Ntot, int H, int W, int hypotheses) {
  const int64_t nseg = cdiv((int64_t)H * W, RS_SEG);
  Layout l;
  l.segcnt = 0;
  l.segstart = l.segcnt + (int64_t)prn_align256((size_t)(Ntot * nseg));
  l.hyp = l.segstart + (int64_t)prn_align256((size_t)(Ntot * (nseg + 1)) * sizeof(int));
  l.score = l.hyp + (int64_t)prn_align256((size_t)Ntot * hypotheses * 4 * sizeof(double));
  l.tab = l.score + (int64_t)prn_align256((size_t)Ntot * hypotheses * sizeof(int));
  l.fit = l.tab + (int64_t)prn_align256((size_t)B * sizeof(void*));
  l.total = l.fit + prn_planes_ws_bytes(B, Ntot, H, W);
  return l;
}

}  // namespace

extern "C" int64_t prn_planes_ransac_ws_bytes(int B, int Ntot, int H, int W, int hypotheses) {
  if (!ransac_sizes_ok(B, Ntot, H, W, hypotheses)) return -1;
  return layout(B, Ntot, H, W, hypotheses).total;
}

extern "C" int prn_planes_ransac_fit(const float* depth, const unsigned char* const* masks_dev, const int* first_dev, const double* k_dev, int B, int Ntot,
                                     int H, int W, double threshold, int relative, int hypotheses, int refine, unsigned long long seed, double* planes,
                                     double* centroid, unsigned char* valid, int64_t* count, int64_t* inliers, int* hypothesis,
                                     unsigned char* inlier_masks, void* ws, void* stream) {
  PRN_REQUIRE(hypotheses >= 1 && hypotheses <= RS_MAX_HYP, "prn_planes_ransac_fit: hypotheses must be 1 .. %d (got %d)", RS_MAX_HYP, hypotheses);
  PRN_REQUIRE(refine >= 0 && refine <= RS_MAX_REFINE, "prn_planes_ransac_fit: refine must be 0 .. %d (got %d)", RS_MAX_REFINE, refine);
  PRN_REQUIRE(threshold > 0.0 && threshold < (double)INFINITY, "prn_planes_ransac_fit: threshold must be positive and finite (got %g)", threshold);
  PRN_REQUIRE(ransac_sizes_ok(B, Ntot, H, W, hypotheses), "prn_planes_ransac_fit: bad sizes (B=%d Ntot=%d H=%d W=%d hypotheses=%d)", B, Ntot, H, W, hypotheses);
  PRN_REQUIRE(depth && masks_dev && first_dev && k_dev && ws, "prn_planes_ransac_fit: null depth / masks / first / K / workspace");
  PRN_REQUIRE(Ntot == 0 || (planes && centroid && valid && count && inliers && hypothesis && inlier_masks), "prn_planes_ransac_fit: null output");
  PRN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "prn_planes_ransac_fit: workspace must be 16-byte aligned");
  if (Ntot == 0) return 0;                                        // no instance: no output to write
  const int HW = H * W, ntiles = cdiv(HW, RS_TILE), nseg = cdiv(HW, RS_SEG), ngroups = cdiv(HW, 16);
  const Layout l = layout(B, Ntot, H, W, hypotheses);
  char* base = static_cast<char*>(ws);
  unsigned char* segcnt = reinterpret_cast<unsigned char*>(base + l.segcnt);
  int* segstart = reinterpret_cast<int*>(base + l.segstart);
  double* hyp = reinterpret_cast<double*>(base + l.hyp);
  int* score = reinterpret_cast<int*>(base + l.score);
  unsigned char** tab = reinterpret_cast<unsigned char**>(base + l.tab);
  hipStream_t st = (hipStream_t)stream;
  const prn_mask_src src{masks_dev, first_dev, B, nullptr};
  const int ny = Ntot < 65535 ? Ntot : 65535;
  if (hipMemsetAsync(score, 0, (size_t)Ntot * hypotheses * sizeof(int), st) != hipSuccess) { prn_set_error("prn_planes_ransac_fit: memset failed"); return 1; }
  hipLaunchKernelGGL(ransac_count_kernel, dim3(cdiv(ngroups, 256), ny), dim3(256), 0, st, src, Ntot, HW, nseg, segcnt, tab, inlier_masks);
  PRN_CHECK_LAUNCH("prn_planes_ransac_fit/count");
  hipLaunchKernelGGL(ransac_scan_kernel, dim3(Ntot), dim3(256), 0, st, (const unsigned char*)segcnt, nseg, segstart);
  PRN_CHECK_LAUNCH("prn_planes_ransac_fit/scan");
  hipLaunchKernelGGL(ransac_sample_kernel, dim3(cdiv((int64_t)Ntot * hypotheses, 256)), dim3(256), 0, st, depth, masks_dev, first_dev, k_dev,
                     (const int*)segstart, B, Ntot, hypotheses, W, HW, nseg, seed, hyp);
  PRN_CHECK_LAUNCH("prn_planes_ransac_fit/sample");
  // a workgroup's time is proportional to the non-empty instances of its block, so the launch wants many more workgroups than the GPU runs at once:
  // the hypothesis chunks spread over grid z up to about 8192 workgroups (measured at B = 8: 1574 -> 1232 us from 2400 to 9600; the scores do not
  // depend on the split)
  const int nchunks = cdiv(hypotheses, RS_CHUNK);
  const int tiles_x = cdiv(W, RS_TW), blocks = tiles_x * cdiv(H, RS_TH);
  int zsplit = cdiv(8192, (int64_t)blocks * B);
  zsplit = zsplit < 1 ? 1 : (zsplit > nchunks ? nchunks : zsplit);
  if (relative)
    hipLaunchKernelGGL(ransac_score_kernel<true>, dim3(blocks, B, zsplit), dim3(256), 0, st, depth, masks_dev, first_dev, k_dev, (const double*)hyp, W, H,
                       tiles_x, hypotheses, nchunks, threshold, score);
  else
    hipLaunchKernelGGL(ransac_score_kernel<false>, dim3(blocks, B, zsplit), dim3(256), 0, st, depth, masks_dev, first_dev, k_dev, (const double*)hyp, W, H,
                       tiles_x, hypotheses, nchunks, threshold, score);
  PRN_CHECK_LAUNCH("prn_planes_ransac_fit/score");
  hipLaunchKernelGGL(ransac_select_kernel, dim3(cdiv(Ntot, 4)), dim3(256), 0, st, (const int*)score, (const double*)hyp, (const int*)segstart, Ntot, hypotheses,
                     nseg, planes, hypothesis, reinterpret_cast<long long*>(count));
  PRN_CHECK_LAUNCH("prn_planes_ransac_fit/select");
  for (int r = 0; r <= refine; ++r) {                             // S_r from P_{r-1} (r = 0: from the chosen hypothesis), then P_r
    if (relative)
      hipLaunchKernelGGL(ransac_classify_kernel<true>, dim3(ntiles, B), dim3(256), 0, st, depth, masks_dev, first_dev, k_dev, (const double*)planes, W, HW,
                         threshold, inlier_masks);
    else
      hipLaunchKernelGGL(ransac_classify_kernel<false>, dim3(ntiles, B), dim3(256), 0, st, depth, masks_dev, first_dev, k_dev, (const double*)planes, W, HW,
                         threshold, inlier_masks);
    PRN_CHECK_LAUNCH("prn_planes_ransac_fit/classify");
    const int rc = prn_planes_fit(depth, (const unsigned char* const*)tab, first_dev, k_dev, B, Ntot, H, W, planes, centroid, valid, inliers, base + l.fit, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(ransac_finish_kernel, dim3(cdiv(ngroups, 256), ny), dim3(256), 0, st, (const unsigned char*)valid, Ntot, HW, inlier_masks,
                     reinterpret_cast<long long*>(inliers), hypothesis, centroid);
  PRN_CHECK_LAUNCH("prn_planes_ransac_fit/finish");
  return 0;
}
