// Plane parameters of detected instances and the planar depth map (include/prn.h: prn_planes_*).
// The reference derives them in its iBims-1 "plane depth" exporter (simple_inference.py:240-324, PCA_svd of
// models/functions/funcs.py:287-291) with a Python loop over the instances: boolean indexing, torch.svd and torch.where per
// instance, one device -> host round trip each.  Here a whole ragged batch is three launches:
//   moments  grid (tiles, B): one 1024-pixel tile of one image per workgroup, its four waves take the image's instances round
//            robin; every mask byte is read once (16 per lane: prn_masks.h), the depth once per tile.  Per (instance, tile): count, mean and
//            centred scatter in fp64 -- two passes over the lane's 16 points, then Chan's pairwise update across the wave in a
//            fixed butterfly order.  The same pass writes the owner map (highest covering instance index per pixel).
//   solve    one wave per instance: the tile partials merged in index order (lane-strided, then the same butterfly), a cyclic
//            Jacobi 3x3 eigensolve in fp64, the normal of the smallest eigenvalue.
//   render   one pixel per lane: the owner's plane evaluated along the pixel's ray, optional (lo, hi) -> NaN epilogue.
// No atomics on floating-point values and no order that depends on scheduling: results are bit-identical run to run and
// between a batched call and per-image calls (an instance's partials depend only on its own image and the tile grid).
#include "prn_masks.h"

namespace {

constexpr int PL_PX = 16;                     // pixels per lane: one 16-byte mask load
constexpr int PL_TILE = PRN_WAVE * PL_PX;     // pixels per workgroup tile
constexpr int PL_WAVES = 4;                   // waves per moments workgroup (instances round robin)
constexpr int PL_STATS = 10;                  // count, mean x y z, centred scatter xx xy xz yy yz zz

struct Mom {
  double n, mx, my, mz, sxx, sxy, sxz, syy, syz, szz;
};

__device__ __forceinline__ Mom mom_zero() { return Mom{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// a <- a merged with b (Chan et al.): exact in the counts, the scatter stays centred
__device__ __forceinline__ void chan_merge(Mom& a, const Mom& b) {
  if (b.n == 0.0) return;
  if (a.n == 0.0) { a = b; return; }
  const double n = a.n + b.n, inv = 1.0 / n;
  const double dx = b.mx - a.mx, dy = b.my - a.my, dz = b.mz - a.mz;
  const double wb = b.n * inv, f = a.n * wb;
  a.mx += dx * wb; a.my += dy * wb; a.mz += dz * wb;
  a.sxx += b.sxx + dx * dx * f; a.sxy += b.sxy + dx * dy * f; a.sxz += b.sxz + dx * dz * f;
  a.syy += b.syy + dy * dy * f; a.syz += b.syz + dy * dz * f; a.szz += b.szz + dz * dz * f;
  a.n = n;
}

// fixed butterfly over the 64 lanes; lane 0 holds the result (other lanes merge in a different order and are not used)
__device__ __forceinline__ void wave_merge(Mom& m) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Mom o;
    o.n = __shfl_xor(m.n, off); o.mx = __shfl_xor(m.mx, off); o.my = __shfl_xor(m.my, off); o.mz = __shfl_xor(m.mz, off);
    o.sxx = __shfl_xor(m.sxx, off); o.sxy = __shfl_xor(m.sxy, off); o.sxz = __shfl_xor(m.sxz, off);
    o.syy = __shfl_xor(m.syy, off); o.syz = __shfl_xor(m.syz, off); o.szz = __shfl_xor(m.szz, off);
    chan_merge(m, o);
  }
}

// grid (ntiles, B), 256 threads.  part [Ntot][ntiles][PL_STATS] (an empty pair writes only its count), owner [B][HW].
__global__ __launch_bounds__(256) void planes_moments_kernel(const float* __restrict__ depth, const unsigned char* const* __restrict__ masks,
                                                             const int* __restrict__ first, const double* __restrict__ K, int W, int HW, int ntiles,
                                                             double* __restrict__ part, int* __restrict__ owner) {
  __shared__ int own[PL_TILE];
  const int b = blockIdx.y, tile = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i0 = first[b], nb = first[b + 1] - i0;
  const unsigned char* mb = masks[b];
  for (int k = threadIdx.x; k < PL_TILE; k += 256) own[k] = -1;
  const double* Kb = K + 9 * b;
  const double fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
  const int p0 = tile * PL_TILE + lane * PL_PX;
  const float* db = depth + (size_t)b * HW;
  // the lane's points, the reference's fp64 arithmetic: X = (u - cx) * Z / fx, Y = (v - cy) * Z / fy (integer pixel indices)
  double X[PL_PX], Y[PL_PX], Z[PL_PX];
  int ow[PL_PX];
#pragma unroll
  for (int k = 0; k < PL_PX; ++k) {
    const int p = p0 + k < HW ? p0 + k : HW - 1;
    const double z = (double)db[p];
    const int v = p / W, u = p - v * W;
    X[k] = ((double)u - cx) * z / fx;
    Y[k] = ((double)v - cy) * z / fy;
    Z[k] = z;
    ow[k] = -1;
  }
  unsigned cur = wave < nb ? prn_mask_bits16(mb + (size_t)wave * HW + p0, HW - p0) : 0u;
  for (int i = wave; i < nb; i += PL_WAVES) {
    const unsigned bits = cur;
    cur = i + PL_WAVES < nb ? prn_mask_bits16(mb + (size_t)(i + PL_WAVES) * HW + p0, HW - p0) : 0u;      // next instance's bytes in flight
    double* dst = part + ((size_t)(i0 + i) * ntiles + tile) * PL_STATS;
    if (!__any(bits != 0u)) {                                     // wave-uniform: nothing of this instance in the tile
      if (lane == 0) dst[0] = 0.0;
      continue;
    }
    Mom m = mom_zero();
    double sx = 0, sy = 0, sz = 0;
#pragma unroll
    for (int k = 0; k < PL_PX; ++k)
      if ((bits >> k) & 1u) { m.n += 1.0; sx += X[k]; sy += Y[k]; sz += Z[k]; ow[k] = i; }
    if (m.n > 0.0) {
      m.mx = sx / m.n; m.my = sy / m.n; m.mz = sz / m.n;
#pragma unroll
      for (int k = 0; k < PL_PX; ++k)
        if ((bits >> k) & 1u) {
          const double dx = X[k] - m.mx, dy = Y[k] - m.my, dz = Z[k] - m.mz;
          m.sxx += dx * dx; m.sxy += dx * dy; m.sxz += dx * dz; m.syy += dy * dy; m.syz += dy * dz; m.szz += dz * dz;
        }
    }
    wave_merge(m);
    if (lane == 0) {
      dst[0] = m.n; dst[1] = m.mx; dst[2] = m.my; dst[3] = m.mz; dst[4] = m.sxx;
      dst[5] = m.sxy; dst[6] = m.sxz; dst[7] = m.syy; dst[8] = m.syz; dst[9] = m.szz;
    }
  }
  __syncthreads();                                                // own[] initialised
#pragma unroll
  for (int k = 0; k < PL_PX; ++k)
    if (ow[k] >= 0) atomicMax(&own[lane * PL_PX + k], ow[k]);     // max of integers: order-independent
  __syncthreads();
  int* ob = owner + (size_t)b * HW;
  for (int k = threadIdx.x; k < PL_TILE; k += 256) {
    const int p = tile * PL_TILE + k;
    if (p < HW) ob[p] = own[k];
  }
}

// one Jacobi rotation zeroing a[p][q] (a symmetric, v accumulates the rotations: its columns are the eigenvectors)
template <int p, int q>
__device__ __forceinline__ void jacobi_rot(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double akp = a[k][p], akq = a[k][q];
    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double apk = a[p][k], aqk = a[q][k];
    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
  }
  a[p][q] = a[q][p] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = v[k][p], vkq = v[k][q];
    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
  }
}

// grid cdiv(Ntot, 4), 256 threads: one wave per instance
__global__ __launch_bounds__(256) void planes_solve_kernel(const double* __restrict__ part, int Ntot, int ntiles, double* __restrict__ planes,
                                                           double* __restrict__ centroid, unsigned char* __restrict__ valid, long long* __restrict__ count) {
  const int inst = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (inst >= Ntot) return;                                       // wave-uniform
  Mom m = mom_zero();
  for (int t = lane; t < ntiles; t += PRN_WAVE) {
    const double* q = part + ((size_t)inst * ntiles + t) * PL_STATS;
    if (q[0] == 0.0) continue;
    const Mom o{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]};
    chan_merge(m, o);
  }
  wave_merge(m);
  if (lane != 0) return;
  double a[3][3] = {{m.sxx, m.sxy, m.sxz}, {m.sxy, m.syy, m.syz}, {m.sxz, m.syz, m.szz}};
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double dg = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (!(off > 1e-36 * dg)) break;                               // (also ends on NaN)
    jacobi_rot<0, 1>(a, v);
    jacobi_rot<0, 2>(a, v);
    jacobi_rot<1, 2>(a, v);
  }
  const double e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
  const int imin = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);
  const double emax = fmax(e0, fmax(e1, e2));
  const double emid = imin == 0 ? fmin(e1, e2) : (imin == 1 ? fmin(e0, e2) : fmin(e0, e1));
  double nx = imin == 0 ? v[0][0] : (imin == 1 ? v[0][1] : v[0][2]);
  double ny = imin == 0 ? v[1][0] : (imin == 1 ? v[1][1] : v[1][2]);
  double nz = imin == 0 ? v[2][0] : (imin == 1 ? v[2][1] : v[2][2]);
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  nx /= len; ny /= len; nz /= len;
  double d = m.mx * nx + m.my * ny + m.mz * nz;
  if (d < 0.0) { nx = -nx; ny = -ny; nz = -nz; d = -d; }
  const bool ok = m.n >= 3.0 && emid > 1e-12 * emax;              // fewer than 3 points or a degenerate scatter (collinear): no plane
  const double nan = __builtin_nan("");
  planes[4 * inst + 0] = ok ? nx : nan;
  planes[4 * inst + 1] = ok ? ny : nan;
  planes[4 * inst + 2] = ok ? nz : nan;
  planes[4 * inst + 3] = ok ? d : nan;
  centroid[3 * inst + 0] = m.n > 0.0 ? m.mx : nan;
  centroid[3 * inst + 1] = m.n > 0.0 ? m.my : nan;
  centroid[3 * inst + 2] = m.n > 0.0 ? m.mz : nan;
  valid[inst] = ok ? 1 : 0;
  count[inst] = (long long)m.n;
}

// grid (cdiv(HW, 256), B), 256 threads: one pixel per lane
__global__ __launch_bounds__(256) void planes_render_kernel(const float* __restrict__ depth, const unsigned char* const* __restrict__ masks,
                                                            const int* __restrict__ first, const double* __restrict__ K, const double* __restrict__ planes,
                                                            const unsigned char* __restrict__ valid, const int* __restrict__ owner, int W, int HW,
                                                            int has_range, float lo, float hi, float* __restrict__ out) {
  __shared__ double kinv[9];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {                                         // K^-1 by the adjugate, fp64
    const double* k = K + 9 * b;
    const double c00 = k[4] * k[8] - k[5] * k[7], c01 = k[5] * k[6] - k[3] * k[8], c02 = k[3] * k[7] - k[4] * k[6];
    const double id = 1.0 / (k[0] * c00 + k[1] * c01 + k[2] * c02);
    kinv[0] = c00 * id; kinv[1] = (k[2] * k[7] - k[1] * k[8]) * id; kinv[2] = (k[1] * k[5] - k[2] * k[4]) * id;
    kinv[3] = c01 * id; kinv[4] = (k[0] * k[8] - k[2] * k[6]) * id; kinv[5] = (k[2] * k[3] - k[0] * k[5]) * id;
    kinv[6] = c02 * id; kinv[7] = (k[1] * k[6] - k[0] * k[7]) * id; kinv[8] = (k[0] * k[4] - k[1] * k[3]) * id;
  }
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const size_t g = (size_t)b * HW + p;
  float z = depth[g];
  int o = owner[g];
  const int i0 = first[b];
  if (o >= 0 && !valid[i0 + o]) {                                 // rare: the next valid instance below that covers the pixel
    const unsigned char* mb = masks[b];
    do {
      --o;
      while (o >= 0 && mb[(size_t)o * HW + p] == 0) --o;
    } while (o >= 0 && !valid[i0 + o]);
  }
  if (o >= 0) {
    const double* pl = planes + 4 * (size_t)(i0 + o);
    const int v = p / W, u = p - v * W;
    const double rx = kinv[0] * u + kinv[1] * v + kinv[2], ry = kinv[3] * u + kinv[4] * v + kinv[5], rz = kinv[6] * u + kinv[7] * v + kinv[8];
    z = (float)(pl[3] / (pl[0] * rx + pl[1] * ry + pl[2] * rz));
  }
  if (has_range && !(z > lo && z < hi)) z = __builtin_nanf("");
  out[g] = z;
}

// ws = the per-(instance, tile) partials | the owner map (sizes_ok: positive and far below 2^63)
inline int64_t pl_part_bytes(int64_t Ntot, int64_t ntiles) { return (int64_t)prn_align256((size_t)(Ntot * ntiles * PL_STATS) * sizeof(double)); }

bool sizes_ok(int B, int Ntot, int H, int W) {
  return B > 0 && B < 65536 && Ntot >= 0 && H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) && (int64_t)B * H * W < (1LL << 40) &&
         (int64_t)Ntot * cdiv((int64_t)H * W, PL_TILE) < (1LL << 40);
}

}  // namespace

extern "C" int64_t prn_planes_ws_bytes(int B, int Ntot, int H, int W) {
  if (!sizes_ok(B, Ntot, H, W)) return -1;
  const int64_t HW = (int64_t)H * W, ntiles = cdiv(HW, PL_TILE);
  return pl_part_bytes(Ntot, ntiles) + (int64_t)prn_align256((size_t)B * HW * sizeof(int));
}

extern "C" int prn_planes_fit(const float* depth, const unsigned char* const* masks_dev, const int* first_dev, const double* k_dev, int B, int Ntot,
                              int H, int W, double* planes, double* centroid, unsigned char* valid, int64_t* count, void* ws, void* stream) {
  PRN_REQUIRE(sizes_ok(B, Ntot, H, W), "prn_planes_fit: bad sizes (B=%d Ntot=%d H=%d W=%d)", B, Ntot, H, W);
  PRN_REQUIRE(depth && masks_dev && first_dev && k_dev && ws, "prn_planes_fit: null depth / masks / first / K / workspace");
  PRN_REQUIRE(Ntot == 0 || (planes && centroid && valid && count), "prn_planes_fit: null output");
  PRN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "prn_planes_fit: workspace must be 16-byte aligned");
  const int HW = H * W, ntiles = cdiv(HW, PL_TILE);
  double* part = static_cast<double*>(ws);
  int* owner = reinterpret_cast<int*>(static_cast<char*>(ws) + pl_part_bytes(Ntot, ntiles));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(planes_moments_kernel, dim3(ntiles, B), dim3(256), 0, st, depth, masks_dev, first_dev, k_dev, W, HW, ntiles, part, owner);
  PRN_CHECK_LAUNCH("prn_planes_fit/moments");
  if (Ntot > 0) {
    hipLaunchKernelGGL(planes_solve_kernel, dim3(cdiv(Ntot, 4)), dim3(256), 0, st, (const double*)part, Ntot, ntiles, planes, centroid, valid,
                       reinterpret_cast<long long*>(count));
    PRN_CHECK_LAUNCH("prn_planes_fit/solve");
  }
  return 0;
}

extern "C" int prn_planes_render(const float* depth, const unsigned char* const* masks_dev, const int* first_dev, const double* k_dev, const double* planes,
                                 const unsigned char* valid, int B, int Ntot, int H, int W, int has_range, float lo, float hi, float* out, const void* ws,
                                 void* stream) {
  PRN_REQUIRE(sizes_ok(B, Ntot, H, W), "prn_planes_render: bad sizes (B=%d Ntot=%d H=%d W=%d)", B, Ntot, H, W);
  PRN_REQUIRE(depth && masks_dev && first_dev && k_dev && ws && out, "prn_planes_render: null depth / masks / first / K / workspace / output");
  PRN_REQUIRE(Ntot == 0 || (planes && valid), "prn_planes_render: null planes / valid");
  PRN_REQUIRE(!has_range || lo < hi, "prn_planes_render: empty depth range (lo=%g hi=%g)", (double)lo, (double)hi);
  PRN_REQUIRE(out != depth, "prn_planes_render: the output must not alias the input depth");
  const int HW = H * W, ntiles = cdiv(HW, PL_TILE);
  const int* owner = reinterpret_cast<const int*>(static_cast<const char*>(ws) + pl_part_bytes(Ntot, ntiles));
  hipLaunchKernelGGL(planes_render_kernel, dim3(cdiv(HW, 256), B), dim3(256), 0, (hipStream_t)stream, depth, masks_dev, first_dev, k_dev, planes, valid,
                     owner, W, HW, has_range, lo, hi, out);
  PRN_CHECK_LAUNCH("prn_planes_render");
  return 0;
}
