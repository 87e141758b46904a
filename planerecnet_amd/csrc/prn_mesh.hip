// Triangle mesh and point cloud of a depth map (include/prn.h: prn_mesh).  A pixel with a usable depth becomes a vertex,
// the two triangles of a pixel quad are kept where their corners are vertices of one label and close in depth: a stream compaction whose outputs
// are exact integers (ids, faces) and once-rounded fp64 products (positions), so numpy restates all of it bit for bit.
//   count     one workgroup per MESH_PX consecutive pixels (row-major) of one image: a thread takes one pixel, the flags of a wave are two 64-bit
//             ballots, their popcounts summed over the four waves give cells[image][workgroup] = (vertices, triangles)
//   scan      one workgroup per image: cells <- their exclusive scan in workgroup order (chunks of MESH_CHUNK cells with a carry), totals to counts
//   vertices  the flags again; a vertex's id = its workgroup's offset + its rank among the workgroup's valid pixels (ballot, popcount below the
//             lane, the waves' totals before it).  The id map is written as it is computed; positions and colours are staged in LDS at their
//             rank and leave as whole dwords, consecutive lanes on consecutive dwords (12-byte records would otherwise be three strided stores
//             per lane; the colours' first and last bytes outside a 4-byte boundary go as bytes)
//   faces     the triangle flags again, the four ids of the quad from the id map, the records staged in LDS and stored the same way
// The image is the grid's y, so a batch costs the launches of one image.  No workgroup waits for another, there is no atomic, placement is
// integer arithmetic on counts every launch recomputes from the same untouched inputs: results are identical run to run.
#include "prn_common.h"

namespace {

typedef unsigned long long u64;

constexpr int MESH_PX = 256;                     // pixels (= threads) of one workgroup
constexpr int MESH_CHUNK = 256;                  // cells one step of the scan takes
static_assert(MESH_PX == 256 && MESH_CHUNK == 256, "four waves a workgroup: the wave totals below are four words");

struct mesh_in {
  const float* depth;                            // [B][H][W]
  const int* labels;                             // [B][H][W] or NULL (all 0)
  int H, W, HW;
  float lo, hi, gap;
  int flags;
};

struct mesh_px { bool valid, t0, t1; float z; int lab; };

__device__ __forceinline__ bool mesh_valid(const mesh_in& m, float z, int lab) {
  return __builtin_isfinite(z) && m.lo < z && z < m.hi && (!(m.flags & PRN_MESH_PLANAR_ONLY) || lab > 0);
}

// three valid corners: one label (if asked) and zmax - zmin <= gap (x zmin if relative), every operation rounded to fp32 on its own
__device__ __forceinline__ bool mesh_tri(const mesh_in& m, float z0, float z1, float z2, int l0, int l1, int l2) {
  if ((m.flags & PRN_MESH_SAME_LABEL) && !(l0 == l1 && l1 == l2)) return false;
  const float zmax = fmaxf(fmaxf(z0, z1), z2), zmin = fminf(fminf(z0, z1), z2);
  const float bound = (m.flags & PRN_MESH_RELATIVE) ? __fmul_rn(m.gap, zmin) : m.gap;
  return __fsub_rn(zmax, zmin) <= bound;
}

// pixel p of one image (d, l: that image): its validity and, with TRI, whether the quad whose corner a it is emits t0 = (a, b, c), t1 = (c, b, d)
template <bool TRI>
__device__ __forceinline__ mesh_px mesh_pixel(const mesh_in& m, const float* __restrict__ d, const int* __restrict__ l, int p) {
  mesh_px r = {false, false, false, 0.f, 0};
  if (p >= m.HW) return r;
  r.z = d[p];
  r.lab = l ? l[p] : 0;
  r.valid = mesh_valid(m, r.z, r.lab);
  if (!TRI) return r;
  const int v = p / m.W, u = p - v * m.W;
  if (u >= m.W - 1 || v >= m.H - 1) return r;                       // (so p + W + 1 <= HW - 1)
  const float zb = d[p + m.W], zc = d[p + 1], zd = d[p + m.W + 1];
  const int lb = l ? l[p + m.W] : 0, lc = l ? l[p + 1] : 0, ld = l ? l[p + m.W + 1] : 0;
  if (!(mesh_valid(m, zb, lb) && mesh_valid(m, zc, lc))) return r;  // b and c are corners of both
  r.t0 = r.valid && mesh_tri(m, r.z, zb, zc, r.lab, lb, lc);
  r.t1 = mesh_valid(m, zd, ld) && mesh_tri(m, zc, zb, zd, lc, lb, ld);
  return r;
}

// set lanes of `b` below this lane
__device__ __forceinline__ unsigned below(u64 b) { return (unsigned)__popcll(b & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// n: this wave's total (the same in every lane) -> the totals of the waves before this one; total = of the workgroup.  sm: 4 words
__device__ __forceinline__ unsigned waves_before(unsigned n, unsigned* sm, unsigned& total) {
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = n;
  __syncthreads();
  unsigned base = 0u, tot = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned t = sm[i];
    if (i < w) base += t;
    tot += t;
  }
  total = tot;
  return base;
}

// launch 1: cells[image][workgroup] = (valid pixels, emitted triangles) of the workgroup's pixels
template <bool FACES>
__global__ __launch_bounds__(MESH_PX) void mesh_count_kernel(mesh_in m, int nblk, uint2* __restrict__ cells) {
  __shared__ unsigned s_v[4], s_t[4];
  const int img = blockIdx.y;
  const size_t at = (size_t)img * m.HW;
  const mesh_px px = mesh_pixel<FACES>(m, m.depth + at, m.labels ? m.labels + at : nullptr, (int)(blockIdx.x * MESH_PX + threadIdx.x));
  const unsigned nv = (unsigned)__popcll(__ballot(px.valid));
  const unsigned nt = FACES ? (unsigned)(__popcll(__ballot(px.t0)) + __popcll(__ballot(px.t1))) : 0u;
  unsigned tv, tt;
  waves_before(nv, s_v, tv);
  waves_before(nt, s_t, tt);
  if (threadIdx.x == 0) cells[(size_t)img * nblk + blockIdx.x] = make_uint2(tv, tt);
}

// inclusive scan of v over the lanes of a wave
__device__ __forceinline__ unsigned wave_scan_incl(unsigned v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// launch 2, one workgroup per image: cells[image][.] <- their exclusive scan, counts[image] = (vertices, triangles)
__global__ __launch_bounds__(MESH_CHUNK) void mesh_scan_kernel(uint2* __restrict__ cells, int nblk, int* __restrict__ counts) {
  __shared__ unsigned s_v[4], s_t[4];
  uint2* c = cells + (size_t)blockIdx.x * nblk;
  unsigned cv = 0u, ct = 0u;
  for (int i0 = 0; i0 < nblk; i0 += MESH_CHUNK) {                    // (nblk <= 2^16)
    const int i = i0 + threadIdx.x;
    const uint2 x = i < nblk ? c[i] : make_uint2(0u, 0u);
    const unsigned iv = wave_scan_incl(x.x), it = wave_scan_incl(x.y);
    __syncthreads();                                                // the previous chunk's wave totals are no longer read
    unsigned tv, tt;
    const unsigned bv = waves_before(__shfl(iv, 63, 64), s_v, tv), bt = waves_before(__shfl(it, 63, 64), s_t, tt);
    if (i < nblk) c[i] = make_uint2(cv + bv + iv - x.x, ct + bt + it - x.y);
    cv += tv;
    ct += tt;
  }
  if (threadIdx.x == 0) {
    counts[2 * blockIdx.x] = (int)cv;
    counts[2 * blockIdx.x + 1] = (int)ct;
  }
}

// n dwords of LDS to o, consecutive lanes on consecutive dwords
template <class T>
__device__ __forceinline__ void store_words(T* __restrict__ o, const T* s, unsigned n) {
  for (unsigned i = threadIdx.x; i < n; i += MESH_PX) o[i] = s[i];
}

// launch 3: the id map, and positions, labels and colours of the workgroup's vertices at (the workgroup's offset + rank)
__global__ __launch_bounds__(MESH_PX) void mesh_vertex_kernel(mesh_in m, const unsigned char* __restrict__ colors, const double* __restrict__ kmat, int nblk,
                                                              const uint2* __restrict__ cells, float* __restrict__ vertices, int* __restrict__ vlabels,
                                                              unsigned char* __restrict__ vcolors, int* __restrict__ vertex_id) {
  __shared__ unsigned s_w[4];
  __shared__ float s_pos[3 * MESH_PX];
  __shared__ unsigned char s_col[3 * MESH_PX];
  const int img = blockIdx.y;
  const size_t at = (size_t)img * m.HW;
  const int p = (int)(blockIdx.x * MESH_PX + threadIdx.x);
  const mesh_px px = mesh_pixel<false>(m, m.depth + at, m.labels ? m.labels + at : nullptr, p);
  const u64 bv = __ballot(px.valid);
  unsigned tot;
  const unsigned r = waves_before((unsigned)__popcll(bv), s_w, tot) + below(bv);
  const unsigned off = cells[(size_t)img * nblk + blockIdx.x].x;
  if (off + tot > (unsigned)m.HW) return;                           // (cannot happen while the inputs are what launch 1 counted: no store past a buffer)
  if (p < m.HW) vertex_id[at + p] = px.valid ? (int)(off + r) : -1;
  if (px.valid) {
    const double* k = kmat + 9 * img;
    const double fx = k[0], fy = k[4], cx = k[2], cy = k[5], z = (double)px.z;
    const int v = p / m.W, u = p - v * m.W;
    s_pos[3 * r] = (float)__ddiv_rn(__dmul_rn(__dsub_rn((double)u, cx), z), fx);
    s_pos[3 * r + 1] = (float)__ddiv_rn(__dmul_rn(__dsub_rn((double)v, cy), z), fy);
    s_pos[3 * r + 2] = px.z;
    vlabels[at + off + r] = px.lab;                                 // (a wave's valid lanes: consecutive words)
    if (colors) {
      const unsigned char* c = colors + (at + p) * 3;
      s_col[3 * r] = c[0];
      s_col[3 * r + 1] = c[1];
      s_col[3 * r + 2] = c[2];
    }
  }
  __syncthreads();
  store_words(vertices + (at + off) * 3, s_pos, 3u * tot);
  if (colors) {
    unsigned char* o = vcolors + (at + off) * 3;
    const unsigned n = 3u * tot;
    const unsigned head = min(n, (unsigned)((4u - (unsigned)(reinterpret_cast<uintptr_t>(o) & 3u)) & 3u));     // bytes before the first 4-byte boundary
    const unsigned words = (n - head) >> 2, tail = head + 4u * words;
    if (threadIdx.x < head) o[threadIdx.x] = s_col[threadIdx.x];
    unsigned* ow = reinterpret_cast<unsigned*>(o + head);
    for (unsigned i = threadIdx.x; i < words; i += MESH_PX) {
      const unsigned char* s = s_col + head + 4u * i;
      ow[i] = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    }
    if (threadIdx.x < n - tail) o[tail + threadIdx.x] = s_col[tail + threadIdx.x];
  }
}

// launch 4: the triangles of the workgroup's quads at (the workgroup's offset + rank), t0 before t1
__global__ __launch_bounds__(MESH_PX) void mesh_face_kernel(mesh_in m, const int* __restrict__ vertex_id, int nblk, const uint2* __restrict__ cells,
                                                            int64_t capf, int* __restrict__ faces) {
  __shared__ unsigned s_w[4];
  __shared__ int s_f[6 * MESH_PX];
  const int img = blockIdx.y;
  const size_t at = (size_t)img * m.HW;
  const int p = (int)(blockIdx.x * MESH_PX + threadIdx.x);
  const mesh_px px = mesh_pixel<true>(m, m.depth + at, m.labels ? m.labels + at : nullptr, p);
  const u64 b0 = __ballot(px.t0), b1 = __ballot(px.t1);
  unsigned tot;
  unsigned r = waves_before((unsigned)(__popcll(b0) + __popcll(b1)), s_w, tot) + below(b0) + below(b1);
  const unsigned off = cells[(size_t)img * nblk + blockIdx.x].y;
  if ((int64_t)off + tot > capf) return;                            // (as in launch 3)
  if (px.t0 || px.t1) {
    const int* id = vertex_id + at + p;
    const int b = id[m.W], c = id[1];
    if (px.t0) {
      s_f[3 * r] = id[0];
      s_f[3 * r + 1] = b;
      s_f[3 * r + 2] = c;
      ++r;
    }
    if (px.t1) {
      s_f[3 * r] = c;
      s_f[3 * r + 1] = b;
      s_f[3 * r + 2] = id[m.W + 1];
    }
  }
  __syncthreads();
  store_words(faces + ((int64_t)img * capf + off) * 3, s_f, 3u * tot);
}

}  // namespace

extern "C" {

int prn_mesh_block_pixels(void) { return MESH_PX; }
int prn_mesh_scan_chunk(void) { return MESH_CHUNK; }

int64_t prn_mesh_ws_bytes(int B, int H, int W) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (int64_t)H * W >= (1LL << 24)) return -1;
  return (int64_t)B * cdiv((int64_t)H * W, MESH_PX) * 8;
}

int prn_mesh(const float* depth, const int* labels, const unsigned char* colors, const double* k, int B, int H, int W, float lo, float hi, float max_gap,
             int flags, void* ws, float* vertices, int* vertex_labels, unsigned char* vertex_colors, int* vertex_id, int* faces, int* counts, void* stream) {
  PRN_REQUIRE(H > 0 && W > 0 && B > 0 && B <= 65535, "prn_mesh: sizes must be positive and B <= 65535 (B=%d H=%d W=%d)", B, H, W);
  PRN_REQUIRE((int64_t)H * W < (1LL << 24), "prn_mesh: H * W = %lld must be below 2^24", (long long)((int64_t)H * W));
  PRN_REQUIRE(max_gap >= 0.f && max_gap <= 3.402823466e38f, "prn_mesh: max_gap must be finite and >= 0, got %g", (double)max_gap);
  PRN_REQUIRE((flags & ~(PRN_MESH_RELATIVE | PRN_MESH_SAME_LABEL | PRN_MESH_PLANAR_ONLY | PRN_MESH_FACES)) == 0, "prn_mesh: unknown flags 0x%x", flags);
  PRN_REQUIRE(depth && k && ws && vertices && vertex_labels && vertex_id && counts, "prn_mesh: null argument");
  PRN_REQUIRE((colors == nullptr) == (vertex_colors == nullptr), "prn_mesh: colors and vertex_colors go together");
  PRN_REQUIRE(!(flags & PRN_MESH_FACES) || faces || H < 2 || W < 2, "prn_mesh: PRN_MESH_FACES without a face buffer");
  PRN_REQUIRE(((uintptr_t)ws & 7u) == 0, "prn_mesh: the workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const mesh_in m = {depth, labels, H, W, H * W, lo, hi, max_gap, flags};
  const int nblk = cdiv((int64_t)H * W, MESH_PX);
  const bool with_faces = (flags & PRN_MESH_FACES) && H > 1 && W > 1;
  const dim3 grid(nblk, B);
  uint2* cells = (uint2*)ws;
  if (with_faces) mesh_count_kernel<true><<<grid, MESH_PX, 0, st>>>(m, nblk, cells);
  else mesh_count_kernel<false><<<grid, MESH_PX, 0, st>>>(m, nblk, cells);
  PRN_CHECK_LAUNCH("prn_mesh (count)");
  mesh_scan_kernel<<<B, MESH_CHUNK, 0, st>>>(cells, nblk, counts);
  PRN_CHECK_LAUNCH("prn_mesh (scan)");
  mesh_vertex_kernel<<<grid, MESH_PX, 0, st>>>(m, colors, k, nblk, cells, vertices, vertex_labels, vertex_colors, vertex_id);
  PRN_CHECK_LAUNCH("prn_mesh (vertices)");
  if (with_faces) {
    mesh_face_kernel<<<grid, MESH_PX, 0, st>>>(m, vertex_id, nblk, cells, 2LL * (H - 1) * (W - 1), faces);
    PRN_CHECK_LAUNCH("prn_mesh (faces)");
  }
  return 0;
}

}  // extern "C"
