// Label maps of instance masks and the overlap tables of two label maps (include/prn.h: prn_label_map, prn_label_overlap; DESIGN.md
// section 21).  Every plane-level evaluation figure -- Rand index, variation of information, segmentation covering, plane and pixel recall
// over depth-error thresholds -- is a function of one small table per frame:
//   T[g][p]  pixels that carry label g in map a (ground truth) and label p in map b (prediction)
//   S[g][p]  the sum over the same pixels of the depth error, as a fixed-point integer (below)
// so the device side is a paint pass and a 2-D histogram, all integers, and the floating-point scoring is fp64 on the host.
//
//   paint    one launch.  A thread owns 16 consecutive pixels of one image and walks that image's masks in priority order until every one of its
//            pixels has a label (label 0 = no mask, i + 1 = instance i).  A mask's 16 bytes are one 16-byte load where base + i * H * W + pixel
//            is 16-byte aligned, four 4-byte loads where it is 4-byte aligned, single bytes otherwise (prn_masks.h: an odd H * W puts most masks
//            on an odd address); a byte at or past the mask's end is never read.  Where every mask is aligned the loads of LM_AHEAD masks are
//            issued before the first is tested.  One image given as a flat [N][H][W] block needs no pointer table (prn_label_map_flat).
//   tables   one launch.  A thread owns OV_RUN consecutive pixels and adds a bin's RUN (count, error sum) once when the bin changes: neighbouring
//            pixels mostly hit the same bin, so a thread issues a few atomics, not one per pixel.  While (A + 1) * (B + 1) <= OV_LDS_BINS the
//            workgroup adds into its own tables in LDS (uint32 counts: a workgroup sees 4096 pixels; uint64 sums) and flushes its non-zero bins
//            with 64-bit global atomics at the end; above that every run goes to the global tables directly.
// Fixed point: e = |depth_b - depth_a| in fp32, 0 where depth_a < 1e-4 (no ground truth), q = rint(min(e, 1024) * 2^20) with NaN -> 1024: the
// product by a power of two is exact and rint is ties-to-even, so numpy restates q bit for bit; 2^30 * 2^24 pixels fit 64 bits.
// No workgroup waits for another, every loop is bounded by the sizes, the only atomics are integer adds: results are identical run to run and
// between a batched call and per-image calls.
#include "prn_masks.h"

namespace {

typedef unsigned long long u64;

constexpr int LM_PX = 16, LM_THREADS = 64;       // pixels per thread, threads per workgroup of the paint
constexpr int LM_AHEAD = 4;                     // masks whose bytes a thread of the paint loads before it tests the first of them
constexpr int OV_RUN = 16, OV_THREADS = 256;     // pixels per thread, threads per workgroup of the tables
constexpr int OV_LDS_BINS = PRN_LABEL_OVERLAP_LDS_BINS;
static_assert(OV_LDS_BINS * 12 <= 48 * 1024, "uint32 counts + uint64 sums of a workgroup stay within 48 KB of LDS");
static_assert(OV_RUN * OV_THREADS <= (1 << 16), "a workgroup's count of one bin fits its uint32 by a wide margin");

// ---- paint ----
// bit k = (p[k] != 0) for k < min(avail, 16): the widest loads the address admits, each under the rule of prn_masks.h
__device__ __forceinline__ unsigned lm_bits16(const unsigned char* __restrict__ p, int64_t avail) {
  if (__builtin_expect(avail >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0, 1)) return prn_mask_bits16(p, avail);
  unsigned bits = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) bits |= prn_mask_bits4(p + 4 * g, avail - 4 * g) << (4 * g);      // (avail <= 0 reads nothing)
  return bits;
}

// src: one pointer-table entry per image, or (flat != NULL) ONE image of n_flat masks back to back
__global__ __launch_bounds__(LM_THREADS) void label_map_kernel(prn_mask_src src, int n_flat, int64_t HW, int last_wins, int* __restrict__ labels) {
  const int b = blockIdx.y;
  const int64_t i0 = ((int64_t)blockIdx.x * LM_THREADS + threadIdx.x) * LM_PX;
  if (i0 >= HW) return;
  const int64_t avail = HW - i0;
  const unsigned want = avail >= LM_PX ? 0xffffu : ((1u << (int)avail) - 1u);
  const int n = src.flat ? n_flat : src.first[b + 1] - src.first[b];
  const unsigned char* base = (src.flat ? src.flat : src.masks[b]) + i0;      // (n == 0: never dereferenced)
  int lab[LM_PX];
#pragma unroll
  for (int k = 0; k < LM_PX; ++k) lab[k] = 0;
  unsigned done = 0;                                                // pixels that have their label
  // H * W a multiple of 16 on an aligned tensor -- the usual case -- puts this thread's bytes of EVERY mask on a 16-byte boundary: the loads of
  // LM_AHEAD masks are then issued together (prn_masks.h: prn_mask_bits16_each).
  const bool together = avail >= LM_PX && ((((uintptr_t)HW) | reinterpret_cast<uintptr_t>(base)) & 15) == 0;
  const int64_t step = last_wins ? -HW : HW;
  for (int j0 = 0; j0 < n && done != want; j0 += LM_AHEAD) {        // in priority order: the first mask that sets a pixel keeps it
    unsigned bits[LM_AHEAD];
    if (together && j0 + LM_AHEAD <= n) {
      prn_mask_bits16_each<LM_AHEAD>(base + (size_t)(last_wins ? n - 1 - j0 : j0) * (size_t)HW, step, avail, bits);
    } else {
#pragma unroll
      for (int u = 0; u < LM_AHEAD; ++u) {
        const int i = last_wins ? n - 1 - (j0 + u) : j0 + u;
        bits[u] = j0 + u < n ? lm_bits16(base + (size_t)i * (size_t)HW, avail) : 0u;
      }
    }
#pragma unroll
    for (int u = 0; u < LM_AHEAD; ++u) {
      const int i = last_wins ? n - 1 - (j0 + u) : j0 + u;
      const unsigned fresh = bits[u] & ~done;
      if (fresh) {
#pragma unroll
        for (int k = 0; k < LM_PX; ++k)
          if ((fresh >> k) & 1u) lab[k] = i + 1;
        done |= fresh;
      }
    }
  }
  int* o = labels + (size_t)b * (size_t)HW + i0;
#pragma unroll
  for (int k = 0; k < LM_PX; ++k)
    if (k < avail) o[k] = lab[k];
}

// ---- tables ----
struct __attribute__((packed, aligned(4))) ov_i4u { int v[4]; };    // four ints at a 4-byte aligned address: one load (as prn_f4u)

__device__ __forceinline__ unsigned ov_quantise(float da, float db) {
  float e = fabsf(db - da);
  if (da < 1e-4f) e = 0.f;                                          // no ground truth here
  e = (e < 1024.f) ? e : 1024.f;                                    // = fminf(e, 1024): NaN and everything above 1024 m become 1024 m
  return (unsigned)rintf(e * 1048576.f);                            // exact product, ties to even; at most 2^30
}

template <bool LDS>
__global__ __launch_bounds__(OV_THREADS) void label_overlap_kernel(const int* __restrict__ labels_a, const int* __restrict__ labels_b,
                                                                   const float* __restrict__ depth_a, const float* __restrict__ depth_b, int64_t HW, int A,
                                                                   int B, u64* __restrict__ count, u64* __restrict__ wsum) {
  __shared__ unsigned s_cnt[LDS ? OV_LDS_BINS : 1];
  __shared__ u64 s_sum[LDS ? OV_LDS_BINS : 1];
  const int img = blockIdx.y;
  const int bins = (A + 1) * (B + 1);
  const size_t tbase = (size_t)img * (size_t)bins;
  if (LDS) {
    for (int k = threadIdx.x; k < bins; k += OV_THREADS) { s_cnt[k] = 0u; s_sum[k] = 0ull; }
    __syncthreads();
  }
  const int64_t i0 = ((int64_t)blockIdx.x * OV_THREADS + threadIdx.x) * OV_RUN;
  if (i0 < HW) {
    const size_t off = (size_t)img * (size_t)HW + (size_t)i0;
    const int* la = labels_a + off;
    const int* lb = labels_b + off;
    const float* da = depth_a ? depth_a + off : nullptr;
    const float* db = depth_b ? depth_b + off : nullptr;
    const int64_t avail = HW - i0;
    int cur = -1;                                                   // the bin of the run in hand (-1: none)
    unsigned run_cnt = 0;
    u64 run_sum = 0;
#pragma unroll
    for (int g = 0; g < OV_RUN; g += 4) {
      int a4[4], b4[4];
      float x4[4], y4[4];
      if (g + 4 <= avail) {
        const ov_i4u va = *reinterpret_cast<const ov_i4u*>(la + g), vb = *reinterpret_cast<const ov_i4u*>(lb + g);
#pragma unroll
        for (int k = 0; k < 4; ++k) { a4[k] = va.v[k]; b4[k] = vb.v[k]; x4[k] = 0.f; y4[k] = 0.f; }
        if (da) {
          const prn_f4u vx = *reinterpret_cast<const prn_f4u*>(da + g), vy = *reinterpret_cast<const prn_f4u*>(db + g);
#pragma unroll
          for (int k = 0; k < 4; ++k) { x4[k] = vx.v[k]; y4[k] = vy.v[k]; }
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = g + k < avail;
          a4[k] = in ? la[g + k] : -1;                              // past the end: dropped like any label out of range
          b4[k] = in ? lb[g + k] : -1;
          x4[k] = (in && da) ? da[g + k] : 0.f;
          y4[k] = (in && da) ? db[g + k] : 0.f;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = (unsigned)a4[k] <= (unsigned)A && (unsigned)b4[k] <= (unsigned)B;
        const int bin = ok ? a4[k] * (B + 1) + b4[k] : -1;
        if (bin != cur) {
          if (cur >= 0) {
            if (LDS) {
              atomicAdd(&s_cnt[cur], run_cnt);
              if (run_sum) atomicAdd(&s_sum[cur], run_sum);
            } else {
              atomicAdd(count + tbase + cur, (u64)run_cnt);
              if (run_sum) atomicAdd(wsum + tbase + cur, run_sum);
            }
          }
          cur = bin; run_cnt = 0; run_sum = 0;
        }
        if (ok) {
          ++run_cnt;
          if (da) run_sum += ov_quantise(x4[k], y4[k]);
        }
      }
    }
    if (cur >= 0) {
      if (LDS) {
        atomicAdd(&s_cnt[cur], run_cnt);
        if (run_sum) atomicAdd(&s_sum[cur], run_sum);
      } else {
        atomicAdd(count + tbase + cur, (u64)run_cnt);
        if (run_sum) atomicAdd(wsum + tbase + cur, run_sum);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int k = threadIdx.x; k < bins; k += OV_THREADS) {          // only what this workgroup touched
      const unsigned c = s_cnt[k];
      if (c) {
        atomicAdd(count + tbase + k, (u64)c);
        const u64 s = s_sum[k];
        if (s) atomicAdd(wsum + tbase + k, s);
      }
    }
  }
}

}  // namespace

extern "C" int prn_label_overlap_lds_bins(void) { return OV_LDS_BINS; }

extern "C" int prn_label_map(const unsigned char* const* masks_dev, const int* first_dev, int B, int H, int W, int priority, int* labels, void* stream) {
  PRN_REQUIRE(masks_dev && first_dev && labels, "prn_label_map: null pointer argument");
  PRN_REQUIRE(B >= 1 && B <= 65535 && H > 0 && W > 0, "prn_label_map: needs 1 <= B <= 65535, H > 0, W > 0 (got B=%d H=%d W=%d)", B, H, W);
  PRN_REQUIRE((int64_t)H * W < (1LL << 31), "prn_label_map: needs H * W < 2^31 (got %d x %d)", H, W);
  PRN_REQUIRE(priority == PRN_LABEL_FIRST_WINS || priority == PRN_LABEL_LAST_WINS, "prn_label_map: priority must be 0 (lowest index wins) or 1 (highest) (got %d)",
              priority);
  const int64_t HW = (int64_t)H * W;
  const prn_mask_src src = {masks_dev, first_dev, B, nullptr};
  hipLaunchKernelGGL(label_map_kernel, dim3(cdiv(HW, (int64_t)LM_PX * LM_THREADS), B), dim3(LM_THREADS), 0, (hipStream_t)stream, src, 0, HW, priority, labels);
  PRN_CHECK_LAUNCH("prn_label_map");
  return 0;
}

extern "C" int prn_label_map_flat(const unsigned char* masks, int N, int H, int W, int priority, int* labels, void* stream) {
  PRN_REQUIRE(masks && labels, "prn_label_map_flat: null pointer argument");
  PRN_REQUIRE(N >= 1 && H > 0 && W > 0, "prn_label_map_flat: needs N >= 1, H > 0, W > 0 (got N=%d H=%d W=%d)", N, H, W);
  PRN_REQUIRE((int64_t)H * W < (1LL << 31), "prn_label_map_flat: needs H * W < 2^31 (got %d x %d)", H, W);
  PRN_REQUIRE(priority == PRN_LABEL_FIRST_WINS || priority == PRN_LABEL_LAST_WINS, "prn_label_map_flat: priority must be 0 (lowest index wins) or 1 (highest) (got %d)",
              priority);
  const int64_t HW = (int64_t)H * W;
  const prn_mask_src src = {nullptr, nullptr, 1, masks};
  hipLaunchKernelGGL(label_map_kernel, dim3(cdiv(HW, (int64_t)LM_PX * LM_THREADS), 1), dim3(LM_THREADS), 0, (hipStream_t)stream, src, N, HW, priority, labels);
  PRN_CHECK_LAUNCH("prn_label_map_flat");
  return 0;
}

extern "C" int prn_label_overlap(const int* labels_a, const int* labels_b, const float* depth_a, const float* depth_b, int nimg, int H, int W, int A, int B,
                                 uint64_t* count, uint64_t* wsum, void* stream) {
  PRN_REQUIRE(labels_a && labels_b, "prn_label_overlap: null label pointer");
  PRN_REQUIRE(count && wsum, "prn_label_overlap: null output pointer");
  PRN_REQUIRE((depth_a == nullptr) == (depth_b == nullptr), "prn_label_overlap: depth_a and depth_b go together (one of them is null)");
  PRN_REQUIRE(A >= 0 && B >= 0 && A <= 1023 && B <= 1023, "prn_label_overlap: needs 0 <= A, B <= 1023 labels (got A=%d B=%d)", A, B);
  PRN_REQUIRE(nimg >= 1 && nimg <= 65535 && H > 0 && W > 0, "prn_label_overlap: needs 1 <= images <= 65535, H > 0, W > 0 (got %d images, %d x %d)", nimg, H, W);
  PRN_REQUIRE((int64_t)H * W < (1LL << 24), "prn_label_overlap: needs H * W < 2^24 (2^30 per pixel must fit 64 bits; got %d x %d)", H, W);
  const int64_t HW = (int64_t)H * W;
  const dim3 grid(cdiv(HW, (int64_t)OV_RUN * OV_THREADS), nimg);
  if ((A + 1) * (B + 1) <= OV_LDS_BINS)
    hipLaunchKernelGGL(label_overlap_kernel<true>, grid, dim3(OV_THREADS), 0, (hipStream_t)stream, labels_a, labels_b, depth_a, depth_b, HW, A, B, (u64*)count,
                       (u64*)wsum);
  else
    hipLaunchKernelGGL(label_overlap_kernel<false>, grid, dim3(OV_THREADS), 0, (hipStream_t)stream, labels_a, labels_b, depth_a, depth_b, HW, A, B, (u64*)count,
                       (u64*)wsum);
  PRN_CHECK_LAUNCH("prn_label_overlap");
  return 0;
}
