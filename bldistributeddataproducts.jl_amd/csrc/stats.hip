// stats.hip — fqavfunc median, var and std of Float32 windows (gfx950).
//
// Julia's Statistics applied as f(reshape(A, (F, :, ...)); dims=1): one result
// per block of F channels (c' F .. c' F + F - 1) of every (IF, spectrum) row.
// No time integration (T = 1).  The window geometry is the reduce's
// (RedArgs: any channel offset, step and direction, IF and time steps);
// unit-step windows whose F is a multiple of 4 load float4 (16 bytes per
// lane, at any dword alignment: f4u), the others one dword per element.
//
//   var / std  k_mom_lanes (F <= 1024): the 1 .. 64 lanes of a wave that share
//              a block hold it in registers (<= 16 values per lane), the
//              partial sums meet by xor-shuffles, then the squared deviations
//              about the mean.  k_mom_block (F > 1024): one workgroup per
//              block, in registers up to 4096 values, else read twice (the
//              second read hits L2: a block is <= 256 KiB at the 0002
//              products' F = 65536); waves meet through LDS.
//              The mean is taken as K + sum(x - K) / F with K the block's
//              first element: a constant block then has mean == its value and
//              the result is exactly 0.0 whatever F does to a rounded sum, and
//              the sum of the differences keeps more bits than the sum.
//   median     keys are the order-preserving uint32 image of the float
//              (isless order: -0.0 < 0.0, -Inf lowest, +Inf highest), NaN is
//              found apart and wins.
//              k_median_sort (F <= 64): next_pow2(F) / 4 lanes hold 4 keys
//              each and run a bitonic network, the exchanges at distance < 4
//              in registers and the others by xor-shuffles; missing elements
//              are the maximal key.
//              k_median_select (F > 64): one workgroup per block, an MSB-first
//              radix select, 8 bits a pass, of rank (F-1)/2 and rank F/2 in
//              the same four passes: the two ranks share a 256-bin LDS
//              histogram while their prefixes agree and take one each after.
//              Four passes fix all 32 bits, so ties need nothing special.
//              Keys stay in registers up to 4096 (PATH_MEDIAN_SELECT), else
//              every pass reads the block again (PATH_MEDIAN_STREAM).
//   mad        StatsBase's mad(x; normalize=true): c = median(x), m = the median
//              (same rule, NaN wins) of |x - c| with the difference rounded
//              once, result = Float32(Float64(m) * 1.4826022185056018).  The
//              median's kernels with MAD set run their selection twice: the
//              keys in registers become those of |x - c| in place (one read
//              of the block), the stream form reads the block again and forms
//              the deviations on the way.  Plans and paths are the median's.
//   quantile   Statistics.quantile(x, p) (type 7): the host turns (F, p) into
//              the lower rank q = j - 1 and the weight g (RedArgs qrank, qg);
//              the median's kernels with SEL_QUANTILE select ranks q and q + 1
//              where the median's take (F-1)/2 and F/2, and quantile_of joins
//              them: a + g (b - a), the difference rounded once to Float32, the
//              rest once each in Float64; NaN wins.  Plans and paths are the
//              median's.
//   quantiles  quantiles(ps): K <= 8 quantiles of every block from ONE selection.
//              The host turns (F, ps) into a QSet (bldp_impl.h): the sorted
//              distinct ranks {j_k - 1, j_k} (<= 16) and, per plane, which two
//              of them it joins and with what weight; it is a kernel argument
//              of these instantiations alone.  Plane k is written k *
//              out_ld_q elements after plane 0 and is, bit for bit, the
//              quantile instantiation's result for ps[k].
//              k_median_sort with SEL_QUANTILES sorts once and then picks and
//              stores plane by plane.  k_quantiles_select is k_median_select's
//              radix select for R ranks: still four passes over keys loaded
//              once (registers) or four reads of the block (stream), whatever
//              K is.  Per rank the prefix fixed so far and the rank among that
//              prefix's keys live in LDS.  The ranks are sorted, so their
//              prefixes are too: equal prefixes are adjacent, each distinct
//              one gets a slot of 256 counters (<= 16 slots, 16 KiB), a key
//              matches at most one slot and is counted at slot * 256 + digit
//              with hist_add's leader trick.  The waves then scan one slot
//              each and settle every rank of that slot.  Plans and paths are
//              the median's; reads of the block: 1, 1 and 4.
//   outliers   (the bldp_outliers_* entry points) c = median(x), s = mad(x) as
//              above, thr = Float32(nsigma * Float64(s)); sample i is flagged
//              when |x_i - c| > thr, strictly, and never when c or s is NaN.
//              The median's kernels with SEL_OUTLIERS run mad's two selections
//              and then write what the trailing OutlArgs (bldp_impl.h) asks for:
//              the median, the scaled mad, the count of flagged samples and the
//              flags.  Sort and register-select forms: the keys held are those
//              of |x - c|, compared against the threshold's key and counted over
//              the lane group (xor-shuffles) or the workgroup (LDS); the mask
//              reloads the block for the positions (1 read, 2 with a mask).
//              Stream form: one more pass over the block (9 reads).  Plans and
//              paths are mad's.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "bldp_impl.h"

namespace bldp {
namespace {

constexpr int kBlock = 256;  // 4 waves of 64
// a float4 on any dword boundary (kernels.hip f4u)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int64_t kLaneMaxF = 1024;  // k_mom_lanes: 64 lanes x 16 values
constexpr int64_t kRegMaxF = 4096;   // a workgroup's registers: 256 lanes x 16 values
constexpr int64_t kSortMaxF = 64;    // k_median_sort

__device__ __forceinline__ float4 ld4(const float *p) {
  const f4u v = *reinterpret_cast<const f4u *>(p);
  return make_float4(v.x, v.y, v.z, v.w);
}

// q = x / d, r = x % d for x >= 0 and a wave-uniform d > 0: a shift for a power
// of two (the products' channel counts and fqavby, nif = 1), else 32-bit
// division where both fit (a 64-bit one is ~100 instructions a lane).
__device__ __forceinline__ void divmod(int64_t x, int64_t d, int64_t &q, int64_t &r) {
  if ((d & (d - 1)) == 0) {
    q = x >> __builtin_ctzll((unsigned long long)d);
    r = x & (d - 1);
  } else if ((((uint64_t)x | (uint64_t)d) >> 32) == 0) {
    const uint32_t q32 = (uint32_t)x / (uint32_t)d;
    q = q32;
    r = (uint32_t)x - q32 * (uint32_t)d;
  } else {
    q = x / d;
    r = x - q * d;
  }
}

// Block g of bank blockIdx.y: its first element and its output; false past the end.
__device__ __forceinline__ bool stat_group(const RedArgs &a, int64_t g, const float *&p,
                                           float *&o) {
  if (g >= a.nco * a.ni * a.nto) return false;
  int64_t co, r, i, t;
  divmod(g, a.nco, r, co);
  divmod(r, a.ni, t, i);
  const int64_t b = blockIdx.y;
  p = a.in[b] + a.in_off + co * a.F * a.in_cs + i * a.in_ld_i + t * a.in_ld_t;
  o = a.out + b * a.out_bank + co + i * a.out_ld_i + t * a.out_ld_t;
  return true;
}

// outliers: where the mask holds the first element of block g of bank blockIdx.y
__device__ __forceinline__ uint8_t *outl_mask(const RedArgs &a, const OutlArgs &oa, int64_t g) {
  int64_t co, r, i, t;
  divmod(g, a.nco, r, co);
  divmod(r, a.ni, t, i);
  return oa.mask + blockIdx.y * oa.mask_bank + co * a.F + i * oa.mask_ld_i + t * oa.mask_ld_t;
}

// ---------------------------------------------------------------------------
// var / std

// corrected variance (F = 1: 0/0 = NaN, as Julia), or its root
__device__ __forceinline__ float mom_finish(float ssq, float n, int op) {
  const float var = ssq / (n - 1.0f);
  return op == BLDP_OP_STD ? sqrtf(var) : var;
}

template <int LPG, bool VEC>
__global__ __launch_bounds__(kBlock) void k_mom_lanes(const RedArgs a, const int op) {
  const int lg = threadIdx.x % LPG;
  const int64_t tile = xcd_order(blockIdx.x, gridDim.x, a.xcd_lg);
  const float *p = nullptr;
  float *o = nullptr;
  const bool ok = stat_group(a, tile * (kBlock / LPG) + threadIdx.x / LPG, p, o);
  const int F = (int)a.F;
  float v[16];
  // element slot u of this lane is valid when has(u)
  auto has = [&](int u) {
    return ok && (VEC ? 4 * (lg + (u / 4) * LPG) < F : lg + u * LPG < F);
  };
  const float K = ok ? p[0] : 0.0f;  // the block's first element (the lanes' own cache line)
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (has(4 * j)) {
        const float4 x = ld4(p + 4 * (lg + j * LPG));
        v[4 * j] = x.x, v[4 * j + 1] = x.y, v[4 * j + 2] = x.z, v[4 * j + 3] = x.w;
      }
  } else {
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (has(u)) v[u] = p[(int64_t)(lg + u * LPG) * a.in_cs];
  }
  float s = 0.0f;  // of x - K
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if (has(u)) s += v[u] - K;
#pragma unroll
  for (int w = LPG / 2; w >= 1; w /= 2) s += __shfl_xor(s, w, 64);
  const float mean = K + s / (float)F;
  float q = 0.0f;
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if (has(u)) {
      const float d = v[u] - mean;
      q += d * d;
    }
#pragma unroll
  for (int w = LPG / 2; w >= 1; w /= 2) q += __shfl_xor(q, w, 64);
  if (ok && lg == 0) *o = mom_finish(q, (float)F, op);
}

// sum over the workgroup, the same value in every thread (sh: 4 floats, one use)
__device__ __forceinline__ float block_sum(float x, float *sh) {
#pragma unroll
  for (int w = 32; w >= 1; w /= 2) x += __shfl_xor(x, w, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_mom_block(const RedArgs a, const int op) {
  __shared__ float sh[2][4];
  const int tid = threadIdx.x;
  const float *p = nullptr;
  float *o = nullptr;
  if (!stat_group(a, blockIdx.x, p, o)) return;  // (uniform)
  const int64_t F = a.F, n = VEC ? F / 4 : F;    // items: float4s or values
  const bool regs = F <= kRegMaxF;
  float v[16];
  auto has = [&](int u) { return (VEC ? tid + (u / 4) * kBlock : tid + u * kBlock) < n; };
  const float K = p[0];  // the block's first element
  float s = 0.0f;        // of x - K
  if (regs) {
    if (VEC) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (has(4 * j)) {
          const float4 x = ld4(p + 4 * (tid + j * kBlock));
          v[4 * j] = x.x, v[4 * j + 1] = x.y, v[4 * j + 2] = x.z, v[4 * j + 3] = x.w;
        }
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (has(u)) v[u] = p[(int64_t)(tid + u * kBlock) * a.in_cs];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (has(u)) s += v[u] - K;
  } else {
#pragma unroll 4
    for (int64_t k = tid; k < n; k += kBlock) {
      if (VEC) {
        const float4 x = ld4(p + 4 * k);
        s += ((x.x - K) + (x.y - K)) + ((x.z - K) + (x.w - K));
      } else {
        s += p[k * a.in_cs] - K;
      }
    }
  }
  const float mean = K + block_sum(s, sh[0]) / (float)F;
  float q = 0.0f;
  if (regs) {
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (has(u)) {
        const float d = v[u] - mean;
        q += d * d;
      }
  } else {
#pragma unroll 4
    for (int64_t k = tid; k < n; k += kBlock) {
      if (VEC) {
        const float4 x = ld4(p + 4 * k);
        const float d0 = x.x - mean, d1 = x.y - mean, d2 = x.z - mean, d3 = x.w - mean;
        q += d0 * d0, q += d1 * d1, q += d2 * d2, q += d3 * d3;
      } else {
        const float d = p[k * a.in_cs] - mean;
        q += d * d;
      }
    }
  }
  q = block_sum(q, sh[1]);
  if (tid == 0) *o = mom_finish(q, (float)F, op);
}

// ---------------------------------------------------------------------------
// median

// isless order of Float32 as unsigned order (NaN aside)
__device__ __forceinline__ uint32_t f2key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// Statistics.middle(a, b) = a/2 + b/2 (no overflow next to floatmax), each half
// rounded before the sum.  The products must not be contracted into a fused
// multiply-add (tstats.hip middle): half a subnormal, or a normal below 2^-125,
// with an odd significand is inexact, and fma(a, 0.5, b/2) keeps the exact
// half.  hipcc contracts by default, __fmul_rn or not: the sort and select
// kernels here held v_fmac_f32 v, 0.5, v before the pragma.
__device__ __forceinline__ float middle(float x, float y) {
#pragma clang fp contract(off)
  const float hx = x * 0.5f, hy = y * 0.5f;
  return hx + hy;
}
// Ranks (F-1)/2 and F/2 of a block of F: the element itself for odd F, else
// middle() even of two equal values (a/2 + a/2 is not a for a subnormal with
// an odd significand).
__device__ __forceinline__ float median_of(uint32_t k0, uint32_t k1, bool odd, bool nan) {
  if (nan) return __uint_as_float(0x7fc00000u);
  return odd ? key2f(k0) : middle(key2f(k0), key2f(k1));
}

// Ranks q and q + 1 of a block joined with weight g (bldp_impl.h quantile_mix)
__device__ __forceinline__ float quantile_of(uint32_t k0, uint32_t k1, double g, bool nan) {
  if (nan) return __uint_as_float(0x7fc00000u);
  return quantile_mix(key2f(k0), key2f(k1), g);
}

constexpr uint32_t kPadKey = 0xffffffffu;  // above every non-NaN key

// The bitonic network over the L keys of a group of L / 4 lanes (key e = 4 *
// lane + r): runs of kk keys, ascending where (e & kk) == 0.
template <int L>
__device__ __forceinline__ void bitonic_sort4(uint32_t (&k)[4], const int lg) {
#pragma unroll
  for (int kk = 2; kk <= L; kk *= 2) {
#pragma unroll
    for (int j = kk / 2; j >= 1; j /= 2) {
      if (j >= 4) {  // partner key e ^ j sits in lane ^ (j / 4), same r
        const bool up = kk == L || ((4 * lg) & kk) == 0;
        const bool low = (lg & (j / 4)) == 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t other = __shfl_xor(k[r], j / 4, 64);
          k[r] = (low == up) ? min(k[r], other) : max(k[r], other);
        }
      } else {  // both keys in this lane
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if ((r & j) == 0) {
            const bool up = kk == L || ((4 * lg + r) & kk) == 0;
            const uint32_t lo = min(k[r], k[r | j]), hi = max(k[r], k[r | j]);
            k[r] = up ? lo : hi;
            k[r | j] = up ? hi : lo;
          }
      }
    }
  }
}

// L = next_pow2(F) >= 4 keys over L / 4 lanes, key e = 4 * lane + r.  MAD: the
// sorted keys become those of |x - median| in place (the padding, which sorts
// to e >= F, stays) and the network runs again.  SEL_QUANTILE: the ranks are
// a.qrank and the next.  SEL_QUANTILES: one more argument, the QSet (QS is empty
// for every other selector: their signature is (RedArgs)); the planes' ranks
// are picked and stored one plane after the other.  SEL_OUTLIERS: mad's two
// sorts, then the trailing OutlArgs' outputs: the sorted keys of |x - median|
// above the threshold's are counted over the group, and the mask reloads the
// lane's elements for their positions.
template <typename T>
__device__ __forceinline__ const T &first_arg(const T &x) {
  return x;
}
template <int L, bool VEC, Sel SEL, typename... QS>
__global__ __launch_bounds__(kBlock) void k_median_sort(const RedArgs a, const QS... qs) {
  constexpr bool MAD = SEL == SEL_MAD || SEL == SEL_OUTLIERS;
  constexpr int LG = L / 4;
  const int lg = threadIdx.x % LG;
  const int64_t tile = xcd_order(blockIdx.x, gridDim.x, a.xcd_lg);
  const float *p = nullptr;
  float *o = nullptr;
  const bool ok = stat_group(a, tile * (kBlock / LG) + threadIdx.x / LG, p, o);
  const int F = (int)a.F;
  uint32_t k[4] = {kPadKey, kPadKey, kPadKey, kPadKey};
  bool nan = false;
  if (VEC) {
    if (ok && 4 * lg < F) {
      const float4 x = ld4(p + 4 * lg);
      nan = x.x != x.x || x.y != x.y || x.z != x.z || x.w != x.w;
      k[0] = f2key(x.x), k[1] = f2key(x.y), k[2] = f2key(x.z), k[3] = f2key(x.w);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ok && 4 * lg + r < F) {
        const float x = p[(int64_t)(4 * lg + r) * a.in_cs];
        nan = nan || x != x;
        k[r] = f2key(x);
      }
  }
  bitonic_sort4<L>(k, lg);
  // ranks (F-1)/2 and F/2 (the same for odd F); the padding sorts above them
  const int q0 = SEL == SEL_QUANTILE ? a.qrank : (F - 1) / 2;
  const int q1 = SEL == SEL_QUANTILE ? a.qrank + 1 : F / 2;
  auto pick = [&](int q) {
    const int r = q & 3;
    uint32_t x;
    if constexpr (SEL == SEL_OUTLIERS) {
      // (copies: choosing among the addresses of k, which is written again
      // below, kept k in scratch at L = 4)
      const uint32_t k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3];
      x = r == 0 ? k0 : r == 1 ? k1 : r == 2 ? k2 : k3;
    } else {
      x = r == 0 ? k[0] : r == 1 ? k[1] : r == 2 ? k[2] : k[3];
    }
    if (LG > 1) x = __shfl(x, (int)(threadIdx.x & 63) - lg + q / 4, 64);
    return x;
  };
  uint32_t k0 = pick(q0), k1 = pick(q1);
  const unsigned long long gmask = LG == 64 ? ~0ull : ((1ull << LG) - 1ull);
  float c = 0.0f;     // MAD: the block's median
  bool nan0 = false;  // SEL_OUTLIERS: the block holds a NaN
  if (MAD) {
    c = median_of(k0, k1, F & 1, false);  // (a NaN block: NaN below, whatever c is)
    if constexpr (SEL == SEL_OUTLIERS)
      nan0 = ((__ballot(nan) >> ((threadIdx.x & 63) - lg)) & gmask) != 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * lg + r < F) {
        const float d = abs_dev(key2f(k[r]), c);
        nan = nan || d != d;
        k[r] = f2key(d);
      }
    bitonic_sort4<L>(k, lg);
    k0 = pick(q0), k1 = pick(q1);
  }
  const unsigned long long bal = __ballot(nan);
  const bool gnan = ((bal >> ((threadIdx.x & 63) - lg)) & gmask) != 0;
  if constexpr (SEL == SEL_OUTLIERS) {
    const OutlArgs &oa = first_arg(qs...);
    const float sc = mad_scale(median_of(k0, k1, F & 1, gnan));
    const float thr = outl_thr(oa.nsigma, sc);
    const bool live = !gnan && thr == thr;  // (a NaN median or scale flags nothing)
    const uint32_t kthr = f2key(thr);
    uint32_t cnt = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) cnt += live && 4 * lg + r < F && k[r] > kthr;  // (padding: e >= F)
#pragma unroll
    for (int w = LG / 2; w >= 1; w /= 2) cnt += __shfl_xor(cnt, w, 64);
    if (!ok) return;  // (no shuffle below)
    if (lg == 0) {
      const int64_t e = o - a.out;
      if (oa.med) oa.med[e] = nan0 ? __uint_as_float(0x7fc00000u) : c;
      if (oa.mad) oa.mad[e] = sc;
      if (oa.count) oa.count[e] = cnt;
    }
    if (oa.mask) {
      uint8_t *m = outl_mask(a, oa, tile * (kBlock / LG) + threadIdx.x / LG);
      if (VEC) {
        if (4 * lg < F) {
          const float4 x = ld4(p + 4 * lg);
          outl_store4(m + 4 * lg, live && abs_dev(x.x, c) > thr, live && abs_dev(x.y, c) > thr,
                      live && abs_dev(x.z, c) > thr, live && abs_dev(x.w, c) > thr);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * lg + r < F)
            m[4 * lg + r] = live && abs_dev(p[(int64_t)(4 * lg + r) * a.in_cs], c) > thr;
      }
    }
  } else if constexpr (SEL == SEL_QUANTILES) {
    const QSet &s = first_arg(qs...);
    for (int kq = 0; kq < s.np; ++kq) {  // (uniform: pick shuffles, whole waves)
      const uint32_t ka = pick(s.rank[s.lo[kq]]), kb = pick(s.rank[s.hi[kq]]);
      if (ok && lg == 0) o[kq * s.out_ld_q] = quantile_of(ka, kb, s.g[kq], gnan);
    }
  } else if (ok && lg == 0) {
    if constexpr (SEL == SEL_QUANTILE) {
      *o = quantile_of(k0, k1, a.qg, gnan);
    } else {
      const float m = median_of(k0, k1, F & 1, gnan);
      *o = MAD ? mad_scale(m) : m;
    }
  }
}

// Count digit d of the lanes with pred in the wave's histogram h.  The digits
// of the first two leaders are counted once for the wave (spectra share their
// exponent byte, and tied data whole keys: all 64 lanes on one LDS counter
// otherwise); what is left goes one by one.  Called by whole waves.
__device__ __forceinline__ void hist_add(uint32_t *h, uint32_t d, bool pred) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const unsigned long long act = __ballot(pred);
    if (act == 0) return;  // (wave-uniform)
    const int lead = __ffsll(act) - 1;
    const uint32_t d0 = __shfl(d, lead, 64);
    const bool eq = pred && d == d0;
    const unsigned long long m = __ballot(eq);
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[d0], (uint32_t)__popcll(m));
    pred = pred && !eq;
  }
  if (pred) atomicAdd(&h[d], 1u);
}

// MAD: the four passes run twice, the second time over |x - c| with c the
// median the first found: the register keys are transformed in place (REG),
// or the block is read again and the deviations formed on the way (!REG).
// SEL_QUANTILE: the two ranks start at a.qrank and the next.  SEL_OUTLIERS:
// mad's eight passes, then the trailing OutlArgs' outputs (OA is empty for every
// other selector): the register keys of |x - c| are counted against the
// threshold's, or, for the mask and in the stream form, the block is read once
// more, the deviations formed on the way.
template <bool VEC, bool REG, Sel SEL, typename... OA>
__global__ __launch_bounds__(kBlock) void k_median_select(const RedArgs a, const OA... oas) {
  constexpr bool MAD = SEL == SEL_MAD || SEL == SEL_OUTLIERS;
  __shared__ uint32_t hist[2][256];
  __shared__ uint32_t wtot[2][4];
  __shared__ uint32_t sel[2][2];  // per rank: its digit, its rank among that digit's keys
  __shared__ int nanflag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *p = nullptr;
  float *o = nullptr;
  if (!stat_group(a, blockIdx.x, p, o)) return;  // (uniform)
  const int64_t F = a.F, n = VEC ? F / 4 : F;    // items: float4s or values
  float cen = 0.0f;  // MAD, second round: the block's median
  bool dev = false;  // MAD, second round (uniform): the keys are those of |x - cen|
  // item `it` (uniform loop index) of this thread: VEC 4 keys, else 1
  auto load = [&](int64_t it, uint32_t *k, bool &nan) {
    const int64_t idx = it * kBlock + tid;
    if (idx >= n) return false;
    if (VEC) {
      float4 x = ld4(p + 4 * idx);
      if (MAD && dev)
        x = make_float4(abs_dev(x.x, cen), abs_dev(x.y, cen), abs_dev(x.z, cen),
                        abs_dev(x.w, cen));
      nan = nan || x.x != x.x || x.y != x.y || x.z != x.z || x.w != x.w;
      k[0] = f2key(x.x), k[1] = f2key(x.y), k[2] = f2key(x.z), k[3] = f2key(x.w);
    } else {
      float x = p[idx * a.in_cs];
      if (MAD && dev) x = abs_dev(x, cen);
      nan = nan || x != x;
      k[0] = f2key(x);
    }
    return true;
  };
  constexpr int KPI = VEC ? 4 : 1;         // keys per item
  constexpr int NREG = VEC ? 4 : 16;       // items a lane keeps (REG)
  const int64_t nit = (n + kBlock - 1) / kBlock;  // items per thread (uniform)
  uint32_t keys[16];
  bool nan = false;
  if (REG) {
#pragma unroll
    for (int it = 0; it < NREG; ++it) (void)load(it, &keys[it * KPI], nan);
  }
  if (tid == 0) nanflag = 0;
  uint32_t pre0 = 0, pre1 = 0;                       // key bits fixed so far
  // rank among the prefix's keys
  uint32_t r0 = SEL == SEL_QUANTILE ? (uint32_t)a.qrank : (uint32_t)((F - 1) / 2);
  uint32_t r1 = SEL == SEL_QUANTILE ? (uint32_t)a.qrank + 1u : (uint32_t)(F / 2);
  bool nan0 = false;  // SEL_OUTLIERS: the block holds a NaN
  for (int pass = 0; pass < (MAD ? 8 : 4); ++pass) {
    if (MAD && pass == 4) {  // the median is known: the same four passes over |x - cen|
      cen = median_of(pre0, pre1, F & 1, false);  // (a NaN block: NaN below, whatever cen is)
      // (pass 0's flag; pass 4 sets it again only behind its first barrier)
      if constexpr (SEL == SEL_OUTLIERS) nan0 = nanflag != 0;
      dev = true;
      if (REG) {
#pragma unroll
        for (int it = 0; it < NREG; ++it) {
          if ((int64_t)it * kBlock + tid < n) {
#pragma unroll
            for (int c = 0; c < KPI; ++c) {
              const float d = abs_dev(key2f(keys[it * KPI + c]), cen);
              nan = nan || d != d;
              keys[it * KPI + c] = f2key(d);
            }
          }
        }
      }
      pre0 = pre1 = 0;
      r0 = (uint32_t)((F - 1) / 2), r1 = (uint32_t)(F / 2);
    }
    const int ps = MAD ? pass & 3 : pass;  // the pass of this selection
    const int shift = 24 - 8 * ps;
    const uint32_t mask = ps == 0 ? 0u : 0xffffffffu << (shift + 8);
    const bool same = pre0 == pre1;
    hist[0][tid] = 0;
    hist[1][tid] = 0;
    __syncthreads();
    auto count = [&](uint32_t key, bool valid) {
      const uint32_t d = (key >> shift) & 255u;
      hist_add(hist[0], d, valid && (key & mask) == pre0);
      if (!same) hist_add(hist[1], d, valid && (key & mask) == pre1);
    };
    if (REG) {
#pragma unroll
      for (int it = 0; it < NREG; ++it) {
        const bool valid = (int64_t)it * kBlock + tid < n;
#pragma unroll
        for (int c = 0; c < KPI; ++c) count(keys[it * KPI + c], valid);
      }
    } else {
      for (int64_t it = 0; it < nit; ++it) {
        uint32_t k[4] = {0, 0, 0, 0};
        const bool valid = load(it, k, nan);
#pragma unroll
        for (int c = 0; c < KPI; ++c) count(k[c], valid);
      }
    }
    if (ps == 0 && nan) nanflag = 1;
    __syncthreads();
    // inclusive scan of the 256 bins: in the wave, then over the waves
    const uint32_t c0 = hist[0][tid], c1 = same ? c0 : hist[1][tid];
    uint32_t i0 = c0, i1 = c1;
#pragma unroll
    for (int w = 1; w < 64; w *= 2) {
      const uint32_t u0 = __shfl_up(i0, w, 64), u1 = __shfl_up(i1, w, 64);
      if (lane >= w) i0 += u0, i1 += u1;
    }
    if (lane == 63) wtot[0][wave] = i0, wtot[1][wave] = i1;
    __syncthreads();
    for (int w = 0; w < wave; ++w) i0 += wtot[0][w], i1 += wtot[1][w];
    // the bin whose keys hold the rank
    if (c0 && i0 - c0 <= r0 && r0 < i0) sel[0][0] = tid, sel[0][1] = r0 - (i0 - c0);
    if (c1 && i1 - c1 <= r1 && r1 < i1) sel[1][0] = tid, sel[1][1] = r1 - (i1 - c1);
    __syncthreads();
    pre0 |= sel[0][0] << shift;
    r0 = sel[0][1];
    pre1 |= sel[1][0] << shift;
    r1 = sel[1][1];
  }
  if constexpr (SEL == SEL_OUTLIERS) {
    const OutlArgs &oa = first_arg(oas...);
    const float sc = mad_scale(median_of(pre0, pre1, F & 1, nanflag != 0));
    const float thr = outl_thr(oa.nsigma, sc);
    const bool live = nanflag == 0 && thr == thr;  // (a NaN median or scale flags nothing)
    const uint32_t kthr = f2key(thr);
    uint32_t cnt = 0;
    if (REG && !oa.mask) {
#pragma unroll
      for (int it = 0; it < NREG; ++it) {
        const bool valid = (int64_t)it * kBlock + tid < n;
#pragma unroll
        for (int c = 0; c < KPI; ++c) cnt += live && valid && keys[it * KPI + c] > kthr;
      }
    } else {  // one more read: the keys of |x - cen| (dev is set) with their positions
      uint8_t *m = oa.mask ? outl_mask(a, oa, blockIdx.x) : nullptr;
      for (int64_t it = 0; it < nit; ++it) {
        uint32_t k[4] = {0, 0, 0, 0};
        bool unused = false;
        if (!load(it, k, unused)) continue;
        const int64_t idx = it * kBlock + tid;
        bool f[KPI];
#pragma unroll
        for (int c = 0; c < KPI; ++c) f[c] = live && k[c] > kthr, cnt += f[c];
        if (m) {
          if constexpr (VEC)
            outl_store4(m + 4 * idx, f[0], f[1], f[2], f[3]);
          else
            m[idx] = f[0];
        }
      }
    }
#pragma unroll
    for (int w = 32; w >= 1; w /= 2) cnt += __shfl_xor(cnt, w, 64);
    if (lane == 0) wtot[0][wave] = cnt;  // (free: the last pass's barrier is behind every reader)
    __syncthreads();
    if (tid == 0) {
      const int64_t e = o - a.out;
      if (oa.med) oa.med[e] = nan0 ? __uint_as_float(0x7fc00000u) : cen;
      if (oa.mad) oa.mad[e] = sc;
      if (oa.count) oa.count[e] = (wtot[0][0] + wtot[0][1]) + (wtot[0][2] + wtot[0][3]);
    }
  } else if (tid == 0) {
    if constexpr (SEL == SEL_QUANTILE) {
      *o = quantile_of(pre0, pre1, a.qg, nanflag != 0);
    } else {
      const float m = median_of(pre0, pre1, F & 1, nanflag != 0);
      *o = MAD ? mad_scale(m) : m;
    }
  }
}

// quantiles(ps): k_median_select's select for the qs.nr sorted ranks of a QSet
// at once (the file's head).  State per rank in LDS: pre, the key bits fixed
// so far, and rem, its rank among the keys with that prefix (two copies by
// pass parity: a pass reads one and writes the other).  Every pass: wave 0
// lists the distinct prefixes (slots), everyone counts its keys at slot * 256 +
// digit, wave w scans slots w, w + 4, ... (4 bins a lane) and settles their
// ranks.  REG: the keys stay in registers, else every pass reads the block.
template <bool VEC, bool REG>
__global__ __launch_bounds__(kBlock) void k_quantiles_select(const RedArgs a, const QSet qs) {
  constexpr int NR = 2 * BLDP_MAX_QUANTILES;
  __shared__ uint32_t hist[NR * 256];
  __shared__ uint32_t pre[NR];
  __shared__ uint32_t rem[2][NR];
  __shared__ uint32_t dpre[NR];    // the distinct prefixes, ascending
  __shared__ int sfirst[NR + 1];   // slot s holds ranks sfirst[s] .. sfirst[s + 1] - 1
  __shared__ int nslot;
  __shared__ int nanflag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *p = nullptr;
  float *o = nullptr;
  if (!stat_group(a, blockIdx.x, p, o)) return;  // (uniform)
  const int64_t F = a.F, n = VEC ? F / 4 : F;    // items: float4s or values
  const int nr = qs.nr;
  auto load = [&](int64_t it, uint32_t *k, bool &nan) {
    const int64_t idx = it * kBlock + tid;
    if (idx >= n) return false;
    if (VEC) {
      const float4 x = ld4(p + 4 * idx);
      nan = nan || x.x != x.x || x.y != x.y || x.z != x.z || x.w != x.w;
      k[0] = f2key(x.x), k[1] = f2key(x.y), k[2] = f2key(x.z), k[3] = f2key(x.w);
    } else {
      const float x = p[idx * a.in_cs];
      nan = nan || x != x;
      k[0] = f2key(x);
    }
    return true;
  };
  constexpr int KPI = VEC ? 4 : 1;                // keys per item
  constexpr int NREG = VEC ? 4 : 16;              // items a lane keeps (REG)
  const int64_t nit = (n + kBlock - 1) / kBlock;  // items per thread (uniform)
  uint32_t keys[16];
  bool nan = false;
  if (REG) {
#pragma unroll
    for (int it = 0; it < NREG; ++it) (void)load(it, &keys[it * KPI], nan);
  }
  if (tid < NR) {
    pre[tid] = 0;
    rem[0][tid] = tid < nr ? (uint32_t)qs.rank[tid] : 0u;
  }
  if (tid == 0) nanflag = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass, par = pass & 1;
    const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    __syncthreads();  // (pre and rem of the pass before)
    if (wave == 0) {
      const uint32_t mine = lane < nr ? pre[lane] : 0u;
      const uint32_t prev = __shfl_up(mine, 1, 64);
      const bool head = lane < nr && (lane == 0 || mine != prev);
      const unsigned long long hb = __ballot(head);
      if (head) {
        const int s = __popcll(hb & ((1ull << lane) - 1ull));
        dpre[s] = mine;
        sfirst[s] = lane;
      }
      if (lane == 0) {
        nslot = __popcll(hb);
        sfirst[__popcll(hb)] = nr;
      }
    }
    __syncthreads();
    const int ns = nslot;  // (uniform, 1 .. nr)
    for (int k = tid; k < ns * 256; k += kBlock) hist[k] = 0;
    __syncthreads();
    // a key has the prefix of at most one slot
    auto count = [&](uint32_t key, bool valid) {
      const uint32_t pk = key & mask;
      int sl = -1;
      for (int s = 0; s < ns; ++s) sl = pk == dpre[s] ? s : sl;
      hist_add(hist, (uint32_t)(sl < 0 ? 0 : sl) * 256u + ((key >> shift) & 255u),
               valid && sl >= 0);
    };
    if (REG) {
#pragma unroll
      for (int it = 0; it < NREG; ++it) {
        const bool valid = (int64_t)it * kBlock + tid < n;
#pragma unroll
        for (int c = 0; c < KPI; ++c) count(keys[it * KPI + c], valid);
      }
    } else {
      for (int64_t it = 0; it < nit; ++it) {
        uint32_t k[4] = {0, 0, 0, 0};
        const bool valid = load(it, k, nan);
#pragma unroll
        for (int c = 0; c < KPI; ++c) count(k[c], valid);
      }
    }
    if (pass == 0 && nan) nanflag = 1;
    __syncthreads();
    for (int s = wave; s < ns; s += kBlock / 64) {  // (uniform in the wave)
      const uint32_t *h = hist + s * 256 + 4 * lane;
      const uint32_t c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
      const uint32_t tot = (c0 + c1) + (c2 + c3);
      uint32_t incl = tot;
#pragma unroll
      for (int w = 1; w < 64; w *= 2) {
        const uint32_t u = __shfl_up(incl, w, 64);
        if (lane >= w) incl += u;
      }
      const uint32_t excl = incl - tot;
      for (int r = sfirst[s]; r < sfirst[s + 1]; ++r) {
        const uint32_t want = rem[par][r];
        if (excl <= want && want < incl) {  // (one lane: the bins holding the rank)
          uint32_t acc = excl, d = 0;
          if (want >= acc + c0) {
            acc += c0, d = 1;
            if (want >= acc + c1) {
              acc += c1, d = 2;
              if (want >= acc + c2) acc += c2, d = 3;
            }
          }
          pre[r] |= (uint32_t)(4 * lane + d) << shift;
          rem[par ^ 1][r] = want - acc;
        }
      }
    }
  }
  __syncthreads();
  if (tid < qs.np)
    o[tid * qs.out_ld_q] =
        quantile_of(pre[qs.lo[tid]], pre[qs.hi[tid]], qs.g[tid], nanflag != 0);
}

}  // namespace

int plan_stats(RedArgs &a, int op, bool words, int xcd_lg, Plan *pp) {
  Plan p{};
  const int64_t F = a.F;
  p.nout = a.nco * a.ni * a.nto;
  a.ts = 1;
  a.tpb = 1;
  a.tsub_log2 = 0;
  a.rsplit = 1;
  a.bpack = 0;
  a.st_plain = 1;
  a.vec_out = 0;
  a.nchunk = 1;
  a.rows_per_chunk = 1;
  a.blocks_c = 1;
  a.div = (float)F;
  a.k4 = (words && F % 4 == 0) ? 1 : 0;  // float4 loads
  const int64_t items = a.k4 ? F / 4 : F;
  auto pow2_lanes = [](int64_t n) {
    int l = 1;
    while (l < 64 && l < n) l *= 2;
    return l;
  };
  // F = 1: fqav(A, n <= 1) returns A whatever f is (src/gbtworkerfunctions.jl:17),
  // which is what the median of one element copies
  // (mad: the median's path, its selection run twice; quantile: its ranks moved)
  if (median_op(op) || F == 1) {
    if (F >= ((int64_t)1 << 31))
      return set_error(BLDP_EINVAL, "median: fqavby=%lld is beyond 2^31 - 1", (long long)F);
    if (F <= kSortMaxF) {
      p.path = PATH_MEDIAN_SORT;
      p.lpg = pow2_lanes((F + 3) / 4);
    } else {
      p.path = F <= kRegMaxF ? PATH_MEDIAN_SELECT : PATH_MEDIAN_STREAM;
      p.lpg = kBlock;
    }
  } else {
    p.path = PATH_MOMENTS;
    p.lpg = F <= kLaneMaxF ? pow2_lanes(items) : kBlock;
  }
  // one block per workgroup, or kBlock / lpg of them side by side
  a.ntiles = p.lpg == kBlock ? p.nout : (p.nout + kBlock / p.lpg - 1) / (kBlock / p.lpg);
  if (a.ntiles > INT32_MAX)
    return set_error(BLDP_EINVAL,
                     "median/var/std/mad/quantile: %lld blocks of %lld are too many for one launch",
                     (long long)p.nout, (long long)F);
  p.grid = a.ntiles;
  p.ws_bytes = 0;
  // the per-XCD tile order where neighbouring workgroups read neighbouring
  // memory, as k_reduce_vec (kernels.hip xcd_order_pays); a workgroup per block: off
  a.xcd_lg = p.lpg == kBlock ? 0 : xcd_lg;
  *pp = p;
  return BLDP_OK;
}


namespace {
}  // namespace

hipError_t launch_stats(const RedArgs &a, const Plan &p, int op, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  const dim3 grid((unsigned)p.grid, (unsigned)a.nbank);
  const auto go = [&](auto *kn, auto... args) {
    return launch_kernel(kn, grid, dim3(kBlock), 0, s, args...);
  };
  const bool vec = a.k4 != 0;
  // (F = 1: the copy, as every op)
  const Sel sel = a.F <= 1 ? SEL_MEDIAN
                           : op == BLDP_OP_MAD ? SEL_MAD : op == kOpQuantile ? SEL_QUANTILE : SEL_MEDIAN;
  if (sel == SEL_QUANTILE && (a.qrank < 0 || (int64_t)a.qrank + 1 >= a.F))
    return hipErrorInvalidValue;  // (the upper rank must be a key of the block)
#define BLDP_VECSEL(KN, N) (vec ? KN<N, true> : KN<N, false>)
  switch (p.path) {
    case PATH_MOMENTS:
      switch (p.lpg) {
        case 1: return go(BLDP_VECSEL(k_mom_lanes, 1), a, op);
        case 2: return go(BLDP_VECSEL(k_mom_lanes, 2), a, op);
        case 4: return go(BLDP_VECSEL(k_mom_lanes, 4), a, op);
        case 8: return go(BLDP_VECSEL(k_mom_lanes, 8), a, op);
        case 16: return go(BLDP_VECSEL(k_mom_lanes, 16), a, op);
        case 32: return go(BLDP_VECSEL(k_mom_lanes, 32), a, op);
        case 64: return go(BLDP_VECSEL(k_mom_lanes, 64), a, op);
        case kBlock: return go(vec ? k_mom_block<true> : k_mom_block<false>, a, op);
      }
      break;
#undef BLDP_VECSEL
#define BLDP_MEDSEL(KN, A, B)               \
  (sel == SEL_MAD ? KN<A, B, SEL_MAD>       \
                  : sel == SEL_QUANTILE ? KN<A, B, SEL_QUANTILE> : KN<A, B, SEL_MEDIAN>)
#define BLDP_VECSEL(KN, N) (vec ? BLDP_MEDSEL(KN, N, true) : BLDP_MEDSEL(KN, N, false))
    case PATH_MEDIAN_SORT:
      switch (p.lpg) {  // lanes of 4 keys
        case 1: return go(BLDP_VECSEL(k_median_sort, 4), a);
        case 2: return go(BLDP_VECSEL(k_median_sort, 8), a);
        case 4: return go(BLDP_VECSEL(k_median_sort, 16), a);
        case 8: return go(BLDP_VECSEL(k_median_sort, 32), a);
        case 16: return go(BLDP_VECSEL(k_median_sort, 64), a);
      }
      break;
    case PATH_MEDIAN_SELECT:
      return go(vec ? BLDP_MEDSEL(k_median_select, true, true)
                    : BLDP_MEDSEL(k_median_select, false, true), a);
    case PATH_MEDIAN_STREAM:
      return go(vec ? BLDP_MEDSEL(k_median_select, true, false)
                    : BLDP_MEDSEL(k_median_select, false, false), a);
#undef BLDP_VECSEL
#undef BLDP_MEDSEL
  }
  return hipErrorInvalidValue;
}

int stats_q_reads(const Plan &p) { return p.path == PATH_MEDIAN_STREAM ? 4 : 1; }

// mad's 8 reads and the flag pass; the register forms read once, and once more
// for the positions of a mask
int stats_outl_reads(const Plan &p, bool mask) {
  return p.path == PATH_MEDIAN_STREAM ? 9 : mask ? 2 : 1;
}

hipError_t launch_stats_outl(const RedArgs &a, const Plan &p, const OutlArgs &oa, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  if (a.F < 2 || a.out || !(oa.nsigma >= 0.0 && oa.nsigma <= 1.7976931348623157e308))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)p.grid, (unsigned)a.nbank);
  const auto go = [&](auto *kn) { return launch_kernel(kn, grid, dim3(kBlock), 0, s, a, oa); };
  const bool vec = a.k4 != 0;
#define BLDP_OSORT(N)                                         \
  (vec ? k_median_sort<N, true, SEL_OUTLIERS, OutlArgs>       \
       : k_median_sort<N, false, SEL_OUTLIERS, OutlArgs>)
#define BLDP_OSEL(REG)                                        \
  (vec ? k_median_select<true, REG, SEL_OUTLIERS, OutlArgs>   \
       : k_median_select<false, REG, SEL_OUTLIERS, OutlArgs>)
  switch (p.path) {
    case PATH_MEDIAN_SORT:
      switch (p.lpg) {  // lanes of 4 keys
        case 1: return go(BLDP_OSORT(4));
        case 2: return go(BLDP_OSORT(8));
        case 4: return go(BLDP_OSORT(16));
        case 8: return go(BLDP_OSORT(32));
        case 16: return go(BLDP_OSORT(64));
      }
      break;
    case PATH_MEDIAN_SELECT: return go(BLDP_OSEL(true));
    case PATH_MEDIAN_STREAM: return go(BLDP_OSEL(false));
  }
#undef BLDP_OSORT
#undef BLDP_OSEL
  return hipErrorInvalidValue;
}

hipError_t launch_stats_q(const RedArgs &a, const Plan &p, const QSet &qs, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  // (every rank must be a key of the block; the kernels index by these counts)
  if (a.F < 2 || qs.np < 1 || qs.np > BLDP_MAX_QUANTILES || qs.nr < 1 ||
      qs.nr > 2 * BLDP_MAX_QUANTILES)
    return hipErrorInvalidValue;
  for (int r = 0; r < qs.nr; ++r)
    if (qs.rank[r] < 0 || qs.rank[r] >= a.F || (r && qs.rank[r] <= qs.rank[r - 1]))
      return hipErrorInvalidValue;
  for (int k = 0; k < qs.np; ++k)
    if (qs.lo[k] >= qs.nr || qs.hi[k] >= qs.nr) return hipErrorInvalidValue;
  const dim3 grid((unsigned)p.grid, (unsigned)a.nbank);
  const auto go = [&](auto *kn) { return launch_kernel(kn, grid, dim3(kBlock), 0, s, a, qs); };
  const bool vec = a.k4 != 0;
#define BLDP_QSORT(N) \
  (vec ? k_median_sort<N, true, SEL_QUANTILES, QSet> : k_median_sort<N, false, SEL_QUANTILES, QSet>)
  switch (p.path) {
    case PATH_MEDIAN_SORT:
      switch (p.lpg) {  // lanes of 4 keys
        case 1: return go(BLDP_QSORT(4));
        case 2: return go(BLDP_QSORT(8));
        case 4: return go(BLDP_QSORT(16));
        case 8: return go(BLDP_QSORT(32));
        case 16: return go(BLDP_QSORT(64));
      }
      break;
#undef BLDP_QSORT
    case PATH_MEDIAN_SELECT:
      return go(vec ? k_quantiles_select<true, true> : k_quantiles_select<false, true>);
    case PATH_MEDIAN_STREAM:
      return go(vec ? k_quantiles_select<true, false> : k_quantiles_select<false, false>);
  }
  return hipErrorInvalidValue;
}

}  // namespace bldp
