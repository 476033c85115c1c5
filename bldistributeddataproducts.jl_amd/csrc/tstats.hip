// tstats.hip — tavfunc median, var and std of Float32 windows (gfx950).
//
// Julia's Statistics applied along time, fqav's rule on axis 3: one result per
// block of T selected spectra (b T .. b T + T - 1) of every (channel, IF)
// column, R[c, i, b] = f(A[c, i, bT+1 : (b+1)T]).  The rules are those of
// stats.hip (the channel-axis forms): the corrected variance about the mean,
// its root, the median ordered by isless with middle(a, b) = a/2 + b/2 of an
// even block and NaN for a block holding a NaN.
//
// The window geometry is the reduce's (any channel offset, step and direction,
// IF and time steps).  A column's T values lie in_ld_t apart, so consecutive
// lanes own consecutive channels and every load is a row segment: float4 per
// lane (4 columns) on unit-step windows whose channel count is a multiple of
// 4, at any dword alignment (f4u), one dword per lane otherwise.
//
//   T <= 32    register form (k_tstat_regs): a lane holds its columns' T values
//              in registers, templated on the next power of two and fully
//              unrolled (a register array indexed at run time would go to
//              scratch).  var / std: mean = K + sum(x - K) / T with K the
//              block's first element, then the squared deviations (the recipe
//              of stats.hip k_mom_lanes: a constant block gives exactly 0.0).
//              median: the order-preserving uint32 keys, padded with the
//              maximal key, through a bitonic compare-exchange network in
//              registers; the two ranks are picked by an unrolled chain.
//   T > 32     split form: a workgroup takes a tile of 2^lx_log2 lanes of
//              channels and one block; its 256 >> lx_log2 time slices stride
//              the block's spectra and meet through LDS.
//              k_tstat_mom_split: two passes (sum(x - K), then the squared
//              deviations about the mean; the second read hits L2 / MALL where
//              the tile's block fits), Float64 accumulators.  Blocks too few
//              to fill the GPU are cut into time chunks, one workgroup each:
//              k_tstat_mom_chunk leaves the chunks' partials in a workspace
//              (sum(x - K), then the squared deviations about the mean of the
//              partials added in chunk order), k_tstat_mom_finish adds them.
//              k_tstat_med_split: an MSB-first radix select of rank (T-1)/2,
//              8 bits a pass, one 256-bin LDS histogram per column (<= 32
//              columns a workgroup), the block re-read every pass.  The last
//              pass also tells how many keys equal the selected one; rank T/2
//              of an even block is that key again, or else the smallest key
//              above it, found by a fifth pass.
//   mad        (stats.hip's rule) the median's two forms with their selection
//              run twice: the register form sorts the keys of |x - median| made
//              from its sorted keys, the split form repeats its passes forming
//              the deviations from the block as it re-reads it.
//   quantile   (stats.hip's rule) the median's two forms selecting the run-time
//              ranks q = TStatArgs.qrank and q + 1: the register form's chain
//              compares against them, the split form selects rank q and always
//              runs its fifth pass (rank q + 1 is the same key again or the
//              smallest above it); quantile_of joins the two with weight qg.
//   quantiles  (stats.hip's rule) K <= 8 quantiles from one selection, the ranks
//              in a QSet (bldp_impl.h), a kernel argument of these
//              instantiations alone; plane k lies k * out_ld_q after plane 0.
//              Register form (k_tstat_regs, MED = 4): one sort, then the
//              unrolled chain and a store per plane.  One read of the block.
//              Split form (k_tquantiles_split): the L distinct lower ranks
//              j_k - 1 are selected as the quantile form selects its one, each
//              followed by "the same key again or the smallest key above it".
//              Pass 0 builds one histogram per column and serves all L ranks.
//              Passes 1 to 3 and the pass for the smallest key above run in
//              sweeps of G = min(L, 3) ranks, one histogram per (rank, column).
//              L = 1 keeps the quantile form's tile, 32 columns a workgroup
//              (32 KiB of LDS); L >= 2 takes 16 columns (G x 16 KiB = 32 or 48
//              KiB, three workgroups a CU: 64-byte row segments, as the
//              moments' narrowed tile).  Reads of the block: 1 + 4 ceil(L / G),
//              that is 5, 5, 5, 9, 9, 9, 13, 13 for L = 1 .. 8 (K separate
//              calls: 5 K).
//   outliers   (stats.hip's rule) mad's two selections, then what the trailing
//              OutlArgs (bldp_impl.h) asks for: median, scaled mad, the count of
//              samples with |x - c| > thr and the flags.  Register form
//              (k_tstat_regs, MED = 5): the sorted keys of |x - c| against the
//              threshold's key; the mask reloads the block (1 read, 2 with a
//              mask; a lane's 4 columns pack their flags into a dword).  Split
//              form (k_tstat_med_split, SEL_OUTLIERS): one more pass of the time
//              slices over the block, their counts added in LDS (mad's reads
//              and 1).
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

constexpr int64_t kRegMaxT = 32;  // k_tstat_regs
constexpr int kMedCols = 32;      // k_tstat_med_split: columns (histograms) per workgroup
constexpr int kScanLanes = kBlock / kMedCols;  // lanes scanning one column's histogram
constexpr int kScanBins = 256 / kScanLanes;    // bins each of them sums
constexpr int64_t kChunkMin = 4096;            // chunked moments: spectra a chunk, at least

// the CPL values of consecutive channels at p (CPL = 4: unit channel step)
template <int CPL>
__device__ __forceinline__ void ldcols(const float *p, float (&x)[CPL]) {
  if constexpr (CPL == 4) {
    const f4u v = *reinterpret_cast<const f4u *>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
    x[0] = *p;
  }
}

// q = x / d, r = x % d for x >= 0 and a wave-uniform d > 0 (stats.hip divmod)
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

// isless order of Float32 as unsigned order (NaN aside), as stats.hip
__device__ __forceinline__ uint32_t f2key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// Statistics.middle(a, b) = a/2 + b/2, each half rounded before the sum.  The
// products must not be contracted into a fused multiply-add: fma(a, 0.5, b/2)
// of a = -1e-45, b = 0 keeps the exact -2^-150 and rounds to -0.0 where
// -0.0 + 0.0 is +0.0 (hipcc contracts by default, __fmul_rn or not).
__device__ __forceinline__ float middle(float x, float y) {
#pragma clang fp contract(off)
  const float hx = x * 0.5f, hy = y * 0.5f;
  return hx + hy;
}
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

// ---------------------------------------------------------------------------
// T <= TP <= 32: the block in registers

// Bitonic network over the time index of a lane's TP keys per column: runs of
// kk keys, ascending where (e & kk) == 0; every index is a compile-time constant.
template <int TP, int CPL>
__device__ __forceinline__ void bitonic_cols(uint32_t (&k)[TP][CPL]) {
#pragma unroll
  for (int kk = 2; kk <= TP; kk *= 2) {
#pragma unroll
    for (int j = kk / 2; j >= 1; j /= 2) {
#pragma unroll
      for (int e = 0; e < TP; ++e) {
        if ((e & j) == 0) {
          const bool up = kk == TP || (e & kk) == 0;
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            const uint32_t lo = min(k[e][c], k[e | j][c]), hi = max(k[e][c], k[e | j][c]);
            k[e][c] = up ? lo : hi;
            k[e | j][c] = up ? hi : lo;
          }
        }
      }
    }
  }
}

// MED: 0 var / std, 1 median, 2 mad (the network runs again over |x - median|),
// 3 quantile (ranks a.qrank and the next, wave-uniform, compared in the chain),
// 4 quantiles (one more argument, the QSet: QS is empty for every other MED,
// whose signature is (TStatArgs, int); the chain and a store per plane),
// 5 outliers (mad's two sorts, then the trailing OutlArgs' outputs: the sorted
// keys of |x - median| above the threshold's are counted, and the mask reloads
// the block for their positions)
template <typename T>
__device__ __forceinline__ const T &first_arg(const T &x) {
  return x;
}
template <int TP, int CPL, int MED, typename... QS>
__global__ __launch_bounds__(kBlock) void k_tstat_regs(const TStatArgs a, const int op,
                                                       const QS... qs) {
  const int64_t tile = xcd_order(blockIdx.x, gridDim.x, a.xcd_lg);
  const int64_t item = tile * kBlock + threadIdx.x;
  if (item >= a.ncg * a.ni * a.nb) return;  // (no shuffle or barrier below)
  int64_t cg, r, i, b;
  divmod(item, a.ncg, r, cg);
  divmod(r, a.ni, b, i);
  const float *p = a.in[blockIdx.y] + a.in_off + cg * CPL * a.in_cs + i * a.in_ld_i +
                   b * a.T * a.in_ld_t;
  float *o = a.out + blockIdx.y * a.out_bank + cg * CPL + i * a.out_ld_i + b * a.out_ld_b;
  const int T = (int)a.T;
  float v[TP][CPL];
#pragma unroll
  for (int t = 0; t < TP; ++t)
    if (t < T) ldcols<CPL>(p + t * a.in_ld_t, v[t]);
  if constexpr (!MED) {
    const float n = (float)T;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const float K = v[0][c];
      float s = 0.0f;  // of x - K
#pragma unroll
      for (int t = 0; t < TP; ++t)
        if (t < T) s += v[t][c] - K;
      const float mean = K + s / n;
      float q = 0.0f;
#pragma unroll
      for (int t = 0; t < TP; ++t)
        if (t < T) {
          const float d = v[t][c] - mean;
          q += d * d;
        }
      const float var = q / (n - 1.0f);
      o[c] = op == BLDP_OP_STD ? sqrtf(var) : var;
    }
  } else {
    uint32_t k[TP][CPL];
    bool nan[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) nan[c] = false;
#pragma unroll
    for (int t = 0; t < TP; ++t)
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        if (t < T) {
          nan[c] = nan[c] || v[t][c] != v[t][c];
          k[t][c] = f2key(v[t][c]);
        } else {
          k[t][c] = kPadKey;
        }
      }
    bitonic_cols<TP, CPL>(k);
    // ranks (T-1)/2 and T/2 (the same for odd T); the padding sorts above them
    const int q0 = MED == 3 ? a.qrank : (T - 1) / 2;
    const int q1 = MED == 3 ? a.qrank + 1 : T / 2;
    auto ranks = [&](int c, uint32_t &k0, uint32_t &k1) {
      k0 = 0, k1 = 0;
#pragma unroll
      for (int e = 0; e < TP; ++e) {
        k0 = e == q0 ? k[e][c] : k0;
        k1 = e == q1 ? k[e][c] : k1;
      }
    };
    float cen[CPL];  // mad, outliers: the columns' medians
    bool nan0[CPL];  // outliers: the block holds a NaN
    if constexpr (MED == 2 || MED == 5) {
      // the sorted keys (the padding is at e >= T) become those of |x - median|
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        uint32_t k0, k1;
        ranks(c, k0, k1);
        cen[c] = median_of(k0, k1, T & 1, false);  // (a NaN block: NaN below)
        nan0[c] = nan[c];
#pragma unroll
        for (int e = 0; e < TP; ++e)
          if (e < T) {
            const float d = abs_dev(key2f(k[e][c]), cen[c]);
            nan[c] = nan[c] || d != d;
            k[e][c] = f2key(d);
          }
      }
      bitonic_cols<TP, CPL>(k);
    }
    if constexpr (MED == 5) {
      const OutlArgs &oa = first_arg(qs...);
      const int64_t eo = o - a.out;
      float thr[CPL];
      bool live[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        uint32_t k0, k1;
        ranks(c, k0, k1);
        const float sc = mad_scale(median_of(k0, k1, T & 1, nan[c]));
        thr[c] = outl_thr(oa.nsigma, sc);
        live[c] = !nan[c] && thr[c] == thr[c];  // (a NaN median or scale flags nothing)
        const uint32_t kthr = f2key(thr[c]);
        uint32_t cnt = 0;
#pragma unroll
        for (int e = 0; e < TP; ++e) cnt += live[c] && e < T && k[e][c] > kthr;
        if (oa.med) oa.med[eo + c] = nan0[c] ? __uint_as_float(0x7fc00000u) : cen[c];
        if (oa.mad) oa.mad[eo + c] = sc;
        if (oa.count) oa.count[eo + c] = cnt;
      }
      if (oa.mask) {
        uint8_t *m = oa.mask + blockIdx.y * oa.mask_bank + cg * CPL + i * oa.mask_ld_i +
                     b * a.T * oa.mask_ld_t;
#pragma unroll
        for (int t = 0; t < TP; ++t)
          if (t < T) {
            float x[CPL];
            ldcols<CPL>(p + t * a.in_ld_t, x);
            bool f[CPL];
#pragma unroll
            for (int c = 0; c < CPL; ++c) f[c] = live[c] && abs_dev(x[c], cen[c]) > thr[c];
            if constexpr (CPL == 4)
              outl_store4(m + t * oa.mask_ld_t, f[0], f[1], f[2], f[3]);
            else
              m[t * oa.mask_ld_t] = f[0];
          }
      }
      return;
    }
    if constexpr (MED == 4) {
      const QSet &s = first_arg(qs...);
      for (int kq = 0; kq < s.np; ++kq) {  // (uniform)
        const int qa = s.rank[s.lo[kq]], qb = s.rank[s.hi[kq]];
        const double g = s.g[kq];
        float *const oq = o + kq * s.out_ld_q;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          uint32_t ka = 0, kb = 0;
#pragma unroll
          for (int e = 0; e < TP; ++e) {
            ka = e == qa ? k[e][c] : ka;
            kb = e == qb ? k[e][c] : kb;
          }
          oq[c] = quantile_of(ka, kb, g, nan[c]);
        }
      }
      return;
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      uint32_t k0, k1;
      ranks(c, k0, k1);
      if constexpr (MED == 3) {
        o[c] = quantile_of(k0, k1, a.qg, nan[c]);
      } else {
        const float m = median_of(k0, k1, T & 1, nan[c]);
        o[c] = MED == 2 ? mad_scale(m) : m;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// T > 32: the time slices of a workgroup split the block

// The tile of workgroup x: channel tile ct of (IF i, block b); thread tid is
// lane tx of the tile's lx lanes (column group cg) in time slice ty.
struct SplitGeo {
  int lx, tx, ty, ny;
  int64_t cg, i, b;
  bool ok;  // the column group exists
};
__device__ __forceinline__ SplitGeo split_geo(const TStatArgs &a) {
  SplitGeo g;
  g.lx = 1 << a.lx_log2;
  g.tx = threadIdx.x & (g.lx - 1);
  g.ty = threadIdx.x >> a.lx_log2;
  g.ny = kBlock >> a.lx_log2;
  int64_t ct, r;
  divmod(blockIdx.x, a.ctiles, r, ct);
  divmod(r, a.ni, g.b, g.i);
  g.cg = ct * g.lx + g.tx;
  g.ok = g.cg < a.ncg;
  return g;
}

template <int CPL>
__global__ __launch_bounds__(kBlock) void k_tstat_mom_split(const TStatArgs a, const int op) {
  __shared__ double sh[kBlock][CPL];
  const SplitGeo g = split_geo(a);
  const int64_t T = a.T;
  const float *p = a.in[blockIdx.y] + a.in_off + (g.ok ? g.cg : 0) * CPL * a.in_cs +
                   g.i * a.in_ld_i + g.b * T * a.in_ld_t;
  // sum over the time slices of this lane's columns, the same value (the same
  // order of additions) in every slice
  auto meet = [&](double (&x)[CPL]) {
    __syncthreads();  // (sh is free again)
#pragma unroll
    for (int c = 0; c < CPL; ++c) sh[threadIdx.x][c] = x[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CPL; ++c) x[c] = 0.0;
    for (int y = 0; y < g.ny; ++y)
#pragma unroll
      for (int c = 0; c < CPL; ++c) x[c] += sh[y * g.lx + g.tx][c];
  };
  float K[CPL];  // the block's first element
#pragma unroll
  for (int c = 0; c < CPL; ++c) K[c] = 0.0f;
  if (g.ok) ldcols<CPL>(p, K);
  double s[CPL];  // of x - K
#pragma unroll
  for (int c = 0; c < CPL; ++c) s[c] = 0.0;
  if (g.ok) {
#pragma unroll 4
    for (int64_t t = g.ty; t < T; t += g.ny) {
      float x[CPL];
      ldcols<CPL>(p + t * a.in_ld_t, x);
#pragma unroll
      for (int c = 0; c < CPL; ++c) s[c] += (double)x[c] - (double)K[c];
    }
  }
  meet(s);
  double mean[CPL], q[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) mean[c] = (double)K[c] + s[c] / (double)T, q[c] = 0.0;
  if (g.ok) {
#pragma unroll 4
    for (int64_t t = g.ty; t < T; t += g.ny) {
      float x[CPL];
      ldcols<CPL>(p + t * a.in_ld_t, x);
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const double d = (double)x[c] - mean[c];
        q[c] += d * d;
      }
    }
  }
  meet(q);
  if (g.ok && g.ty == 0) {
    float *o = a.out + blockIdx.y * a.out_bank + g.cg * CPL + g.i * a.out_ld_i + g.b * a.out_ld_b;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      // std is the root of the Float32 variance (Julia's sqrt(var(x))): Inf
      // where the variance overflows Float32
      const float var = (float)(q[c] / (double)(T - 1));
      o[c] = op == BLDP_OP_STD ? sqrtf(var) : var;
    }
  }
}

// var / std of blocks too few to fill the GPU: a block's spectra in nchunk
// chunks of tchunk, one workgroup (tile of channels x time slices, as above)
// each.  PHASE 0 leaves every chunk's sum(x - K) in ws, PHASE 1 adds them (in
// chunk order, the same in every workgroup) for the mean and leaves the
// chunk's squared deviations, k_tstat_mom_finish adds those.  Workgroup x is
// tile ct of chunk ch of (IF i, block b); ws is Float64
// [2][nchunk][nbank][nb][ni][nc].
template <int CPL, int PHASE>
__global__ __launch_bounds__(kBlock) void k_tstat_mom_chunk(const TStatArgs a) {
  __shared__ double sh[kBlock][CPL];
  const int lx = 1 << a.lx_log2, tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> a.lx_log2;
  const int ny = kBlock >> a.lx_log2;
  int64_t ct, r, ch, r2, i, b;
  divmod(blockIdx.x, a.ctiles, r, ct);
  divmod(r, a.nchunk, r2, ch);
  divmod(r2, a.ni, b, i);
  const int64_t cg = ct * lx + tx;
  const bool ok = cg < a.ncg;
  const int64_t T = a.T;
  const float *p = a.in[blockIdx.y] + a.in_off + (ok ? cg : 0) * CPL * a.in_cs + i * a.in_ld_i +
                   b * T * a.in_ld_t;
  const int64_t ncols = (int64_t)a.nbank * a.nb * a.ni * a.nc;  // one plane of ws
  const int64_t col = ((blockIdx.y * a.nb + b) * a.ni + i) * a.nc + (ok ? cg : 0) * CPL;
  float K[CPL];  // the block's first element
#pragma unroll
  for (int c = 0; c < CPL; ++c) K[c] = 0.0f;
  if (ok) ldcols<CPL>(p, K);
  double ref[CPL];  // what the deviations are taken from: K, then the mean
#pragma unroll
  for (int c = 0; c < CPL; ++c) ref[c] = (double)K[c];
  if (PHASE == 1 && ok) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      double s = 0.0;
      for (int g = 0; g < a.nchunk; ++g) s += a.ws[g * ncols + col + c];
      ref[c] += s / (double)T;
    }
  }
  double acc[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc[c] = 0.0;
  const int64_t t1 = (ch + 1) * a.tchunk < T ? (ch + 1) * a.tchunk : T;
  if (ok) {
#pragma unroll 4
    for (int64_t t = ch * a.tchunk + ty; t < t1; t += ny) {
      float x[CPL];
      ldcols<CPL>(p + t * a.in_ld_t, x);
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const double d = (double)x[c] - ref[c];
        acc[c] += PHASE == 0 ? d : d * d;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CPL; ++c) sh[threadIdx.x][c] = acc[c];
  __syncthreads();
  if (ok && ty == 0) {
    double *w = a.ws + (PHASE * (int64_t)a.nchunk + ch) * ncols + col;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      double s = 0.0;
      for (int y = 0; y < ny; ++y) s += sh[y * lx + tx][c];
      w[c] = s;
    }
  }
}

// one thread per output of bank blockIdx.y: the chunks' squared deviations, in order
__global__ __launch_bounds__(kBlock) void k_tstat_mom_finish(const TStatArgs a, const int op) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t per_bank = a.nb * a.ni * a.nc;
  if (e >= per_bank) return;
  const int64_t ncols = (int64_t)a.nbank * per_bank;
  const double *w = a.ws + (int64_t)a.nchunk * ncols + blockIdx.y * per_bank + e;
  double q = 0.0;
  for (int g = 0; g < a.nchunk; ++g) q += w[g * ncols];
  int64_t c, r, i, b;
  divmod(e, a.nc, r, c);
  divmod(r, a.ni, b, i);
  const float var = (float)(q / (double)(a.T - 1));  // (std: the root of the Float32 variance)
  a.out[blockIdx.y * a.out_bank + c + i * a.out_ld_i + b * a.out_ld_b] =
      op == BLDP_OP_STD ? sqrtf(var) : var;
}

// k_tstat_med_split's LDS arrays, per workgroup column (<= kMedCols)
struct MedShared {
  uint32_t (*hist)[256];
  uint32_t (*rank)[kMedCols];  // [2]: of the wanted key among the prefix's keys, by pass parity
  uint32_t *seld;              // the digit selected by the pass
  uint32_t *selc;              // how many of the prefix's keys have it
  uint32_t *mingt;             // smallest key above the selected one
  int *nanflag;
};

// The select of a workgroup's tile: four passes for pre = the key of rank q
// (the median's (T-1)/2) of every column, and where the next rank is wanted
// too (`upper`: the median of an even T, every quantile) a fifth for sh.mingt.
// DEV: the keys are those of |x - cen| (mad's second selection; sh.nanflag is
// kept).
template <int CPL, bool DEV>
__device__ __forceinline__ void med_select(const TStatArgs &a, const SplitGeo &g, const float *p,
                                           const MedShared &sh, const float (&cen)[CPL],
                                           uint32_t (&pre)[CPL], const uint32_t q,
                                           const bool upper) {
  const int tid = threadIdx.x;
  const int64_t T = a.T;
  const int lc0 = g.tx * CPL;  // this lane's first column of the workgroup's (lx * CPL <= kMedCols)
  // the value whose key is counted
  auto val = [&](float x, int c) { return DEV ? abs_dev(x, cen[c]) : x; };
  if (tid < kMedCols) {
    sh.rank[0][tid] = q;
    sh.seld[tid] = 0;
    sh.selc[tid] = 0;
    sh.mingt[tid] = kPadKey;
    if (!DEV) sh.nanflag[tid] = 0;
  }
#pragma unroll
  for (int c = 0; c < CPL; ++c) pre[c] = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t mask = ~(0xffffffffu >> (8 * pass));  // the bits fixed so far
    for (int k = tid; k < kMedCols * 256; k += kBlock) (&sh.hist[0][0])[k] = 0;
    __syncthreads();
    if (g.ok) {
      // a run of equal digits is counted once (spectra share their exponent byte)
      uint32_t rd[CPL], rn[CPL];
      bool nan[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) rd[c] = 0, rn[c] = 0, nan[c] = false;
#pragma unroll 4
      for (int64_t t = g.ty; t < T; t += g.ny) {
        float x[CPL];
        ldcols<CPL>(p + t * a.in_ld_t, x);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          x[c] = val(x[c], c);
          nan[c] = nan[c] || x[c] != x[c];
          const uint32_t key = f2key(x[c]);
          if ((key & mask) == pre[c]) {
            const uint32_t d = (key >> shift) & 255u;
            if (d == rd[c]) {
              ++rn[c];
            } else {
              if (rn[c]) atomicAdd(&sh.hist[lc0 + c][rd[c]], rn[c]);
              rd[c] = d;
              rn[c] = 1;
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        if (rn[c]) atomicAdd(&sh.hist[lc0 + c][rd[c]], rn[c]);
        if (pass == 0 && nan[c]) sh.nanflag[lc0 + c] = 1;
      }
    }
    __syncthreads();
    // the bin holding the rank: kScanLanes lanes a column sum kScanBins bins
    // each, a prefix over them, and the lane whose bins hold it walks them
    {
      const int col = tid / kScanLanes, part = tid % kScanLanes;
      const uint32_t r = sh.rank[pass & 1][col];
      uint32_t mine = 0;
      for (int j = 0; j < kScanBins; ++j) mine += sh.hist[col][part * kScanBins + j];
      uint32_t incl = mine;
#pragma unroll
      for (int w = 1; w < kScanLanes; w *= 2) {
        const uint32_t u = __shfl_up(incl, w, kScanLanes);
        if (part >= w) incl += u;
      }
      uint32_t acc = incl - mine;
      const bool here = mine && acc <= r && r < incl;
      for (int j = 0; j < kScanBins; ++j) {
        const uint32_t n = sh.hist[col][part * kScanBins + j];
        if (here && acc <= r && r < acc + n) {
          sh.seld[col] = (uint32_t)(part * kScanBins + j);
          sh.selc[col] = n;
          sh.rank[(pass + 1) & 1][col] = r - acc;
        }
        acc += n;
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CPL; ++c) pre[c] |= sh.seld[lc0 + c] << shift;
  }
  // pre = the key of rank q; selc of them are equal, and it is number
  // rank[0] among those (four passes: parity 0 again)
  if (upper) {
    if (g.ok) {
      uint32_t mn[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) mn[c] = kPadKey;
#pragma unroll 4
      for (int64_t t = g.ty; t < T; t += g.ny) {
        float x[CPL];
        ldcols<CPL>(p + t * a.in_ld_t, x);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          const uint32_t key = f2key(val(x[c], c));
          if (key > pre[c]) mn[c] = min(mn[c], key);
        }
      }
#pragma unroll
      for (int c = 0; c < CPL; ++c) atomicMin(&sh.mingt[lc0 + c], mn[c]);
    }
    __syncthreads();
  }
}

// SEL_MAD: the select runs twice, over the keys of x for the columns' medians
// cen, then over those of |x - cen|.  SEL_QUANTILE: rank a.qrank and the next.
// SEL_OUTLIERS: mad's two selections, then one more pass over the block for the
// trailing OutlArgs' outputs (OA is empty for every other selector): the time
// slices form |x - cen|, store the flags and add their counts in LDS.
template <int CPL, Sel SEL, typename... OA>
__global__ __launch_bounds__(kBlock) void k_tstat_med_split(const TStatArgs a, const OA... oas) {
  constexpr bool MAD = SEL == SEL_MAD || SEL == SEL_OUTLIERS;
  __shared__ uint32_t hist[kMedCols][256];
  __shared__ uint32_t rank[2][kMedCols];
  __shared__ uint32_t seld[kMedCols];
  __shared__ uint32_t selc[kMedCols];
  __shared__ uint32_t mingt[kMedCols];
  __shared__ int nanflag[kMedCols];
  const MedShared sh{hist, rank, seld, selc, mingt, nanflag};
  const SplitGeo g = split_geo(a);
  const int64_t T = a.T;
  const float *p = a.in[blockIdx.y] + a.in_off + (g.ok ? g.cg : 0) * CPL * a.in_cs +
                   g.i * a.in_ld_i + g.b * T * a.in_ld_t;
  const int lc0 = g.tx * CPL;
  const bool odd = (T & 1) != 0;
  const uint32_t q = SEL == SEL_QUANTILE ? (uint32_t)a.qrank : (uint32_t)((T - 1) / 2);
  const bool upper = SEL == SEL_QUANTILE || !odd;
  float cen[CPL];
  uint32_t pre[CPL];  // key bits fixed so far
#pragma unroll
  for (int c = 0; c < CPL; ++c) cen[c] = 0.0f;
  med_select<CPL, false>(a, g, p, sh, cen, pre, q, upper);
  // the key of the next rank (T/2 of an even block): pre again, or the smallest above it
  auto rank1 = [&](int c) {
    const int lc = lc0 + c;
    return sh.rank[0][lc] + 1 < sh.selc[lc] ? pre[c] : sh.mingt[lc];
  };
  bool nan0[CPL];  // SEL_OUTLIERS: the block holds a NaN
  if constexpr (MAD) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      cen[c] = median_of(pre[c], rank1(c), odd, false);  // (a NaN block: NaN below)
      nan0[c] = SEL == SEL_OUTLIERS && sh.nanflag[lc0 + c] != 0;
    }
    __syncthreads();  // (rank, selc and mingt are read: the second selection resets them)
    med_select<CPL, true>(a, g, p, sh, cen, pre, q, upper);
  }
  if constexpr (SEL == SEL_OUTLIERS) {
    __shared__ uint32_t cnt_s[kMedCols];
    const OutlArgs &oa = first_arg(oas...);
    float sc[CPL], thr[CPL];
    bool live[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool nan = sh.nanflag[lc0 + c] != 0;
      sc[c] = mad_scale(median_of(pre[c], rank1(c), odd, nan));
      thr[c] = outl_thr(oa.nsigma, sc[c]);
      live[c] = !nan && thr[c] == thr[c];  // (a NaN median or scale flags nothing)
    }
    if (threadIdx.x < kMedCols) cnt_s[threadIdx.x] = 0;
    __syncthreads();
    if (g.ok) {
      uint8_t *m = oa.mask ? oa.mask + blockIdx.y * oa.mask_bank + g.cg * CPL +
                                 g.i * oa.mask_ld_i + g.b * T * oa.mask_ld_t
                           : nullptr;
      uint32_t cnt[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) cnt[c] = 0;
#pragma unroll 4
      for (int64_t t = g.ty; t < T; t += g.ny) {
        float x[CPL];
        ldcols<CPL>(p + t * a.in_ld_t, x);
        bool f[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c)
          f[c] = live[c] && abs_dev(x[c], cen[c]) > thr[c], cnt[c] += f[c];
        if (m) {
          if constexpr (CPL == 4)
            outl_store4(m + t * oa.mask_ld_t, f[0], f[1], f[2], f[3]);
          else
            m[t * oa.mask_ld_t] = f[0];
        }
      }
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (cnt[c]) atomicAdd(&cnt_s[lc0 + c], cnt[c]);
    }
    __syncthreads();
    if (g.ok && g.ty == 0) {
      const int64_t eo =
          blockIdx.y * a.out_bank + g.cg * CPL + g.i * a.out_ld_i + g.b * a.out_ld_b;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        if (oa.med) oa.med[eo + c] = nan0[c] ? __uint_as_float(0x7fc00000u) : cen[c];
        if (oa.mad) oa.mad[eo + c] = sc[c];
        if (oa.count) oa.count[eo + c] = cnt_s[lc0 + c];
      }
    }
  } else if (g.ok && g.ty == 0) {
    float *o = a.out + blockIdx.y * a.out_bank + g.cg * CPL + g.i * a.out_ld_i + g.b * a.out_ld_b;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      if constexpr (SEL == SEL_QUANTILE) {
        o[c] = quantile_of(pre[c], rank1(c), a.qg, sh.nanflag[lc0 + c] != 0);
      } else {
        const float m = median_of(pre[c], rank1(c), odd, sh.nanflag[lc0 + c] != 0);
        o[c] = MAD ? mad_scale(m) : m;
      }
    }
  }
}

// quantiles(ps), T > 32 (the file's head): the qs.nlow distinct lower ranks
// qs.low[] of every column of a tile of COLS = 32 (G = 1) or 16 columns, G
// ranks a sweep.  Per (lower rank l, column) in LDS: pre, the key bits fixed so
// far; rem, the rank among that prefix's keys (two copies by pass parity: a
// pass reads one and writes the other; four passes end in copy 0); selc, how
// many keys equal the selected one; mingt, the smallest key above it.
template <int CPL, int G>
__global__ __launch_bounds__(kBlock) void k_tquantiles_split(const TStatArgs a, const QSet qs) {
  constexpr int COLS = G == 1 ? kMedCols : kMedCols / 2;
  constexpr int SCANL = kBlock / COLS;  // lanes scanning one column's histogram
  constexpr int SCANB = 256 / SCANL;    // bins each of them sums
  constexpr int NQ = BLDP_MAX_QUANTILES;
  __shared__ uint32_t hist[G][COLS][256];
  __shared__ uint32_t pre_s[NQ][COLS];
  __shared__ uint32_t rem_s[2][NQ][COLS];
  __shared__ uint32_t selc_s[NQ][COLS];
  __shared__ uint32_t mingt_s[NQ][COLS];
  __shared__ int nanflag[COLS];
  const int tid = threadIdx.x;
  const SplitGeo g = split_geo(a);  // (lx * CPL <= COLS: plan_tstat_q)
  const int64_t T = a.T;
  const float *p = a.in[blockIdx.y] + a.in_off + (g.ok ? g.cg : 0) * CPL * a.in_cs +
                   g.i * a.in_ld_i + g.b * T * a.in_ld_t;
  const int lc0 = g.tx * CPL;  // this lane's first column of the workgroup's
  const int nlow = qs.nlow;
  for (int k = tid; k < NQ * COLS; k += kBlock) {
    const int l = k / COLS;
    (&pre_s[0][0])[k] = 0;
    (&rem_s[0][0][0])[k] = l < nlow ? (uint32_t)qs.low[l] : 0u;
    (&selc_s[0][0])[k] = 0;
    (&mingt_s[0][0])[k] = kPadKey;
  }
  if (tid < COLS) nanflag[tid] = 0;
  // Counts the digits (key >> shift) & 255 of the keys whose bits under mask
  // are pr[j][c] into hist[j] (j < ng), for this lane's columns over its time
  // slice.  A run of equal digits is counted once (spectra share their
  // exponent byte).  Pass 0: mask = 0 and ng = 1, every key counts, and NaNs
  // are noted.
  auto count = [&](const int ng, const int shift, const uint32_t mask,
                   const uint32_t (&pr)[G][CPL], const bool first) {
    for (int k = tid; k < ng * COLS * 256; k += kBlock) (&hist[0][0][0])[k] = 0;
    __syncthreads();
    if (g.ok) {
      uint32_t rd[G][CPL], rn[G][CPL];
      bool nan[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        nan[c] = false;
#pragma unroll
        for (int j = 0; j < G; ++j) rd[j][c] = 0, rn[j][c] = 0;
      }
#pragma unroll 4
      for (int64_t t = g.ty; t < T; t += g.ny) {
        float x[CPL];
        ldcols<CPL>(p + t * a.in_ld_t, x);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          nan[c] = nan[c] || x[c] != x[c];
          const uint32_t key = f2key(x[c]);
          const uint32_t d = (key >> shift) & 255u;
#pragma unroll
          for (int j = 0; j < G; ++j) {
            if (j < ng && (key & mask) == pr[j][c]) {
              if (d == rd[j][c]) {
                ++rn[j][c];
              } else {
                if (rn[j][c]) atomicAdd(&hist[j][lc0 + c][rd[j][c]], rn[j][c]);
                rd[j][c] = d;
                rn[j][c] = 1;
              }
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
#pragma unroll
        for (int j = 0; j < G; ++j)
          if (rn[j][c]) atomicAdd(&hist[j][lc0 + c][rd[j][c]], rn[j][c]);
        if (first && nan[c]) nanflag[lc0 + c] = 1;
      }
    }
    __syncthreads();
  };
  // The bin of hist[j] holding lower rank l of every column: SCANL lanes a
  // column sum SCANB bins each, a prefix over them, and the lane whose bins
  // hold the rank walks them.
  auto settle = [&](const int j, const int l, const int shift, const int par) {
    const int col = tid / SCANL, part = tid % SCANL;
    const uint32_t r = rem_s[par][l][col];
    uint32_t mine = 0;
    for (int b = 0; b < SCANB; ++b) mine += hist[j][col][part * SCANB + b];
    uint32_t incl = mine;
#pragma unroll
    for (int w = 1; w < SCANL; w *= 2) {
      const uint32_t u = __shfl_up(incl, w, SCANL);
      if (part >= w) incl += u;
    }
    uint32_t acc = incl - mine;
    const bool here = mine && acc <= r && r < incl;
    for (int b = 0; b < SCANB; ++b) {
      const uint32_t n = hist[j][col][part * SCANB + b];
      if (here && acc <= r && r < acc + n) {
        pre_s[l][col] |= (uint32_t)(part * SCANB + b) << shift;
        selc_s[l][col] = n;
        rem_s[par ^ 1][l][col] = r - acc;
      }
      acc += n;
    }
  };
  uint32_t pr[G][CPL];
#pragma unroll
  for (int j = 0; j < G; ++j)
#pragma unroll
    for (int c = 0; c < CPL; ++c) pr[j][c] = 0;
  // pass 0: one histogram a column, every lower rank reads it
  count(1, 24, 0u, pr, true);  // (its first barrier covers the setup above)
  for (int l = 0; l < nlow; ++l) settle(0, l, 24, 0);
  __syncthreads();
  for (int l0 = 0; l0 < nlow; l0 += G) {
    const int ng = nlow - l0 < G ? nlow - l0 : G;  // ranks of this sweep (uniform)
    for (int pass = 1; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
#pragma unroll
      for (int j = 0; j < G; ++j)
#pragma unroll
        for (int c = 0; c < CPL; ++c) pr[j][c] = j < ng ? pre_s[l0 + j][lc0 + c] : 0u;
      count(ng, shift, ~(0xffffffffu >> (8 * pass)), pr, false);
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (j < ng) settle(j, l0 + j, shift, pass & 1);
      __syncthreads();
    }
    // pre_s = the keys of the sweep's ranks; the smallest key above each
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int c = 0; c < CPL; ++c) pr[j][c] = j < ng ? pre_s[l0 + j][lc0 + c] : kPadKey;
    if (g.ok) {
      uint32_t mn[G][CPL];
#pragma unroll
      for (int j = 0; j < G; ++j)
#pragma unroll
        for (int c = 0; c < CPL; ++c) mn[j][c] = kPadKey;
#pragma unroll 4
      for (int64_t t = g.ty; t < T; t += g.ny) {
        float x[CPL];
        ldcols<CPL>(p + t * a.in_ld_t, x);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          const uint32_t key = f2key(x[c]);
#pragma unroll
          for (int j = 0; j < G; ++j)
            if (key > pr[j][c]) mn[j][c] = min(mn[j][c], key);
        }
      }
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (j < ng) {
#pragma unroll
          for (int c = 0; c < CPL; ++c) atomicMin(&mingt_s[l0 + j][lc0 + c], mn[j][c]);
        }
    }
    __syncthreads();
  }
  if (g.ok && g.ty == 0) {
    float *o = a.out + blockIdx.y * a.out_bank + g.cg * CPL + g.i * a.out_ld_i + g.b * a.out_ld_b;
    for (int kq = 0; kq < qs.np; ++kq) {
      const int l = qs.lsel[kq];
      const double w = qs.g[kq];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int lc = lc0 + c;
        // the key of the next rank: the same again, or the smallest above it
        const uint32_t ka = pre_s[l][lc];
        const uint32_t kb = rem_s[0][l][lc] + 1 < selc_s[l][lc] ? ka : mingt_s[l][lc];
        o[kq * qs.out_ld_q + c] = quantile_of(ka, kb, w, nanflag[lc] != 0);
      }
    }
  }
}

int pow2_ceil_log2(int64_t n, int cap) {
  int l = 0;
  while (l < cap && ((int64_t)1 << l) < n) ++l;
  return l;
}

}  // namespace

int plan_tstat(TStatArgs &a, int op, bool words, int num_cus, int xcd_lg, TStatPlan *pp) {
  TStatPlan p{};
  const int64_t T = a.T;
  // (mad: the median's path, its selection run twice; quantile: its ranks moved)
  const bool med = median_op(op);
  const int rounds = op == BLDP_OP_MAD ? 2 : 1;
  a.vec = (words && a.in_cs == 1 && a.nc % 4 == 0) ? 1 : 0;  // float4 columns
  const int cpl = a.vec ? 4 : 1;
  a.ncg = a.nc / cpl;
  a.lx_log2 = 0;
  a.ctiles = 1;
  a.xcd_lg = 0;
  a.nchunk = 1;
  a.tchunk = T;
  p.cpl = cpl;
  p.ws_bytes = 0;
  if (med && T >= ((int64_t)1 << 31))
    return set_error(BLDP_EINVAL, "median: tavby=%lld is beyond 2^31 - 1", (long long)T);
  int64_t grid;
  if (T <= kRegMaxT) {
    p.path = med ? TSTAT_REGS_MEDIAN : TSTAT_REGS_MOMENTS;
    p.tsplit = 1;
    p.passes = rounds;
    const int64_t items = a.ncg * a.ni * a.nb;
    grid = (items + kBlock - 1) / kBlock;
    // the per-XCD tile order where neighbouring workgroups read neighbouring
    // memory, as plan_stats
    a.xcd_lg = xcd_lg;
  } else {
    // lanes along the channels: as many as there are column groups, the
    // median's at most kMedCols columns; the moments' tile is narrowed (down
    // to 64-byte row segments) until the workgroups fill the GPU
    int lg = pow2_ceil_log2(a.ncg, 6);
    if (med) {
      lg = std::min(lg, cpl == 4 ? 3 : 5);
    } else {
      const int lg_min = std::min(lg, cpl == 4 ? 2 : 4);
      auto groups = [&](int l) {
        return ((a.ncg + ((int64_t)1 << l) - 1) >> l) * a.ni * a.nb * a.nbank;
      };
      // too few even then: the blocks are cut into time chunks, one
      // workgroup each (4 a CU), the tile as wide as the channels allow
      const int64_t want = 4 * (int64_t)num_cus;
      const int64_t g0 = std::max<int64_t>(groups(lg), 1);
      const int64_t nch = std::min<int64_t>((want + g0 - 1) / g0, T / kChunkMin);
      if (groups(lg_min) < 2 * (int64_t)num_cus && nch >= 2) {
        a.tchunk = (T + nch - 1) / nch;
        a.nchunk = (int32_t)((T + a.tchunk - 1) / a.tchunk);
      } else {
        while (lg > lg_min && groups(lg) < 2 * (int64_t)num_cus) --lg;
      }
    }
    a.lx_log2 = lg;
    a.ctiles = (a.ncg + ((int64_t)1 << lg) - 1) >> lg;
    p.path = med ? TSTAT_SPLIT_MEDIAN : a.nchunk > 1 ? TSTAT_CHUNK_MOMENTS : TSTAT_SPLIT_MOMENTS;
    p.tsplit = kBlock >> lg;
    // (a quantile always takes the next rank too: the fifth pass)
    p.passes = med ? rounds * (T % 2 && op != kOpQuantile ? 4 : 5) : 2;
    grid = a.ctiles * a.nchunk * a.ni * a.nb;
    if (a.nchunk > 1)
      p.ws_bytes = (size_t)2 * a.nchunk * a.nbank * a.nb * a.ni * a.nc * sizeof(double);
  }
  if (grid > INT32_MAX)
    return set_error(BLDP_EINVAL,
                     "tavfunc median/var/std/mad/quantile: %lld blocks of %lld spectra are too many for one "
                     "launch",
                     (long long)a.nb, (long long)T);
  p.grid = grid;
  *pp = p;
  return BLDP_OK;
}

// k_tquantiles_split: lower ranks per sweep, and the columns of a workgroup
static int sweep_ranks(int nlow) { return std::min(std::max(nlow, 1), 3); }
static int sweep_cols(int nlow) { return nlow <= 1 ? kMedCols : kMedCols / 2; }

int plan_tstat_q(TStatArgs &a, int nlow, bool words, int num_cus, int xcd_lg, TStatPlan *pp) {
  const int rc = plan_tstat(a, kOpQuantiles, words, num_cus, xcd_lg, pp);
  if (rc) return rc;
  if (pp->path != TSTAT_SPLIT_MEDIAN) {
    pp->passes = 1;
    return BLDP_OK;
  }
  // the median's tile, narrowed to the columns whose histograms fit
  const int cols = sweep_cols(nlow), G = sweep_ranks(nlow);
  int lg = a.lx_log2;
  while (lg > 0 && (pp->cpl << lg) > cols) --lg;
  a.lx_log2 = lg;
  a.ctiles = (a.ncg + ((int64_t)1 << lg) - 1) >> lg;
  pp->tsplit = kBlock >> lg;
  pp->passes = 1 + 4 * ((std::max(nlow, 1) + G - 1) / G);
  pp->grid = a.ctiles * a.ni * a.nb;
  if (pp->grid > INT32_MAX)
    return set_error(BLDP_EINVAL,
                     "tavfunc quantiles: %lld blocks of %lld spectra are too many for one launch",
                     (long long)a.nb, (long long)a.T);
  return BLDP_OK;
}

namespace {

template <int TP>
hipError_t launch_regs_q(const TStatArgs &a, const QSet &qs, dim3 grid, hipStream_t s) {
  return launch_kernel(a.vec ? k_tstat_regs<TP, 4, 4, QSet> : k_tstat_regs<TP, 1, 4, QSet>, grid,
                       dim3(kBlock), 0, s, a, 0, qs);
}

template <int TP, int CPL>
hipError_t launch_regs_cpl(const TStatArgs &a, bool med, dim3 grid, int op, hipStream_t s) {
  if (!med) return launch_kernel(k_tstat_regs<TP, CPL, 0>, grid, dim3(kBlock), 0, s, a, op);
  return launch_kernel(op == BLDP_OP_MAD ? k_tstat_regs<TP, CPL, 2>
                                         : op == kOpQuantile ? k_tstat_regs<TP, CPL, 3>
                                                             : k_tstat_regs<TP, CPL, 1>,
                       grid, dim3(kBlock), 0, s, a, op);
}
template <int TP>
hipError_t launch_regs(const TStatArgs &a, bool med, dim3 grid, int op, hipStream_t s) {
  return a.vec ? launch_regs_cpl<TP, 4>(a, med, grid, op, s)
               : launch_regs_cpl<TP, 1>(a, med, grid, op, s);
}
}  // namespace

hipError_t launch_tstat(const TStatArgs &a, const TStatPlan &p, int op, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  if (op == kOpQuantile && (a.qrank < 0 || (int64_t)a.qrank + 1 >= a.T))
    return hipErrorInvalidValue;  // (the upper rank must be a key of the block)
  const dim3 grid((unsigned)p.grid, (unsigned)a.nbank);
  const auto go = [&](auto *kn, auto... args) {
    return launch_kernel(kn, grid, dim3(kBlock), 0, s, args...);
  };
  switch (p.path) {
    case TSTAT_REGS_MOMENTS:
    case TSTAT_REGS_MEDIAN: {
      const bool med = p.path == TSTAT_REGS_MEDIAN;
      if (a.T <= 2) return launch_regs<2>(a, med, grid, op, s);
      if (a.T <= 4) return launch_regs<4>(a, med, grid, op, s);
      if (a.T <= 8) return launch_regs<8>(a, med, grid, op, s);
      if (a.T <= 16) return launch_regs<16>(a, med, grid, op, s);
      if (a.T <= 32) return launch_regs<32>(a, med, grid, op, s);
      break;
    }
    case TSTAT_SPLIT_MOMENTS:
      return go(a.vec ? k_tstat_mom_split<4> : k_tstat_mom_split<1>, a, op);
    case TSTAT_SPLIT_MEDIAN:
      if (op == BLDP_OP_MAD)
        return go(a.vec ? k_tstat_med_split<4, SEL_MAD> : k_tstat_med_split<1, SEL_MAD>, a);
      if (op == kOpQuantile)
        return go(a.vec ? k_tstat_med_split<4, SEL_QUANTILE> : k_tstat_med_split<1, SEL_QUANTILE>,
                  a);
      return go(a.vec ? k_tstat_med_split<4, SEL_MEDIAN> : k_tstat_med_split<1, SEL_MEDIAN>, a);
    case TSTAT_CHUNK_MOMENTS: {
      if (!a.ws) return hipErrorInvalidValue;
      const hipStream_t st = s;
      void (*sums)(TStatArgs) = a.vec ? k_tstat_mom_chunk<4, 0> : k_tstat_mom_chunk<1, 0>;
      void (*devs)(TStatArgs) = a.vec ? k_tstat_mom_chunk<4, 1> : k_tstat_mom_chunk<1, 1>;
      hipLaunchKernelGGL(sums, grid, dim3(kBlock), 0, st, a);
      hipLaunchKernelGGL(devs, grid, dim3(kBlock), 0, st, a);
      const int64_t per_bank = a.nb * a.ni * a.nc;
      hipLaunchKernelGGL(k_tstat_mom_finish, dim3((unsigned)((per_bank + kBlock - 1) / kBlock),
                                                  (unsigned)a.nbank),
                         dim3(kBlock), 0, st, a, op);
      return hipGetLastError();
    }
  }
  return hipErrorInvalidValue;
}

// mad's reads and the flag pass; the register form reads once, and once more
// for the positions of a mask
int tstat_outl_reads(const TStatPlan &p, bool mask) {
  return p.path == TSTAT_SPLIT_MEDIAN ? p.passes + 1 : mask ? 2 : 1;
}

namespace {
template <int TP>
hipError_t launch_regs_outl(const TStatArgs &a, const OutlArgs &oa, dim3 grid, hipStream_t s) {
  return launch_kernel(a.vec ? k_tstat_regs<TP, 4, 5, OutlArgs> : k_tstat_regs<TP, 1, 5, OutlArgs>,
                       grid, dim3(kBlock), 0, s, a, 0, oa);
}
}  // namespace

hipError_t launch_tstat_outl(const TStatArgs &a, const TStatPlan &p, const OutlArgs &oa,
                             hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  if (a.T < 2 || a.out || !(oa.nsigma >= 0.0 && oa.nsigma <= 1.7976931348623157e308))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)p.grid, (unsigned)a.nbank);
  if (p.path == TSTAT_REGS_MEDIAN) {
    if (a.T <= 2) return launch_regs_outl<2>(a, oa, grid, s);
    if (a.T <= 4) return launch_regs_outl<4>(a, oa, grid, s);
    if (a.T <= 8) return launch_regs_outl<8>(a, oa, grid, s);
    if (a.T <= 16) return launch_regs_outl<16>(a, oa, grid, s);
    if (a.T <= 32) return launch_regs_outl<32>(a, oa, grid, s);
    return hipErrorInvalidValue;
  }
  if (p.path != TSTAT_SPLIT_MEDIAN) return hipErrorInvalidValue;
  return launch_kernel(a.vec ? k_tstat_med_split<4, SEL_OUTLIERS, OutlArgs>
                             : k_tstat_med_split<1, SEL_OUTLIERS, OutlArgs>,
                       grid, dim3(kBlock), 0, s, a, oa);
}

hipError_t launch_tstat_q(const TStatArgs &a, const TStatPlan &p, const QSet &qs, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  // (every rank must be a key of the block; the kernels index by these counts)
  if (a.T < 2 || qs.np < 1 || qs.np > BLDP_MAX_QUANTILES || qs.nr < 1 ||
      qs.nr > 2 * BLDP_MAX_QUANTILES || qs.nlow < 1 || qs.nlow > BLDP_MAX_QUANTILES)
    return hipErrorInvalidValue;
  for (int r = 0; r < qs.nr; ++r)
    if (qs.rank[r] < 0 || qs.rank[r] >= a.T) return hipErrorInvalidValue;
  for (int l = 0; l < qs.nlow; ++l)
    if (qs.low[l] < 0 || (int64_t)qs.low[l] + 1 >= a.T) return hipErrorInvalidValue;
  for (int k = 0; k < qs.np; ++k)
    if (qs.lo[k] >= qs.nr || qs.hi[k] >= qs.nr || qs.lsel[k] >= qs.nlow)
      return hipErrorInvalidValue;
  const dim3 grid((unsigned)p.grid, (unsigned)a.nbank);
  if (p.path == TSTAT_REGS_MEDIAN) {
    if (a.T <= 2) return launch_regs_q<2>(a, qs, grid, s);
    if (a.T <= 4) return launch_regs_q<4>(a, qs, grid, s);
    if (a.T <= 8) return launch_regs_q<8>(a, qs, grid, s);
    if (a.T <= 16) return launch_regs_q<16>(a, qs, grid, s);
    if (a.T <= 32) return launch_regs_q<32>(a, qs, grid, s);
    return hipErrorInvalidValue;
  }
  if (p.path != TSTAT_SPLIT_MEDIAN) return hipErrorInvalidValue;
  // (the tile's columns have a histogram each: plan_tstat_q)
  if (((a.vec ? 4 : 1) << a.lx_log2) > sweep_cols(qs.nlow)) return hipErrorInvalidValue;
  const auto go = [&](auto *kn) { return launch_kernel(kn, grid, dim3(kBlock), 0, s, a, qs); };
  switch (sweep_ranks(qs.nlow)) {
    case 1: return go(a.vec ? k_tquantiles_split<4, 1> : k_tquantiles_split<1, 1>);
    case 2: return go(a.vec ? k_tquantiles_split<4, 2> : k_tquantiles_split<1, 2>);
    case 3: return go(a.vec ? k_tquantiles_split<4, 3> : k_tquantiles_split<1, 3>);
  }
  return hipErrorInvalidValue;
}

}  // namespace bldp
