// fold.hip — fold a Float32 window over its coarse channels, and unfold it (gfx950).
//
// Selected channel c of the (nc, ni, nt) window has fine index k = c mod nfpc and
// coarse index j = c div nfpc; T selected spectra make a time block.  The fold of
// output (k, i, t') runs over the J*T samples A[k + nfpc*j, i, t'*T + tt] of every
// bank: kept, the count of the samples whose mask byte is 0, and the Float64 sum
// of those samples rounded once to Float32 (the mean: divided once in Float64 by
// Float64(kept) first).  A flagged sample is excluded by a select before the add.
// The unfold divides the window by such a profile, or subtracts it.
//
// An item is the float4 (VEC) or the one value a lane loads; a coarse channel
// holds P = nfpc / (4 or 1) items.  A unit is one spectrum of G coarse channels of
// one bank; a block's nbank * ceil(J/G) * T units are cut into nchunk chunks of CU
// units, a workgroup each.
//   k_fold<ROWS=false>  P > 128: lanes along k, 256 items a workgroup, G = 1; a lane
//                       walks its chunk's (bank, j, tt) with its sums in registers.
//   k_fold<ROWS=true>   P <= 128: the lanes lie along c over G = min(256 div P, J)
//                       coarse channels of a row (a workgroup of the whole waves
//                       that G * P lanes need); lanes with equal c mod nfpc meet
//                       through LDS in a fixed order at the end.
//   k_fold_merge        nchunk > 1: the chunks' Float64 sums and counts, which the
//                       fold left in the workspace [nchunk][nto][ni][nfpc], added in
//                       an order the plan fixes.  No atomics: two calls give
//                       identical bits.
// The mask stream has masked.hip's three forms (MF 0 a byte per element, 1 one
// aligned dword per float4, 2 one byte per row) and MF 3: no mask.
//   k_unfold            one streaming pass, float4 or one dword per element.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bldp_impl.h"

namespace bldp {
namespace {

constexpr int kBlock = 256;  // 4 waves of 64
constexpr int kRun = 8;      // spectra a lane loads before it adds them

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

template <bool VEC, int MF>
__device__ __forceinline__ void fold_load(const float *p, const uint8_t *m, int64_t cs,
                                          int64_t mcs, float *x, uint32_t &f) {
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    if (MF == 0)
      f = (uint32_t)m[0] | ((uint32_t)m[mcs] << 8) | ((uint32_t)m[2 * mcs] << 16) |
          ((uint32_t)m[3 * mcs] << 24);
    else if (MF == 1)
      f = *reinterpret_cast<const uint32_t *>(m);
  } else {
    x[0] = p[0];
    if (MF == 0) f = m[0];
  }
  if (MF == 2) f = m[0];
  if (MF == 3) f = 0u;
  (void)cs;
}

template <bool VEC, int MF>
__device__ __forceinline__ void fold_take(double *s, uint32_t *n, const float *x, uint32_t f) {
  constexpr int EP = VEC ? 4 : 1;
#pragma unroll
  for (int c = 0; c < EP; ++c) {
    const bool flagged = MF == 3 ? false : (VEC && MF != 2) ? ((f >> (8 * c)) & 0xffu) != 0u : f != 0u;
    s[c] += flagged ? 0.0 : (double)x[c];
    n[c] += flagged ? 0u : 1u;
  }
}

// the value of an output: the sum, or the mean, rounded once to Float32
__device__ __forceinline__ float fold_value(const FoldArgs &a, double s, uint32_t n) {
  return (float)(a.mean ? s / (double)n : s);
}

template <bool ROWS, bool VEC, int MF>
__global__ __launch_bounds__(kBlock) void k_fold(const FoldArgs a) {
  constexpr int EP = VEC ? 4 : 1;
  __shared__ double shs[ROWS ? kBlock * EP : 1];
  __shared__ uint32_t shk[ROWS ? kBlock * EP : 1];
  const uint32_t tid = threadIdx.x;
  // workgroup -> (tile along k, chunk, IF, time block)
  int64_t r = blockIdx.x;
  const int64_t xw = r % a.xwg;
  r /= a.xwg;
  const int64_t q = r % a.nchunk;
  r /= a.nchunk;
  const int64_t i = r % a.ni, tb = r / a.ni;
  const uint32_t P = (uint32_t)a.P;
  int64_t item, jsub;
  bool active;
  if (ROWS) {
    item = tid % P, jsub = tid / P;
    active = jsub < a.G;
  } else {
    item = xw * kBlock + tid, jsub = 0;
    active = item < a.P;
  }
  double s[EP];
  uint32_t n[EP];
#pragma unroll
  for (int c = 0; c < EP; ++c) s[c] = 0.0, n[c] = 0u;
  // the chunk's units [u, u1); unit u is spectrum tt of coarse group jg of bank b
  int64_t u = q * a.CU;
  const int64_t u1 = u + a.CU < a.U ? u + a.CU : a.U;
  int64_t tt = u % a.T;
  r = u / a.T;
  int64_t jg = r % a.JG, b = r / a.JG;
  while (u < u1) {
    const int64_t run = a.T - tt < u1 - u ? a.T - tt : u1 - u;
    const int64_t j = jg * a.G + jsub;
    if (active && j < a.J) {
      const int64_t c = j * a.nfpc + item * EP, t = tb * a.T + tt;
      const float *p = a.in[b] + a.in_off + c * a.in_cs + i * a.in_ld_i + t * a.in_ld_t;
      const uint8_t *m =
          MF == 3 ? nullptr : a.mask + b * a.m_bank + c * a.m_cs + i * a.m_ld_i + t * a.m_ld_t;
      int64_t k = 0;
      for (; k + kRun <= run; k += kRun) {
        float x[kRun][EP];
        uint32_t f[kRun];
#pragma unroll
        for (int h = 0; h < kRun; ++h)
          fold_load<VEC, MF>(p + h * a.in_ld_t, m + h * a.m_ld_t, a.in_cs, a.m_cs, x[h], f[h]);
#pragma unroll
        for (int h = 0; h < kRun; ++h) fold_take<VEC, MF>(s, n, x[h], f[h]);
        p += kRun * a.in_ld_t;
        m += kRun * a.m_ld_t;
      }
      for (; k < run; ++k) {
        float x[EP];
        uint32_t f;
        fold_load<VEC, MF>(p, m, a.in_cs, a.m_cs, x, f);
        fold_take<VEC, MF>(s, n, x, f);
        p += a.in_ld_t;
        m += a.m_ld_t;
      }
    }
    u += run;
    tt = 0;
    if (++jg == a.JG) jg = 0, ++b;
  }
  if (ROWS) {  // lanes with equal c mod nfpc meet, in the order of their coarse channels
#pragma unroll
    for (int c = 0; c < EP; ++c) shs[tid * EP + c] = s[c], shk[tid * EP + c] = n[c];
    __syncthreads();
    active = tid < P;
    if (active)
      for (int64_t g = 1; g < a.G; ++g)
#pragma unroll
        for (int c = 0; c < EP; ++c) {
          s[c] += shs[(tid + g * P) * EP + c];
          n[c] += shk[(tid + g * P) * EP + c];
        }
  }
  if (!active) return;
#pragma unroll
  for (int c = 0; c < EP; ++c) {
    const int64_t k = item * EP + c;
    if (a.nchunk > 1) {
      const int64_t e = q * a.nout + k + a.nfpc * (i + a.ni * tb);
      a.ws_sum[e] = s[c];
      a.ws_kept[e] = n[c];
    } else {
      const int64_t o = k + i * a.out_ld_i + tb * a.out_ld_t;
      if (a.out) a.out[o] = fold_value(a, s[c], n[c]);
      if (a.kept) a.kept[o] = n[c];
    }
  }
}

// The chunks' partials of a.mew outputs per workgroup: the kBlock / a.mew slices of
// a workgroup take every (kBlock / a.mew)-th chunk each, then meet through LDS in
// slice order.  The order depends on the plan alone.
__global__ __launch_bounds__(kBlock) void k_fold_merge(const FoldArgs a) {
  __shared__ double shs[kBlock];
  __shared__ uint32_t shk[kBlock];
  const int EW = a.mew, QS = kBlock / EW;
  const int ex = threadIdx.x % EW, qs = threadIdx.x / EW;
  const int64_t e = (int64_t)blockIdx.x * EW + ex;
  double s = 0.0;
  uint32_t n = 0u;
  if (e < a.nout) {
#pragma unroll 4
    for (int64_t q = qs; q < a.nchunk; q += QS) {
      s += a.ws_sum[q * a.nout + e];
      n += a.ws_kept[q * a.nout + e];
    }
  }
  shs[threadIdx.x] = s, shk[threadIdx.x] = n;
  __syncthreads();
  if (qs != 0 || e >= a.nout) return;
  for (int g = 1; g < QS; ++g) s += shs[ex + g * EW], n += shk[ex + g * EW];
  int64_t k, r, i, tb;
  divmod(e, a.nfpc, r, k);
  divmod(r, a.ni, tb, i);
  const int64_t o = k + i * a.out_ld_i + tb * a.out_ld_t;
  if (a.out) a.out[o] = fold_value(a, s, n);
  if (a.kept) a.kept[o] = n;
}

// one rounded operation per element (never fused, never a reciprocal)
__device__ __forceinline__ float unfold_op(int sub, float x, float p) {
  return sub ? __fsub_rn(x, p) : __fdiv_rn(x, p);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_unfold(const UnfoldArgs a) {
  constexpr int EP = VEC ? 4 : 1;
  const int64_t b = blockIdx.y;
  const float *in = a.in[b] + a.in_off;
  float *out = a.out + b * a.nc;
  const int64_t items = a.nc / EP, total = items * a.ni * a.nt;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    int64_t item, r, i, t, k, j, tb, tt;
    divmod(e, items, r, item);
    divmod(r, a.ni, t, i);
    const int64_t c = item * EP;
    divmod(c, a.nfpc, j, k);
    divmod(t, a.T, tb, tt);
    const float *p = in + c * a.in_cs + i * a.in_ld_i + t * a.in_ld_t;
    const float *pr = a.prof + k + i * a.prof_ld_i + tb * a.prof_ld_t;
    float *o = out + c + i * a.out_ld_i + t * a.out_ld_t;
    if (VEC) {
      const float4 x = *reinterpret_cast<const float4 *>(p);
      const float4 d = *reinterpret_cast<const float4 *>(pr);
      float4 y;
      y.x = unfold_op(a.sub, x.x, d.x), y.y = unfold_op(a.sub, x.y, d.y);
      y.z = unfold_op(a.sub, x.z, d.z), y.w = unfold_op(a.sub, x.w, d.w);
      *reinterpret_cast<float4 *>(o) = y;
    } else {
      o[0] = unfold_op(a.sub, p[0], pr[0]);
    }
  }
}

template <bool ROWS>
void (*fold_kernel(bool vec, int mf))(const FoldArgs) {
  switch ((vec ? 4 : 0) | mf) {
    case 0: return k_fold<ROWS, false, 0>;
    case 2: return k_fold<ROWS, false, 2>;
    case 3: return k_fold<ROWS, false, 3>;
    case 4: return k_fold<ROWS, true, 0>;
    case 5: return k_fold<ROWS, true, 1>;
    case 6: return k_fold<ROWS, true, 2>;
    case 7: return k_fold<ROWS, true, 3>;
  }
  return nullptr;  // (dword flags go with float4 data only)
}

}  // namespace

int plan_fold(FoldArgs &a, bool vec, bool mask_words, int num_cus, Plan *p) {
  a.vec = vec && a.nfpc % 4 == 0;
  const int64_t EP = a.vec ? 4 : 1;
  a.P = a.nfpc / EP;
  a.rows = a.P <= kBlock / 2;
  a.G = a.rows ? kBlock / a.P : 1;
  if (a.G > a.J) a.G = a.J > 0 ? a.J : 1;
  a.xwg = a.rows ? 1 : (a.P + kBlock - 1) / kBlock;
  a.JG = (a.J + a.G - 1) / a.G;
  a.U = a.nbank * a.JG * a.T;
  a.nout = a.nfpc * a.ni * a.nto;
  // chunks: where the blocks alone do not fill the machine, a block's units are
  // shared out until about 8 workgroups a CU exist, 32 units a chunk at the least
  // (rows: a workgroup is the whole waves its G * P lanes need)
  const int64_t block = a.rows ? (a.G * a.P + 63) / 64 * 64 : kBlock;
  const int64_t base = a.xwg * a.ni * a.nto, fill = kBlock / block;
  int64_t nchunk = 1;
  if (base > 0 && base < 2 * fill * (int64_t)num_cus) {
    nchunk = (8 * fill * (int64_t)num_cus + base - 1) / base;
    const int64_t most = (a.U + 31) / 32;
    if (nchunk > most) nchunk = most;
    if (nchunk < 1) nchunk = 1;
  }
  a.CU = a.U > 0 ? (a.U + nchunk - 1) / nchunk : 1;
  nchunk = a.U > 0 ? (a.U + a.CU - 1) / a.CU : 1;  // (no empty chunk)
  a.nchunk = (int32_t)nchunk;
  // the merge: 64 outputs a workgroup, fewer while that leaves under 256 workgroups
  a.mew = 64;
  while (a.mew > 1 && a.nout / a.mew < 256) a.mew /= 2;
  if (!a.mask_present)
    a.mform = FOLD_MASK_NONE;
  else if (a.m_cs == 0)
    a.mform = MASK_ROW;
  else if (a.vec && a.m_cs == 1 && mask_words && (a.ni <= 1 || a.m_ld_i % 4 == 0) &&
           (a.nto * a.T <= 1 || a.m_ld_t % 4 == 0) && (a.nbank <= 1 || a.m_bank % 4 == 0))
    a.mform = MASK_DWORD;
  else
    a.mform = MASK_BYTE;
  const int64_t grid = base * nchunk;
  if (grid > INT32_MAX)
    return set_error(BLDP_EINVAL, "fold: %lld workgroups are too many for one launch",
                     (long long)grid);
  p->path = a.rows ? FOLD_ROWS : FOLD_COLS;
  p->lpg = a.rows ? (int)(a.G * a.P) : kBlock;
  p->grid = grid;
  p->block = (uint32_t)block;
  p->nout = a.nout;
  p->ws_bytes = nchunk > 1 ? (size_t)nchunk * (size_t)a.nout * (sizeof(double) + sizeof(uint32_t)) : 0;
  return BLDP_OK;
}

hipError_t launch_fold(const FoldArgs &a, const Plan &p, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  if (a.mform < MASK_BYTE || a.mform > FOLD_MASK_NONE || (a.mform == MASK_DWORD && !a.vec))
    return hipErrorInvalidValue;
  if (a.nchunk > 1 && (!a.ws_sum || !a.ws_kept)) return hipErrorInvalidValue;
  void (*kn)(const FoldArgs) =
      a.rows ? fold_kernel<true>(a.vec != 0, a.mform) : fold_kernel<false>(a.vec != 0, a.mform);
  if (!kn) return hipErrorInvalidValue;
  if (p.block < 64 || p.block > kBlock || p.block % 64) return hipErrorInvalidValue;
  hipError_t e = launch_kernel(kn, dim3((unsigned)p.grid), dim3(p.block), 0, s, a);
  if (e != hipSuccess || a.nchunk <= 1) return e;
  if (a.mew < 1 || a.mew > 64 || (a.mew & (a.mew - 1))) return hipErrorInvalidValue;
  return launch_kernel(k_fold_merge, dim3((unsigned)((a.nout + a.mew - 1) / a.mew)), dim3(kBlock),
                       0, s, a);
}

int64_t plan_unfold(UnfoldArgs &a, bool vec) {
  a.vec = vec && a.nfpc % 4 == 0;
  const int64_t total = a.nc / (a.vec ? 4 : 1) * a.ni * a.nt;
  const int64_t wgs = (total + kBlock - 1) / kBlock;
  return wgs < (1 << 20) ? wgs : (1 << 20);  // grid-stride beyond
}

hipError_t launch_unfold(const UnfoldArgs &a, int64_t grid, hipStream_t s) {
  if (grid <= 0) return hipSuccess;
  const dim3 g((unsigned)grid, (unsigned)a.nbank);
  return a.vec ? launch_kernel(k_unfold<true>, g, dim3(kBlock), 0, s, a)
               : launch_kernel(k_unfold<false>, g, dim3(kBlock), 0, s, a);
}

}  // namespace bldp
