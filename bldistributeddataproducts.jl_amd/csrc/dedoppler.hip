// dedoppler.hip — drift-rate sums of every channel of a Float32 window (gfx950).
//
// T selected spectra make a block; drift d in -D .. D moves off(d, t) =
// sign(d) * floor((2|d|t + (T-1)) / (2(T-1))) selected channels at spectrum t of
// the block.  S[c, i, b, d] is the Float32 sum over t = 0 .. T-1, in that order
// and from +0.0f, of W[c + off(d, t), i, b*T + t]; a term whose channel leaves
// the segment of c (seg channels each, the last one shorter; the whole window
// when seg is 0) is skipped.  best / drift are the isless-greatest sum and its d
// over the scan 0, -1, +1, ..., -D, +D: the first NaN wins, else the first of the
// greatest (argext's BLDP_ARG_MAX rule).
//
// A workgroup of C lanes takes C neighbouring channels of one (bank, IF, block),
// a lane a channel.  R rows of the tile with H >= D channels of halo on each side
// lie in LDS (RW = C + 2H words a row): lane l reads word H + l + off of row t, so
// neighbouring lanes read neighbouring words for every (d, t).  A lane keeps the
// sums of kMag magnitudes |d|, both signs, in registers (G = 2 kMag drifts a
// group; d = 0 rides in the first group), folds them into its running best in
// scan order and goes on to the next group: no merge, no atomics, no workspace.
//   resident  R = T: the block's rows are staged once, the groups loop over them.
//   chunked   R < T: the groups are outermost, the rows are staged R at a time
//             and read again for every group.
// Both add a sum's terms in the order t = 0 .. T-1, so they agree bit for bit.
// The path is stepped: off += (2|d|) div q, the remainder carries (q = 2(T-1));
// it is wave-uniform.  A skipped term adds +0.0f instead: a sum that starts from
// +0.0f is never -0.0f, so that changes no bit.  A tile that no path leaves (no
// segment or window edge within D of it) takes the body without the per-lane
// bounds.
//   k_dedoppler<true>   rows staged by 16-byte loads (unit step, aligned)
//   k_dedoppler<false>  rows staged a dword at a time (any step and offset)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bldp_impl.h"

namespace bldp {
namespace {

constexpr int kMag = 4;                    // magnitudes a group: G = 2 * kMag drifts
constexpr int64_t kLdsSmall = 64 * 1024;   // a chunk, and a resident block that fits
constexpr int64_t kLdsLarge = 160 * 1024;  // a resident block at the most (one workgroup a CU)

// isless order as unsigned order, every NaN the greatest (argext's arg_key)
__device__ __forceinline__ uint32_t dd_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return x != x ? 0xffffffffu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

struct Best {
  float v;
  uint32_t key;
  int32_t d;
  // a strictly greater key only: the first NaN, else the first of the greatest
  __device__ __forceinline__ void take(float x, int32_t dx) {
    const uint32_t k = dd_key(x);
    if (k > key) key = k, v = x, d = dx;
  }
};

// rows [t0, t0 + nr) of the tile at channel c0 into sh: word j of a row is channel
// c0 - H + j, +0.0f outside the window
template <bool VEC>
__device__ __forceinline__ void dd_stage(const DedopArgs &a, float *sh, const float *in,
                                         int64_t c0, int64_t t0, int nr) {
  const uint32_t RW = (uint32_t)a.RW, C = blockDim.x;
  if (VEC) {
    const uint32_t RW4 = RW / 4, total = (uint32_t)nr * RW4;
    for (uint32_t e = threadIdx.x; e < total; e += C) {
      const uint32_t row = e / RW4, j = e - row * RW4;
      const int64_t ch = c0 - a.H + 4 * (int64_t)j;
      const float *p = in + ch + (t0 + row) * a.in_ld_t;
      float4 v;
      if (ch >= 0 && ch + 3 < a.nc) {
        v = *reinterpret_cast<const float4 *>(p);
      } else {
        v.x = (ch >= 0 && ch < a.nc) ? p[0] : 0.0f;
        v.y = (ch + 1 >= 0 && ch + 1 < a.nc) ? p[1] : 0.0f;
        v.z = (ch + 2 >= 0 && ch + 2 < a.nc) ? p[2] : 0.0f;
        v.w = (ch + 3 >= 0 && ch + 3 < a.nc) ? p[3] : 0.0f;
      }
      *reinterpret_cast<float4 *>(sh + (size_t)row * RW + 4 * j) = v;
    }
  } else {
    const uint32_t total = (uint32_t)nr * RW;
    for (uint32_t e = threadIdx.x; e < total; e += C) {
      const uint32_t row = e / RW, j = e - row * RW;
      const int64_t ch = c0 - a.H + (int64_t)j;
      sh[e] = (ch >= 0 && ch < a.nc) ? in[ch * a.in_cs + (t0 + row) * a.in_ld_t] : 0.0f;
    }
  }
}

// The wave-uniform paths of a group's magnitudes: off(m, t) and its remainder.
struct Paths {
  int32_t off[kMag], rem[kMag], sq[kMag], sr[kMag];
};

// nr staged rows added to a group's sums; lane word `lane` = sh + H + tid.  CHECK:
// a term is taken when amin <= off <= amax (the lane's segment, clipped to +-D).
template <bool CHECK, bool ZERO>
__device__ __forceinline__ void dd_rows(const float *lane, int nr, int32_t RW, int32_t q, Paths &p,
                                        float &s0, float *sn, float *sp, int32_t amin,
                                        int32_t amax) {
  for (int tt = 0; tt < nr; ++tt, lane += RW) {
    float xn[kMag], xp[kMag];
#pragma unroll
    for (int g = 0; g < kMag; ++g) xn[g] = lane[-p.off[g]], xp[g] = lane[p.off[g]];
    if (ZERO) {
      const float x0 = lane[0];
      s0 += (!CHECK || amax >= 0) ? x0 : 0.0f;
    }
#pragma unroll
    for (int g = 0; g < kMag; ++g) {
      if (CHECK) {
        xn[g] = -p.off[g] >= amin ? xn[g] : 0.0f;
        xp[g] = p.off[g] <= amax ? xp[g] : 0.0f;
      }
      sn[g] += xn[g];
      sp[g] += xp[g];
      p.off[g] += p.sq[g];
      p.rem[g] += p.sr[g];
      if (p.rem[g] >= q) p.rem[g] -= q, ++p.off[g];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(1024) void k_dedoppler(const DedopArgs a) {
  extern __shared__ __align__(16) float sh[];
  const int32_t tid = (int32_t)threadIdx.x, C = (int32_t)blockDim.x;
  const int32_t D = a.D, RW = a.RW, T = (int32_t)a.T, R = a.R;
  const int32_t q = 2 * (T - 1);
  const int64_t c0 = (int64_t)blockIdx.x * C, c = c0 + tid;
  const bool active = c < a.nc;
  // the lane's segment [lo, hi) as the offsets it may take; no offset for an idle lane
  const int64_t seg = a.seg > 0 ? a.seg : (a.nc > 0 ? a.nc : 1);
  int32_t amin = 1, amax = -1;
  if (active) {
    const int64_t lo = c / seg * seg, hi = lo + seg < a.nc ? lo + seg : a.nc;
    amin = lo - c < -(int64_t)D ? -D : (int32_t)(lo - c);
    amax = hi - 1 - c > (int64_t)D ? D : (int32_t)(hi - 1 - c);
  }
  // no path of the tile leaves its segment (wave-uniform)
  bool inner = false;
  if (c0 + C <= a.nc) {
    const int64_t lo = c0 / seg * seg, hi = lo + seg < a.nc ? lo + seg : a.nc;
    inner = c0 - D >= lo && c0 + C - 1 + D < hi;
  }
  const int ngroups = D > 0 ? (D + kMag - 1) / kMag : 1;
  const float *lane = sh + a.H + tid;
  const float *bank = a.in[blockIdx.z] + a.in_off;
  const int64_t nrows = a.ni * a.nb;
  for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
    const int64_t i = r % a.ni, b = r / a.ni;
    const float *in = bank + i * a.in_ld_i + b * a.T * a.in_ld_t;
    const int64_t o = (int64_t)blockIdx.z * a.out_bank + c + i * a.out_ld_i + b * a.out_ld_t;
    Best best{0.0f, 0u, 0};
    for (int grp = 0; grp < ngroups; ++grp) {
      const int32_t m0 = 1 + grp * kMag;
      Paths p;
      float s0 = 0.0f, sn[kMag], sp[kMag];
#pragma unroll
      for (int g = 0; g < kMag; ++g) {
        // (a magnitude beyond D walks D's path again and is not written)
        const uint32_t m2 = 2u * (uint32_t)(m0 + g <= D ? m0 + g : D);
        p.sq[g] = (int32_t)(m2 / (uint32_t)q), p.sr[g] = (int32_t)(m2 % (uint32_t)q);
        p.off[g] = 0, p.rem[g] = T - 1;
        sn[g] = 0.0f, sp[g] = 0.0f;
      }
      for (int32_t t0 = 0; t0 < T; t0 += R) {
        const int nr = T - t0 < R ? T - t0 : R;
        if (R < T || grp == 0) {
          __syncthreads();  // (the rows' readers of the last chunk, group or block)
          dd_stage<VEC>(a, sh, in, c0, t0, nr);
          __syncthreads();
        }
        if (grp == 0) {
          if (inner)
            dd_rows<false, true>(lane, nr, RW, q, p, s0, sn, sp, amin, amax);
          else
            dd_rows<true, true>(lane, nr, RW, q, p, s0, sn, sp, amin, amax);
        } else {
          if (inner)
            dd_rows<false, false>(lane, nr, RW, q, p, s0, sn, sp, amin, amax);
          else
            dd_rows<true, false>(lane, nr, RW, q, p, s0, sn, sp, amin, amax);
        }
      }
      // the group's sums, in scan order
      if (grp == 0) {
        best.v = s0, best.key = dd_key(s0), best.d = 0;
        if (a.sums && active) a.sums[o + (int64_t)D * a.out_ld_q] = s0;
      }
#pragma unroll
      for (int g = 0; g < kMag; ++g) {
        const int32_t m = m0 + g;
        if (m > D) break;
        best.take(sn[g], -m);
        best.take(sp[g], m);
        if (a.sums && active) {
          a.sums[o + (int64_t)(D - m) * a.out_ld_q] = sn[g];
          a.sums[o + (int64_t)(D + m) * a.out_ld_q] = sp[g];
        }
      }
    }
    if (a.best && active) a.best[o] = best.v, a.drift[o] = best.d;
  }
}

}  // namespace

int plan_dedoppler(DedopArgs &a, bool vec, Plan *p) {
  // the tile grows while the halo of both sides exceeds it
  int32_t C = 256;
  while (C < 1024 && 2 * a.D > C) C *= 2;
  a.C = C;
  a.vec = vec;
  a.H = vec ? (a.D + 3) / 4 * 4 : a.D;
  a.RW = C + 2 * a.H;
  const int64_t row = 4 * (int64_t)a.RW, all = row * a.T;
  int64_t lds;
  if (all <= kLdsLarge) {
    a.R = (int32_t)a.T;
    lds = all;
  } else {
    a.R = (int32_t)(kLdsSmall / row);  // >= 5: a row is 12 KiB at the most
    lds = a.R * row;
  }
  a.tiles = (a.nc + C - 1) / C;
  const int64_t rows = a.ni * a.nb;
  if (a.tiles * C > (int64_t)UINT32_MAX)
    return set_error(BLDP_EINVAL, "dedoppler: %lld workgroups along the channels are too many "
                     "for one launch", (long long)a.tiles);
  p->path = a.R == a.T ? DEDOP_RESIDENT : DEDOP_CHUNKED;
  p->lpg = C;
  p->grid = a.tiles * rows;
  p->gx = (uint32_t)a.tiles;
  p->gy = (uint32_t)(rows < 65535 ? rows : 65535);  // (the kernel strides beyond)
  p->gz = (uint32_t)a.nbank;
  p->block = (uint32_t)C;
  p->shm = (uint32_t)lds;
  p->nout = a.nc * rows;
  p->ws_bytes = 0;
  p->kernel = vec ? DEDOP_K_VEC : DEDOP_K_SCALAR;
  p->nrw = a.D > 0 ? (a.D + kMag - 1) / kMag : 1;  // groups
  return BLDP_OK;
}

int dedoppler_group() { return 2 * kMag; }

hipError_t launch_dedoppler(const DedopArgs &a, const Plan &p, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  if (a.T < 2 || a.D < 0 || a.D > BLDP_MAX_DRIFT || a.H < a.D || a.R < 1 || a.R > a.T)
    return hipErrorInvalidValue;
  if (p.block != (uint32_t)a.C || a.RW != a.C + 2 * a.H ||
      (int64_t)p.shm != 4 * (int64_t)a.RW * a.R || (int64_t)p.shm > kLdsLarge)
    return hipErrorInvalidValue;
  if (a.vec && (a.H % 4 || a.in_cs != 1)) return hipErrorInvalidValue;
  if ((a.best == nullptr) != (a.drift == nullptr) || (!a.best && !a.sums))
    return hipErrorInvalidValue;
  const dim3 g(p.gx, p.gy, p.gz);
  return a.vec ? launch_kernel(k_dedoppler<true>, g, dim3(p.block), p.shm, s, a)
               : launch_kernel(k_dedoppler<false>, g, dim3(p.block), p.shm, s, a);
}

}  // namespace bldp
